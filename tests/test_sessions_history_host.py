"""CPU tests of the undo history of edit sessions (ian_sessions_reserve_history, ian_session_mark, ian_session_undo,
ian_session_history): the bookkeeping model npe_ops.SessionHistory against a naive list-and-cursor model, the C++ header
csrc/ian_session_history.h (compiled into a stand-alone program under AddressSanitizer and UBSan) against SessionHistory, the header /
export list agreement, and the packer (every validation before any library call)."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from neural_photo_editor_amd import api, npe_ops as N
from neural_photo_editor_amd import lib as L
from session_helpers import HEADER, ROOT, header_code, run_c, stub_sessions

NEW_EXPORTS = ("ian_sessions_reserve_history", "ian_session_mark", "ian_session_undo", "ian_session_history")
DEPTHS = (1, 2, 3, 16)
CSRC = os.path.join(ROOT, "neural_photo_editor_amd", "csrc")


class NaiveHistory:
    """The specification without a ring: a Python list of states and a cursor.  States are whatever the caller hands in."""

    def __init__(self, depth):
        self.depth, self.E, self.c = depth, [], 0

    undoable = property(lambda self: self.c)
    redoable = property(lambda self: len(self.E) - 1 - self.c if self.c < len(self.E) else 0)

    def mark(self, live):
        del self.E[self.c:]
        if len(self.E) == self.depth:
            del self.E[0]
        self.E.append(live)
        self.c = len(self.E)

    def undo(self, k, live):
        if self.c == len(self.E):
            self.E.append(live)
        self.c -= k
        return self.E[self.c]

    def redo(self, k):
        self.c += k
        return self.E[self.c]

    def edited(self):
        if self.c < len(self.E):
            del self.E[self.c + 1:]
            self.c = len(self.E)
            if len(self.E) > self.depth:          # depth + 1 entries before the cursor: the oldest goes
                del self.E[0]
                self.c -= 1

    def clear(self):
        self.E, self.c = [], 0


def script(depth, seed, count=3000):
    """A random operation script: (op, k).  Undo / redo steps are drawn a little past what is available, so refusals are in it; edits
    happen with and without a mark before them; a clear now and then.  A deep ring gets more marks, so that it fills and drops too."""
    rs = random.Random(seed)
    ops = []
    p_mark = 0.30 if depth <= 3 else 0.45
    for _ in range(count):
        r = rs.random()
        if r < p_mark:
            ops.append(("m", 0))
        elif r < 0.55:
            ops.append(("u", rs.randint(1, min(depth, 3) + 1)))
        elif r < 0.75:
            ops.append(("r", rs.randint(1, min(depth, 3) + 1)))
        elif r < 0.995:
            ops.append(("e", 0))
        else:
            ops.append(("c", 0))
    return ops


def run_model(depth, ops):
    """SessionHistory over `ops` -> the lines the C++ driver prints for them."""
    H = N.SessionHistory(depth)
    out = []
    for op, k in ops:
        if op == "m":
            head = "m %d" % H.mark()
        elif op == "u" and 1 <= k <= H.undoable:
            head = "u %d %d" % H.undo(k)
        elif op == "r" and 1 <= k <= H.redoable:
            head = "r %d" % H.redo(k)
        elif op == "e":
            H.edited()
            head = "e"
        elif op == "c":
            H.clear()
            head = "c"
        else:
            with pytest.raises(ValueError):
                (H.undo if op == "u" else H.redo)(k)
            head = "x"
        out.append("%s %d %d" % (head, H.undoable, H.redoable))
    return out


# ---- 1. the model against a list and a cursor ------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_session_history_equals_a_list_and_a_cursor(depth):
    H, M = N.SessionHistory(depth), NaiveHistory(depth)
    slots = {}                  # physical slot -> the state saved there
    used = set()
    live = 0                    # a state is a number; every edit makes a new one
    fresh = 1
    counts = {"undo": 0, "redo": 0, "refused": 0, "dropped": 0, "max_undo": 0}
    for step, (op, k) in enumerate(script(depth, 100 + depth)):
        if op == "m":
            before = M.undoable
            s = H.mark()
            slots[s] = live
            used.add(s)
            M.mark(live)
            counts["dropped"] += int(M.undoable == before)
        elif op == "u":
            if not 1 <= k <= M.undoable:
                counts["refused"] += 1
                with pytest.raises(ValueError):
                    H.undo(k)
            else:
                tip = M.c == len(M.E)
                save, load = H.undo(k)
                assert (save >= 0) == tip, step
                if save >= 0:
                    slots[save] = live
                    used.add(save)
                assert load in slots and load != save, (step, "a slot is loaded before it was written")
                live = slots[load]
                assert live == M.undo(k, live if save < 0 else slots[save]), step
                counts["undo"] += 1
        elif op == "r":
            if not 1 <= k <= M.redoable:
                counts["refused"] += 1
                with pytest.raises(ValueError):
                    H.redo(k)
            else:
                load = H.redo(k)
                assert load in slots, (step, "a slot is loaded before it was written")
                live = slots[load]
                assert live == M.redo(k), step
                counts["redo"] += 1
        elif op == "e":
            live, fresh = fresh, fresh + 1
            H.edited()
            M.edited()
        else:
            H.clear()
            M.clear()
            slots.clear()       # nothing saved before a clear may be read after it
        assert (H.undoable, H.redoable) == (M.undoable, M.redoable), step
        assert 0 <= H.undoable <= depth and 0 <= H.redoable <= depth, step
        counts["max_undo"] = max(counts["max_undo"], H.undoable)
    assert used <= set(range(depth + 1)), used
    # the script reached what it is there for
    assert counts["undo"] > 100 and counts["redo"] > 30 and counts["refused"] > 100 and counts["dropped"] > 10, counts
    assert counts["max_undo"] == depth, counts


def test_session_history_by_hand():
    H = N.SessionHistory(2)
    assert (H.undoable, H.redoable) == (0, 0)
    a, b = H.mark(), H.mark()
    assert a != b and H.undoable == 2
    c = H.mark()                                       # depth 2: the first mark is dropped, its slot is not the new one
    assert H.undoable == 2 and c not in (b,)
    save, load = H.undo(1)
    assert save not in (b, c) and load == c and (H.undoable, H.redoable) == (1, 1)
    assert H.undo(1) == (-1, b) and (H.undoable, H.redoable) == (0, 2)
    with pytest.raises(ValueError):
        H.undo(1)
    assert H.redo(2) == save and (H.undoable, H.redoable) == (2, 0)
    H.undo(2)
    H.edited()                                         # the redo tail goes, the state come back to stays an undo target
    assert (H.undoable, H.redoable) == (1, 0)
    H.edited()                                         # at the tip an edit changes nothing
    assert (H.undoable, H.redoable) == (1, 0)
    H.clear()
    assert (H.undoable, H.redoable) == (0, 0)
    for bad in (0, 65, -1):
        with pytest.raises(ValueError):
            N.SessionHistory(bad)


# ---- 2. the C++ header against the model -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def history_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("history") / "session_history"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "session_history_main.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("depth", DEPTHS)
def test_cpp_header_equals_the_model(history_program, depth):
    ops = script(depth, 200 + depth)
    text = "%d\n" % depth + "".join("%s %d\n" % (op, k) if op in "ur" else op + "\n" for op, k in ops)
    r = subprocess.run([history_program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.split("\n")[:-1]
    want = run_model(depth, ops)
    assert len(got) == len(want) == len(ops)
    for step, (g, w) in enumerate(zip(got, want)):
        assert g == w, (step, ops[step], g, w)
    assert sum(l.startswith("x") for l in got) > 100 and sum(l.startswith("u") for l in got) > 100


# ---- 3. header and loader --------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99_with_the_new_declarations(tmp_path):
    """The program defines the four functions itself: a definition that disagreed with the header's declaration would not compile."""
    lines = run_c(tmp_path, [
        '#include <stdio.h>', '#include "ian.h"',
        'int ian_sessions_reserve_history(ian_handle* h, int32_t d) { (void)h; return d; }',
        'int ian_session_mark(ian_handle* h, int32_t n, const int32_t* i, void* s) { (void)h; (void)i; (void)s; return n; }',
        'int ian_session_undo(ian_handle* h, int32_t n, const int32_t* i, const int32_t* k, uint8_t* o, void* s) {',
        '  (void)h; (void)i; (void)k; (void)o; (void)s; return n; }',
        'int ian_session_history(ian_handle* h, int32_t id, int32_t out[3]) { (void)h; out[0] = out[1] = out[2] = id; return 0; }',
        'int main(void) {',
        '  int32_t out[3];',
        '  ian_session_history(0, 7, out);',
        '  printf("%d %d %d %d\\n", ian_sessions_reserve_history(0, 16), ian_session_mark(0, 3, 0, 0), ian_session_undo(0, 2, 0, 0, 0, 0), (int)out[2]);',
        '  return 0;', '}'])
    assert lines == ["16 3 2 7"]


def test_header_and_export_list_agree_on_the_new_names():
    code = header_code()
    declared = set(re.findall(r"\b(ian_[a-z_0-9]+)\s*\(", code))
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS, name
        assert not name.endswith("_local") and not any(w in name for w in ("hires", "render", "view")), name
    lib = L.load_library()
    protos = {name: argt for _, name, argt in L.parse_header_prototypes(HEADER)}
    for name in NEW_EXPORTS:
        fn = getattr(lib, name)                        # exported by the built library
        assert fn.restype is ctypes.c_int32
        assert len(fn.argtypes) == len(protos[name]), name
    assert protos["ian_session_undo"] == ["ptr", "int32_t", "ptr", "ptr", "ptr", "ptr"]
    assert protos["ian_session_history"] == ["ptr", "int32_t", "ptr"]


# ---- 4. EditSessions over a stub -------------------------------------------------------------------------------------------------
def history_stub(**kw):
    s, h = stub_sessions(args=True, **kw)
    s.reserve_history(4)
    assert h.calls == [("sessions_reserve_history", (4,))] and s.history_depth == 4
    h.calls.clear()
    return s, h


def test_packer():
    ids, st = api.pack_session_undo([3, 1, 2])
    assert ids.dtype == np.int32 and st.dtype == np.int32 and list(ids) == [3, 1, 2] and list(st) == [1, 1, 1]
    assert list(api.pack_session_undo([3, 1], 2)[1]) == [2, 2]
    assert list(api.pack_session_undo([3, 1, 0], [1, -2, 64])[1]) == [1, -2, 64]
    assert list(api.pack_session_undo(5, np.int64(3))[1]) == [3]


def test_valid_calls_reach_the_library_with_the_packed_arrays():
    s, h = history_stub()
    s.mark([2, 0])
    (name, (ids,)), = h.calls
    assert name == "session_mark" and ids.dtype == np.int32 and list(ids) == [2, 0]
    h.calls.clear()
    shown = s.undo([2, 0, 3])                          # steps = 1 for every session
    (name, (ids, steps, out)), = h.calls
    assert name == "session_undo" and ids.dtype == np.int32 and steps.dtype == np.int32
    assert list(ids) == [2, 0, 3] and list(steps) == [1, 1, 1]
    assert out is shown and shown.shape == (3, 3, 64, 64) and shown.dtype == np.uint8
    h.calls.clear()
    s.undo([1, 3], [2, 1])
    s.redo([1, 3], [2, 1])                             # redo negates
    s.redo([0])
    assert [list(c[1][1]) for c in h.calls] == [[2, 1], [-2, -1], [-1]]
    assert all(c[0] == "session_undo" and c[1][1].dtype == np.int32 for c in h.calls)
    h.calls.clear()
    s.reserve(6)                                       # reserve and close keep working
    assert s.history_depth == 4 and [c[0] for c in h.calls] == ["sessions_reserve"]
    s.reserve_history(0)
    assert s.history_depth == 0
    s.reserve_history(2)
    s.close()
    assert s.history_depth == 0 and h.calls[-1] == ("sessions_reserve", (0,))


@pytest.mark.parametrize("call", [
    lambda s: s.mark([0, 1, 0]),                                             # an id given twice
    lambda s: s.mark([0, 8]),                                                # an id out of range
    lambda s: s.mark([-1]),
    lambda s: s.mark([4]),                                                   # a session not opened
    lambda s: s.mark([]),                                                    # n = 0
    lambda s: s.mark(list(range(257))),
    lambda s: s.mark([0.5]),
    lambda s: s.undo([0, 1, 0]),
    lambda s: s.undo([0, 8]),
    lambda s: s.undo([4]),
    lambda s: s.undo([]),
    lambda s: s.undo(list(range(257))),
    lambda s: s.undo([0], 0),                                                # zero steps
    lambda s: s.undo([0, 1], [1, 0]),
    lambda s: s.redo([0], 0),
    lambda s: s.undo([0], 1.0),                                              # steps are integers
    lambda s: s.undo([0], [1.5]),
    lambda s: s.redo([0, 1], [1.0, 2.0]),
    lambda s: s.undo([0], True),
    lambda s: s.undo([0, 1], [1]),                                           # one per session
    lambda s: s.undo([0], [[1]]),
    lambda s: s.undo([0], 65),                                               # beyond any depth
    lambda s: s.redo([0], 2 ** 31),
    lambda s: s.history(8),
    lambda s: s.history(4),
    lambda s: s.reserve_history(65),
    lambda s: s.reserve_history(-1),
])
def test_invalid_input_raises_before_any_library_call(call):
    s, h = history_stub()
    with pytest.raises(ValueError):
        call(s)
    assert h.calls == []


@pytest.mark.parametrize("call", [lambda s: s.mark([0]), lambda s: s.undo([0]), lambda s: s.redo([0]), lambda s: s.history(0)])
def test_without_the_reservation_the_calls_are_refused(call):
    s, h = stub_sessions(args=True)
    with pytest.raises(ValueError, match="no history reservation"):
        call(s)
    assert h.calls == []

"""ian_session_stroke on the host: the declaration and the loader, the two structs as strict C99 against their ctypes mirrors, the brush
rectangle and the stroke's footprint of npe_ops against the reference's expressions, pack_session_strokes (sorting, bookkeeping,
every refusal before the library is reached) and EditSessions.stroke / paint_stroke over a stub."""
import ctypes
import re

import numpy as np
import pytest

from neural_photo_editor_amd import api, npe_ops as N
from neural_photo_editor_amd import lib as L
from session_helpers import HEADER, StubHandle, header_code, run_c, stub_sessions

NEW_EXPORTS = ("ian_session_stroke",)


# ---- 1. header and loader ----------------------------------------------------------------------------------------------------------
def test_header_and_export_list_agree_on_the_new_name():
    declared = set(re.findall(r"\b(ian_[a-z_0-9]+)\s*\(", header_code()))
    assert {n for n in declared if "stroke" in n} == set(NEW_EXPORTS)
    assert {n for n in L.EXPORTS if "stroke" in n} == set(NEW_EXPORTS)
    for n in NEW_EXPORTS:       # the patterns the other session tests hold their own names to
        assert not ("hires" in n or "render" in n or "view" in n or "canvas" in n or n.endswith("_local") or n.endswith("_fit")), n
    assert re.search(r"#define\s+IAN_STROKE_MAX_POINTS\s+64\b", open(HEADER).read()) and L.STROKE_MAX_POINTS == 64
    lib = L.load_library()
    protos = {name: argt for _, name, argt in L.parse_header_prototypes(HEADER)}
    assert protos["ian_session_stroke"] == ["ptr", "int32_t", "ptr", "int32_t", "ptr", "int32_t", "ptr", "ptr"]
    fn = lib.ian_session_stroke                        # exported by the built library
    assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == 8
    assert fn.argtypes[1] is ctypes.c_int32 and fn.argtypes[3] is ctypes.c_int32 and fn.argtypes[5] is ctypes.c_int32
    st, bx = (L.SessionStroke * 1)(), (L.StrokeBox * 1)()
    assert fn(None, 1, st, 1, bx, 0, None, None) != 0  # a null handle is an error, not a crash


def test_struct_layouts_and_prototype_match_the_header(tmp_path):
    """The program defines the function itself: a definition that disagreed with the header's declaration would not compile."""
    assert ctypes.sizeof(L.StrokeBox) == 20 and ctypes.sizeof(L.SessionStroke) == 32
    assert [(f, getattr(L.StrokeBox, f).offset) for f, _ in L.StrokeBox._fields_] == [("c1", 0), ("r1", 4), ("c2", 8), ("r2", 12), ("gscale", 16)]
    assert [(f, getattr(L.SessionStroke, f).offset) for f, _ in L.SessionStroke._fields_] == \
        [("session", 0), ("first", 4), ("count", 8), ("mode", 12), ("coef", 16), ("rgb", 20)]
    lines = run_c(tmp_path, [
        '#include <stdio.h>', '#include <stddef.h>', '#include "ian.h"',
        'int ian_session_stroke(ian_handle* h, int32_t n, const ian_session_stroke_item* strokes, int32_t nboxes,',
        '                       const ian_stroke_box* boxes, int32_t flags, uint8_t* shown, void* stream) {',
        '  (void)h; (void)strokes; (void)boxes; (void)shown; (void)stream; return n + nboxes + flags; }',
        'int main(void) {',
        '  ian_session_stroke_item s; ian_stroke_box b;',
        '  s.rgb[2] = 0.5f; b.gscale = 2.0f; (void)s; (void)b;',
        '  printf("%d %d %d %d %d %d\\n", (int)sizeof(ian_stroke_box), (int)offsetof(ian_stroke_box, c1), (int)offsetof(ian_stroke_box, r1),',
        '         (int)offsetof(ian_stroke_box, c2), (int)offsetof(ian_stroke_box, r2), (int)offsetof(ian_stroke_box, gscale));',
        '  printf("%d %d %d %d %d %d %d\\n", (int)sizeof(ian_session_stroke_item), (int)offsetof(ian_session_stroke_item, session),',
        '         (int)offsetof(ian_session_stroke_item, first), (int)offsetof(ian_session_stroke_item, count),',
        '         (int)offsetof(ian_session_stroke_item, mode), (int)offsetof(ian_session_stroke_item, coef),',
        '         (int)offsetof(ian_session_stroke_item, rgb));',
        '  printf("%d %d\\n", IAN_STROKE_MAX_POINTS, ian_session_stroke(0, 3, 0, 20, 0, 1, 0, 0));',
        '  return 0;', '}'])
    assert lines == ["20 0 4 8 12 16", "32 0 4 8 12 16 20", "64 24"]


# ---- 2. the brush rectangle and the footprint of a stroke -----------------------------------------------------------------------------
def test_brush_rect_is_move_mouse_for_every_point_and_brush_size():
    for d in (0, 3, 12, 64):
        for x in range(64):
            for y in range(64):
                brush_width = ((d // 4) + 1)                                             # NPE.py:149
                xmin = max(min(x - brush_width // 2, 64 - brush_width), 0)              # NPE.py:152
                xmax = xmin + brush_width
                ymin = max(min(y - brush_width // 2, 64 - brush_width), 0)              # NPE.py:155
                ymax = ymin + brush_width
                got = N.brush_rect(x, y, d)
                assert got == (xmin, ymin, xmax, ymax), (x, y, d)
                assert 0 <= got[0] < got[2] <= 64 and 0 <= got[1] < got[3] <= 64
    assert N.brush_rect(np.int64(63), 0.0, 12) == (60, 0, 64, 4)


def test_stroke_footprint_is_sequential_umask_paint_in_any_order():
    rs = np.random.RandomState(4)
    t = N.local_falloff_table()
    boxes = np.array([N.brush_rect(x, y, d) for x, y, d in zip(rs.randint(0, 64, 9), rs.randint(0, 64, 9), rs.randint(0, 65, 9))])
    boxes[4, 2] = boxes[4, 0]                                                             # an empty rectangle adds nothing
    U0 = rs.uniform(0, 1, (64, 64)) * (rs.uniform(0, 1, (64, 64)) < 0.3)
    want = U0.copy()
    for b in boxes:
        want = N.umask_paint(want, b, t)
    got = N.stroke_footprint(U0, boxes, t)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(N.stroke_footprint(U0, boxes[rs.permutation(9)], t), want)
    assert np.array_equal(N.stroke_footprint(U0, np.concatenate([boxes, boxes[:3]]), t), want)
    assert np.array_equal(N.stroke_footprint(U0, np.delete(boxes, 4, axis=0), t), want)
    assert np.array_equal(N.stroke_footprint(U0, boxes[4:5], t), U0) and got is not U0
    assert got.max() == 1.0 and np.all(got >= U0)


# ---- 3. pack_session_strokes ------------------------------------------------------------------------------------------------------------
def paths_of(counts, seed=0):
    rs = np.random.RandomState(seed)
    out = []
    for k in counts:
        c1, r1 = rs.randint(0, 50, k), rs.randint(0, 50, k)
        out.append(np.stack([c1, r1, c1 + rs.randint(0, 14, k), r1 + rs.randint(1, 14, k)], axis=1))
    return out


def test_packer_sorts_stably_and_keeps_the_books():
    ids = [7, 2, 5, 0, 3]
    paths = paths_of((2, 3, 1, 3, 2), 1)
    cols = np.array([(10, 20, 30), (40, 50, 60), (70, 80, 90), (100, 110, 120), (130, 140, 150)])
    strokes, boxes, perm = api.pack_session_strokes(ids, paths, cols, [1, 0, 1, 1, 1], weight=[0.05, 0.1, 0.05, 0.2, 0.3],
                                                    sign=[-1, 1, -1, -1, -1])
    assert perm == [1, 3, 0, 4, 2]                                                        # descending count, ties in the caller's order
    assert [s.session for s in strokes] == [2, 0, 7, 3, 5]
    assert [s.count for s in strokes] == [3, 3, 2, 2, 1] and len(boxes) == 11
    assert [s.first for s in strokes] == [0, 3, 6, 8, 10]
    assert [s.mode for s in strokes] == [0, 1, 1, 1, 1]
    for s, i in zip(strokes, perm):
        for k in range(s.count):
            b = boxes[s.first + k]
            assert (b.c1, b.r1, b.c2, b.r2) == tuple(int(v) for v in paths[i][k])
            assert b.gscale == float(1 + (b.c2 - b.c1))
        assert [s.rgb[c] for c in range(3)] == [float(v) for v in api.brush_colour(cols[i])]
    # coef as pack_session_events rounds it: the float64 product stored into a float32 field
    ev = api.pack_session_events(ids, np.array([p[0] for p in paths]), cols, [1, 0, 1, 1, 1], [0.05, 0.1, 0.05, 0.2, 0.3], [-1, 1, -1, -1, -1])
    assert [s.coef for s in strokes] == [ev[i].coef for i in perm]
    assert strokes[0].coef == float(np.float32(0.1)) and strokes[4].coef == float(np.float32(-0.05))
    # the defaults: no colours, every mode 0; one colour and scalars for all; floats truncated as int() does
    strokes, boxes, perm = api.pack_session_strokes([4], [[(1.9, 2.2, 5.7, 6.0)]])
    assert (strokes[0].mode, strokes[0].first, strokes[0].count, perm) == (0, 0, 1, [0])
    assert (boxes[0].c1, boxes[0].r1, boxes[0].c2, boxes[0].r2, boxes[0].gscale) == (1, 2, 5, 6, 5.0)
    strokes, _, _ = api.pack_session_strokes([4, 1], np.zeros((2, 3, 4), int) + (0, 0, 4, 4), (1, 2, 3))
    assert [s.mode for s in strokes] == [1, 1] and [s.count for s in strokes] == [3, 3]
    assert strokes[0].coef == float(np.float32(-0.05))


@pytest.mark.parametrize("call", [
    lambda s: s.stroke([0, 1], [np.zeros((0, 4), int), [(0, 0, 4, 4)]], (1, 2, 3)),          # an empty path
    lambda s: s.stroke([0, 1], [[(0, 0, 4, 4)]] * 2 + [[(0, 0, 4, 4)]], (1, 2, 3)),           # three paths for two sessions
    lambda s: s.stroke([0], [np.tile((0, 0, 4, 4), (65, 1))], (1, 2, 3)),                     # more than 64 points
    lambda s: s.stroke([0, 1], [[(0, 0, 4, 4)], [(0, 0, 4, 4), (10, 10, 65, 20)]], (1, 2, 3)),  # a rectangle outside the image
    lambda s: s.stroke([0, 1], [[(0, 0, 4, 4)], [(-1, 0, 4, 4)]], (1, 2, 3)),
    lambda s: s.stroke([0], [[(0, 0, 4)]], (1, 2, 3)),                                        # not (K, 4)
    lambda s: s.stroke([0, 1], [[(0, 0, 4, 4)]] * 2, None, [1, 0]),                           # mode 1 without a colour
    lambda s: s.stroke([0, 1], [[(0, 0, 4, 4)]] * 2, (1, 2, 3), [2, 0]),
    lambda s: s.stroke([1, 1], [[(0, 0, 4, 4)]] * 2, (1, 2, 3)),                              # an id twice
    lambda s: s.stroke([0, 5], [[(0, 0, 4, 4)]] * 2, (1, 2, 3)),                              # an unopened session
    lambda s: s.stroke([0, 8], [[(0, 0, 4, 4)]] * 2, (1, 2, 3)),                              # outside the pool
    lambda s: s.stroke([], [], (1, 2, 3)),
    lambda s: s.stroke([0], [[(0, 0, 4, 4)]], (1, 2, 3), mark=True),                          # no history reservation
    lambda s: s.paint_stroke([0], [[(1, 2, 3)]], (1, 2, 3), mark=False),                      # points are (K, 2)
])
def test_invalid_input_raises_before_any_library_call(call):
    s, h = stub_sessions()
    with pytest.raises(ValueError):
        call(s)
    assert h.calls == []


# ---- 4. EditSessions.stroke / paint_stroke over a stub ----------------------------------------------------------------------------------
class FillingStub(StubHandle):
    """A stub whose session_stroke answers: row j of shown is filled with the session id of sorted stroke j."""

    def session_stroke(self, strokes, boxes, flags, shown):
        self.calls.append(("session_stroke", (strokes, boxes, flags, shown)))
        for j, s in enumerate(strokes):
            shown[j] = s.session


def test_stroke_unpermutes_shown_and_paint_stroke_builds_the_same_arrays():
    h = FillingStub(args=True)
    s = api.EditSessions(h, 8, 100)
    s._opened = {0, 1, 2, 3}
    h.calls.clear()
    ids = [3, 0, 2]
    paths = paths_of((1, 3, 2), 2)
    shown = s.stroke(ids, paths, (200, 100, 50))
    (name, (strokes, boxes, flags, _)), = h.calls
    assert name == "session_stroke" and flags == 0 and [st.session for st in strokes] == [0, 2, 3] and len(boxes) == 6
    assert shown.shape == (3, 3, 64, 64) and shown.dtype == np.uint8
    assert [int(shown[i, 0, 0, 0]) for i in range(3)] == ids and all(np.all(shown[i] == ids[i]) for i in range(3))
    # paint_stroke: brush_rect per point, then stroke; mark=True is its default and needs the reservation
    pts = [np.array([(10, 12), (11, 13), (63, 0)]), np.array([(0, 63)]), np.array([(30, 30), (31, 29)])]
    with pytest.raises(ValueError):
        s.paint_stroke(ids, pts, (200, 100, 50))
    s.reserve_history(4)
    h.calls.clear()
    a = s.paint_stroke(ids, pts, (200, 100, 50), d=12, weight=0.07)
    b = s.stroke(ids, [np.array([N.brush_rect(x, y, 12) for x, y in p]) for p in pts], (200, 100, 50), None, 0.07, -1.0, mark=True)
    (_, (s1, b1, f1, _)), (_, (s2, b2, f2, _)) = h.calls
    assert f1 == f2 == 1 and bytes(s1) == bytes(s2) and bytes(b1) == bytes(b2) and np.array_equal(a, b)
    assert [st.session for st in s1] == [3, 2, 0] and [st.count for st in s1] == [3, 2, 1]
    assert (b1[2].c1, b1[2].r1, b1[2].c2, b1[2].r2) == (60, 0, 64, 4) and s1[0].coef == float(np.float32(-0.07))

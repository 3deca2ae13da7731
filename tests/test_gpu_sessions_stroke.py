"""Strokes (ian_session_stroke; EditSessions.stroke / paint_stroke): a session's whole brush path in one submission.  The oracle is the
literal loop of the header -- for each k, `brush` on the strokes with more than k points, in sorted order -- run on the SAME model
handle and the SAME pool as the stroke, on a second range of ids opened from the same photos, so that both sides share every tuned
kernel choice.  Every comparison is np.array_equal, on `shown` and on every field read() returns."""
import ctypes as C

import numpy as np
import pytest

from neural_photo_editor_amd import lib as L
from neural_photo_editor_amd import npe_ops as N
from oracle import ian_oracle as O
import session_helpers as H
from session_helpers import model_pool, refused

pytestmark = pytest.mark.gpu

CAP = 18                # ids 16 and 17 are never opened
COLOURS = np.array([(250, 20, 20), (10, 240, 90), (30, 30, 200), (200, 200, 10), (90, 10, 160)])

_cache = {}


def pool_of(arch="IAN_simple"):
    """(model, pool): one per architecture; a test that needs a reservation makes it and frees it again."""
    if arch not in _cache:
        _cache[arch] = model_pool(arch, capacity=CAP)
    return _cache[arch]


def random_paths(counts, seed, empty=None):
    """One (K,4) array of rectangles inside the image per count; empty = (stroke, point) of one rectangle with c2 == c1."""
    rs = np.random.RandomState(seed)
    paths = []
    for i, k in enumerate(counts):
        c1, r1 = rs.randint(0, 56, k), rs.randint(0, 56, k)
        p = np.stack([c1, r1, c1 + rs.randint(1, 9, k), r1 + rs.randint(1, 9, k)], axis=1)
        if empty is not None and empty[0] == i:
            p[empty[1], 2] = p[empty[1], 0]
        paths.append(p)
    return paths


def per_stroke(v, n):
    a = np.asarray(v, np.float64)
    return [float(a)] * n if a.ndim == 0 else [float(t) for t in a]


def oracle_loop(pool, ids, paths, colours, modes, weight, sign):
    """The header's loop on strokes that are already sorted by descending count -> what each session's last event displayed."""
    n = len(ids)
    counts = [len(p) for p in paths]
    assert counts == sorted(counts, reverse=True)
    w, sg = per_stroke(weight, n), per_stroke(sign, n)
    last = [None] * n
    for k in range(counts[0]):
        act = [i for i in range(n) if counts[i] > k]
        shown = pool.brush([ids[i] for i in act], np.array([paths[i][k] for i in act]), np.array([colours[i] for i in act]),
                           [modes[i] for i in act], [w[i] for i in act], [sg[i] for i in act])
        for j, i in enumerate(act):
            last[i] = shown[j]
    return np.stack(last)


def assert_sessions_equal(pool, ids_o, ids_s, tag):
    for a, b in zip(ids_o, ids_s):
        want, got = pool.read(a), pool.read(b)
        assert set(want) == set(got), (tag, a, b)
        for k in want:
            assert np.array_equal(got[k], want[k]), (tag, k, a, b)


def run_both(pool, ids_o, ids_s, paths, colours, modes, weight=0.3, sign=-1.0, mark=False, tag=None):
    """The oracle on ids_o, the stroke on ids_s; the arguments are in the CALLER's order (any counts): the oracle gets them sorted
    stably by descending count, the stroke as they are.  Asserts shown and every field equal -> shown in the caller's order."""
    n = len(ids_s)
    perm = sorted(range(n), key=lambda i: -len(paths[i]))
    w, sg = per_stroke(weight, n), per_stroke(sign, n)
    pick = lambda v: [v[i] for i in perm]
    if mark:
        pool.mark(pick(ids_o))
    want = oracle_loop(pool, pick(ids_o), pick(paths), pick(colours), pick(modes), pick(w), pick(sg))
    got = pool.stroke(ids_s, paths, np.asarray(colours), modes, w, sg, mark=mark)
    assert got.shape == (n, 3, 64, 64) and got.dtype == np.uint8
    for j, i in enumerate(perm):
        assert np.array_equal(got[i], want[j]), (tag, "shown", i)
    assert_sessions_equal(pool, ids_o, ids_s, tag)
    return got


def open_twice(pool, ids_o, ids_s, seed, hires=0):
    ph = H.sources(len(ids_o), hires or 1, seed)
    for ids in (ids_o, ids_s):
        (pool.open_hires if hires else pool.open)(ids, ph)
    return ph


# ---- 1. a ragged batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_ragged_batch_of_mixed_strokes_equals_the_loop_of_brush_calls(arch):
    """Counts (2, 3, 1) in the caller's order (the library sees (3, 2, 1)): two paint strokes, one lighten stroke with sign +1, one session
    in sample mode, one empty rectangle in the middle of the longest stroke."""
    _, pool = pool_of(arch)
    ids_o, ids_s = [1, 4, 7], [9, 12, 15]
    open_twice(pool, ids_o, ids_s, 21)
    z = O.make_latents(1, seed=5)
    pool.sample([ids_o[0]], z)
    pool.sample([ids_s[0]], z)
    paths = random_paths((2, 3, 1), 31, empty=(1, 1))
    got = run_both(pool, ids_o, ids_s, paths, COLOURS[:3], [1, 1, 0], weight=[0.3, 0.3, 0.2], sign=[-1.0, -1.0, 1.0], tag=arch)
    before = pool.read(ids_s[1])
    assert before["MODE"] == 0 and pool.read(ids_s[0])["MODE"] == 1
    assert np.array_equal(got[1], before["IM"])                          # a paint stroke on a photo-mode session stores its blend
    assert not np.array_equal(before["IM"], before["GIM"])               # and the stroke did change the picture


# ---- 2. the smallest call, and the residency --------------------------------------------------------------------------------------------
def test_one_point_is_one_brush_and_the_next_stroke_reuses_the_activations():
    _, pool = pool_of()
    a, b = [3], [11]
    open_twice(pool, a, b, 22)
    box = np.array([(20, 18, 33, 31)])
    col = COLOURS[:1]
    want = [pool.brush(a, box, col, weight=0.3), pool.brush(a, box + 3, col, weight=0.3)]   # the second one hits the residency
    wa = pool.read(a[0])
    want.append(pool.brush(a, box - 5, col, weight=0.3))                                     # a read keeps it
    got = [pool.stroke(b, [box], col, weight=0.3), pool.stroke(b, [box + 3], col, weight=0.3)]
    gb = pool.read(b[0])
    got.append(pool.stroke(b, [box - 5], col, weight=0.3))
    for k in range(3):
        assert np.array_equal(got[k], want[k]), k
    for k in wa:
        assert np.array_equal(gb[k], wa[k]), k
    assert_sessions_equal(pool, a, b, "after the third")
    # a stroke after a brush of the same session, and a brush after a stroke: the residency passes both ways
    want = [pool.brush(a, box + k, col, weight=0.3) for k in range(3)]
    got = [pool.brush(b, box, col, weight=0.3), pool.stroke(b, [box + 1], col, weight=0.3), pool.brush(b, box + 2, col, weight=0.3)]
    for k in range(3):
        assert np.array_equal(got[k], want[k]), ("mixed", k)
    assert_sessions_equal(pool, a, b, "mixed")


# ---- 3. the longest stroke, and the refusal past it ----------------------------------------------------------------------------------------
def raw_strokes(rows, nboxes, box=(4, 4, 12, 12)):
    """ctypes arrays straight for the library: rows = (session, first, count) per stroke, paint mode; every box the same."""
    st = (L.SessionStroke * len(rows))()
    for s, (sid, first, count) in zip(st, rows):
        s.session, s.first, s.count, s.mode, s.coef = sid, first, count, 1, -0.3
        s.rgb[0], s.rgb[1], s.rgb[2] = 0.5, -0.25, 0.0
    bx = (L.StrokeBox * nboxes)()
    for b in bx:
        b.c1, b.r1, b.c2, b.r2 = box
        b.gscale = float(1 + box[2] - box[0])
    return st, bx


def test_64_points_in_one_call_and_65_are_refused():
    m, pool = pool_of()
    a, b = [2], [10]
    open_twice(pool, a, b, 23)
    run_both(pool, a, b, random_paths((L.STROKE_MAX_POINTS,), 33), COLOURS[:1], [1], weight=0.1, tag="K = 64")
    before = pool.read(b[0])
    shown = np.full((1, 3, 64, 64), 7, np.uint8)
    st, bx = raw_strokes([(b[0], 0, 65)], 65)
    refused(lambda: m.handle.session_stroke(st, bx, 0, shown), r"item 0: count 65 outside 1\.\.64", -7)
    after = pool.read(b[0])
    assert np.all(shown == 7) and set(after) == set(before)
    for k in before:
        assert np.array_equal(after[k], before[k]), k


# ---- 4. several passes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_brush_pass_2_splits_five_strokes_into_three_passes_on_both_sides(arch):
    m, pool = pool_of(arch)
    ids_o, ids_s = [0, 1, 2, 3, 4], [8, 9, 10, 11, 12]
    open_twice(pool, ids_o, ids_s, 24)
    m.handle.set_option("brush_pass", 2)
    try:
        run_both(pool, ids_o, ids_s, random_paths((3, 3, 2, 2, 1), 34), COLOURS, [1, 1, 0, 1, 1], sign=[-1, -1, 1, -1, -1], tag=arch)
    finally:
        m.handle.set_option("brush_pass", 256)


# ---- 5. local edits ----------------------------------------------------------------------------------------------------------------------
def test_local_edits_the_user_mask_holds_every_point_of_the_stroke():
    """Flags 1, 3, 2 and 0 on four paint strokes of 4, 3, 2 and 1 points; then a sample-mode session and a lighten stroke, both with the
    local flag, whose UMASK must stay as it was."""
    _, pool = pool_of()
    pool.reserve_local()
    try:
        t = N.local_falloff_table()
        ids_o, ids_s = [0, 1, 2, 3], [8, 9, 10, 11]
        open_twice(pool, ids_o, ids_s, 25)
        flags = [1, 3, 2, 0]
        pool.set_local(ids_o, flags=flags)
        pool.set_local(ids_s, flags=flags)
        paths = random_paths((4, 3, 2, 1), 35, empty=(0, 2))
        run_both(pool, ids_o, ids_s, paths, COLOURS[:4], [1, 1, 1, 1], tag="local")       # UMASK and LOCAL are among the fields compared
        for sid, fl, p in zip(ids_s, flags, paths):
            U = pool.read(sid)["UMASK"]
            assert np.array_equal(U, N.stroke_footprint(np.zeros((64, 64)), p, t) if fl & 1 else np.zeros((64, 64))), (sid, fl)
        # a second stroke adds to the mask of the first
        more = random_paths((4, 3, 2, 1), 36)
        run_both(pool, ids_o, ids_s, more, COLOURS[:4], [1, 1, 1, 1], tag="local, second stroke")
        U = pool.read(ids_s[0])["UMASK"]
        assert np.array_equal(U, N.stroke_footprint(N.stroke_footprint(np.zeros((64, 64)), paths[0], t), more[0], t))
        # sample mode, and a lighten stroke: no footprint
        z = O.make_latents(1, seed=6)
        pool.sample([ids_o[0]], z)
        pool.sample([ids_s[0]], z)
        pool.set_local(ids_o[:2], flags=1)                                               # clears UMASK
        pool.set_local(ids_s[:2], flags=1)
        run_both(pool, ids_o[:2], ids_s[:2], random_paths((3, 2), 37), COLOURS[:2], [1, 0], sign=[-1.0, 1.0], tag="no footprint")
        for sid in ids_s[:2]:
            assert not pool.read(sid)["UMASK"].any(), sid
    finally:
        pool.reserve_local(False)


# ---- 6. full resolution ------------------------------------------------------------------------------------------------------------------
def test_full_resolution_field_kind_and_a_rendered_window_after_the_stroke():
    _, pool = pool_of()
    pool.reserve_hires(2)
    try:
        ids_o, ids_s = [5, 6], [13, 14]
        open_twice(pool, ids_o, ids_s, 26, hires=2)
        run_both(pool, ids_o, ids_s, random_paths((3, 2), 38), COLOURS[:2], [1, 0], sign=[-1.0, 1.0], tag="hires")   # FIELD, FIELD_KIND, SOURCE
        assert [pool.read(i)["FIELD_KIND"] for i in ids_s] == [0, 1]
        assert np.array_equal(pool.render(ids_s, (32, 40), (64, 48)), pool.render(ids_o, (32, 40), (64, 48)))
    finally:
        pool.reserve_hires(0)


# ---- 7. history --------------------------------------------------------------------------------------------------------------------------
def test_mark_first_makes_one_stroke_one_undo_step():
    m, pool = pool_of()
    ids_o, ids_s = [0, 1, 2], [8, 9, 10]
    open_twice(pool, ids_o, ids_s, 27)
    st, bx = raw_strokes([(ids_s[0], 0, 2)], 2)
    refused(lambda: m.handle.session_stroke(st, bx, 1, None), "no history reservation", -6)
    pool.reserve_history(4)
    try:
        hist = lambda ids: [pool.history(i) for i in ids]
        run_both(pool, ids_o, ids_s, random_paths((3, 2, 1), 39), COLOURS[:3], [1, 1, 0], sign=[-1, -1, 1], mark=True, tag="marked")
        assert hist(ids_s) == hist(ids_o) == [{"depth": 4, "undo": 1, "redo": 0}] * 3
        run_both(pool, ids_o, ids_s, random_paths((2, 2, 2), 40), COLOURS[:3], [1, 1, 1], mark=True, tag="marked twice")
        assert hist(ids_s) == hist(ids_o) == [{"depth": 4, "undo": 2, "redo": 0}] * 3
        assert np.array_equal(pool.undo(ids_s), pool.undo(ids_o))
        assert hist(ids_s) == hist(ids_o) == [{"depth": 4, "undo": 1, "redo": 1}] * 3
        assert_sessions_equal(pool, ids_o, ids_s, "undone")
        # an unmarked stroke from an undone state: `edited`, once on one side and three times on the other
        run_both(pool, ids_o, ids_s, random_paths((3, 3, 1), 41), COLOURS[:3], [1, 1, 1], tag="edited")
        assert hist(ids_s) == hist(ids_o)
        assert np.array_equal(pool.undo(ids_s), pool.undo(ids_o))
        assert_sessions_equal(pool, ids_o, ids_s, "undone again")
    finally:
        pool.reserve_history(0)


# ---- 8. refusals through the library ------------------------------------------------------------------------------------------------------
def test_refusals_name_the_item_and_change_nothing():
    import torch
    m, pool = pool_of()
    h = m.handle
    ids = [4, 5, 6]
    pool.open(ids, H.sources(3, 1, 28))
    pool.paint(ids, (10, 10, 30, 30), (200, 100, 50), weight=0.5)
    before = [pool.read(i) for i in ids]
    shown = np.full((3, 3, 64, 64), 7, np.uint8)

    def call(rows, nboxes, flags=0, edit=None):
        st, bx = raw_strokes(rows, nboxes)
        if edit:
            edit(st, bx)
        return lambda: h.session_stroke(st, bx, flags, shown)

    def outside(st, bx):
        bx[3 + 2].c2 = 65                                                 # item 1 starts at box 3: its point 2

    def device_boxes():
        st, bx = raw_strokes([(4, 0, 2)], 2)
        dev = torch.zeros(2 * C.sizeof(L.StrokeBox), dtype=torch.uint8, device="cuda")
        h._check(h.lib.ian_session_stroke(h._h, 1, st, 2, C.cast(dev.data_ptr(), C.POINTER(L.StrokeBox)), 0, L._ptr(shown), C.c_void_p(0)))

    def device_strokes():
        _, bx = raw_strokes([(4, 0, 2)], 2)
        dev = torch.zeros(C.sizeof(L.SessionStroke), dtype=torch.uint8, device="cuda")
        h._check(h.lib.ian_session_stroke(h._h, 1, C.cast(dev.data_ptr(), C.POINTER(L.SessionStroke)), 2, bx, 0, L._ptr(shown), C.c_void_p(0)))

    bad = [
        (r"item 1: count 3 after item 0's 2", call([(4, 0, 2), (5, 2, 3)], 5)),                     # counts that increase
        (r"item 1: rectangles 3\.\.5 outside the 5 boxes", call([(4, 0, 3), (5, 3, 3)], 5)),        # first + count past nboxes
        (r"item 1: rectangles -1\.\.0", call([(4, 0, 2), (5, -1, 2)], 4)),
        (r"item 1: point 2: patch \(4,4,65,12\)", call([(4, 0, 3), (5, 3, 3)], 6, edit=outside)),
        ("item 1: count 0", call([(4, 0, 2), (5, 2, 0)], 4)),
        ("flags 2", call([(4, 0, 2)], 2, flags=2)),                                                 # an unknown flag bit
        ("flags 5", call([(4, 0, 2)], 2, flags=5)),
        ("boxes must be a host array", device_boxes),
        ("must be a host array", device_strokes),
        ("item 1: session 4 already appears as item 0", call([(4, 0, 2), (4, 2, 2)], 4)),          # what the brush checks per item
        ("item 1: session 16 has not been opened", call([(4, 0, 2), (16, 2, 2)], 4)),
        ("item 0: session 18 outside the pool", call([(CAP, 0, 2)], 2)),
        ("item 0 has mode 2", call([(4, 0, 2)], 2, edit=lambda st, bx: setattr(st[0], "mode", 2))),
        ("n = 0", call([], 2)),
    ]
    for needle, c in bad:
        refused(c, needle, -7)
        assert np.all(shown == 7), needle
        for i, b in zip(ids, before):
            got = pool.read(i)
            assert set(got) == set(b)
            for k in b:
                assert np.array_equal(got[k], b[k]), (needle, i, k)
    # and the handle still works: the same strokes, sorted, are accepted
    call([(5, 0, 3), (4, 3, 2)], 5)()
    assert not np.any(np.all(shown[:2].reshape(2, -1) == 7, axis=1))

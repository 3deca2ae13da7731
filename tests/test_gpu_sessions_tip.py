"""Brush tips on the device (ian_sessions_set_tip, ian_session_brush_tip, ian_session_path_tip; EditSessions.brush / paint / stroke with
tips=): a weight per pixel in the place of the rectangle's flat 1/N.  Two models with the same parameters, each with its own pool of 9
sessions carrying every reservation (full resolution, local edits, history, tips), get the same photos; what one side does with tips
the other does by the means the library had before, and the comparisons are np.array_equal on shown and on every field read() returns
-- except where two different seeds are compared (linearity, the half tip), which hold the latents' gradient rows to TOL_GRAD."""
import ctypes as C
import os

import numpy as np
import pytest

from neural_photo_editor_amd import lib as L
from neural_photo_editor_amd import npe_ops as N
from oracle import ian_oracle as O
import session_helpers as H
from session_helpers import model_pool, refused
from test_gpu_brush_batch import TOL_GRAD, rel

pytestmark = pytest.mark.gpu

CAP = 9
NTIPS = 8
COLOURS = np.array([(250, 20, 20), (10, 240, 90), (30, 30, 200)])
BOXES = [(0, 0, 1, 1), (59, 61, 64, 64), (0, 0, 64, 64)]      # 1x1 in the corner; th x tw = 3x5 touching the right and bottom edges; whole
ASYM = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 0]], np.float64)  # not symmetric, one zero
HALF = np.zeros((4, 6), np.float32)
HALF[:, :3] = N.tip_weights(np.ones((4, 3)))
TIPS = {                                                        # tip -> (weights, normalise); tip 7 is never set
    0: (np.ones((1, 1)), True), 1: (np.ones((3, 5)), True), 2: (np.ones((64, 64)), True),
    3: (np.random.RandomState(7).uniform(0.1, 1, (3, 5)), True), 4: (ASYM, True), 5: (HALF, False), 6: (N.round_tip(9, 0.5), True),
}

_cache = {}


def set_tips(pool):
    pool.reserve_tips(NTIPS)
    for t, (w, norm) in TIPS.items():
        pool.set_tip(t, w, normalise=norm)


def pools(arch):
    """((model A, pool A), (model B, pool B)): the same parameters, every reservation on, the same tips."""
    if arch not in _cache:
        pair = []
        for _ in range(2):
            m, pool = model_pool(arch, capacity=CAP)
            pool.reserve_hires(2)
            pool.reserve_local()
            pool.reserve_history(4)
            set_tips(pool)
            pair.append((m, pool))
        _cache[arch] = pair
    return _cache[arch]


def open_both(arch, ids, seed, flags=1, same_photo=False):
    ph = H.sources(1 if same_photo else len(ids), 2, seed)
    if same_photo:
        ph = np.repeat(ph, len(ids), axis=0)
    for _, pool in pools(arch):
        pool.open_hires(ids, ph)
        pool.set_local(ids, flags=flags)


def assert_same(pa, pb, ids, tag, history=False):
    for i in ids:
        want, got = pa.read(i), pb.read(i)
        assert set(want) == set(got) and {"FIELD", "UMASK", "SOURCE"} <= set(want), (tag, i)
        for k in want:
            assert np.array_equal(got[k], want[k]), (tag, i, k)
        if history:
            assert pa.history(i) == pb.history(i), (tag, i)


def latent_grads(m, n):
    """The latents' gradient rows the last backward sweep left: dz before the fused update (dense_bwd_gemv_batch_kernel stores it first)."""
    return m.handle.read_slot_grad(m.lowered.z_slot, n).reshape(n, -1).astype(np.float64)


# ---- 1. an all-ones tip is the rectangle brush ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_ones_tip_is_the_rectangle_brush_bit_for_bit(arch):
    """Rests on 1.f / cnt being the correctly rounded quotient on the host (npe_ops.tip_weights) and on the device (seed_inv)."""
    (_, A), (_, B) = pools(arch)
    ids = [0, 4, 8]
    for t, (c1, r1, c2, r2) in enumerate(BOXES):
        assert np.all(B.tip(t) == np.float32(1) / np.float32(3 * (r2 - r1) * (c2 - c1))) and B.tip(t).shape == (r2 - r1, c2 - c1)
    for mode in (1, 0):
        open_both(arch, ids, 41 + mode)
        before = [A.read(i)["Z"] for i in ids]
        col, sign = (COLOURS, -1.0) if mode else (None, [1.0, -1.0, 1.0])
        sa = A.brush(ids, BOXES, col, None, 0.1, sign)
        sb = B.brush(ids, BOXES, col, None, 0.1, sign, tips=[0, 1, 2])
        assert np.array_equal(sa, sb), (arch, mode)
        assert_same(A, B, ids, (arch, mode))
        for i, z in zip(ids, before):
            assert not np.array_equal(A.read(i)["Z"], z), (arch, mode, i)      # the events did move the latents
        if mode:
            assert all(B.read(i)["UMASK"].any() for i in ids)                  # the rectangle's footprint, on both sides


# ---- 2. tip -1 is the plain event ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_items_without_a_tip_are_the_plain_call_at_the_same_n(arch):
    (_, A), (_, B) = pools(arch)
    ids = [1, 2, 3]
    boxes = [(5, 6, 20, 30), (59, 61, 64, 64), (40, 0, 64, 9)]
    open_both(arch, ids, 43)
    sa = A.brush(ids, boxes, COLOURS, [1, 1, 0], 0.2, [-1.0, -1.0, 1.0])
    sb = B.brush(ids, boxes, COLOURS, [1, 1, 0], 0.2, [-1.0, -1.0, 1.0], tips=[-1, 3, -1])
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[2], sb[2])
    assert_same(A, B, [1, 3], arch)
    assert not np.array_equal(A.read(2)["Z"], B.read(2)["Z"])                  # and the item between them did use its tip


# ---- 3. linearity against the existing gradient ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
@pytest.mark.parametrize("mode", [1, 0])
def test_tip_gradient_is_the_weighted_sum_of_the_one_pixel_gradients(arch, mode):
    """Nine sessions on one photo, the same 3x3 tip event on all nine; the reference is ian_grad_batch at n = 9 on the nine 1x1 boxes of
    that square at the same latents.  A 1x1 box seeds with inv = 1.f / 3.f where the tip seeds with wn[p], the same expression otherwise,
    so in float64 dz_tip = sum_p (wn[p] / inv) * dz_1x1[p].  Catches a transposed tip, a wrong origin, stride or normalisation."""
    (m, A), _ = pools(arch)
    ids = list(range(9))
    open_both(arch, ids, 44, flags=0, same_photo=True)
    Z = np.stack([A.read(i)["Z"] for i in ids])
    assert np.array_equal(Z, np.repeat(Z[:1], 9, axis=0))                      # one photo: one latent
    c1, r1 = 61, 0                                                             # touches the top and right edges
    levels = (250, 20, 90)
    A.brush(ids, (c1, r1, c1 + 3, r1 + 3), levels if mode else None, None, 0.1, -1.0 if mode else 1.0, tips=4)
    dz = latent_grads(m, 9)
    wn = N.tip_weights(ASYM)
    assert np.array_equal(A.tip(4), wn)
    px = [(c1 + p % 3, r1 + p // 3, c1 + p % 3 + 1, r1 + p // 3 + 1) for p in range(9)]
    rgb = np.repeat(H.const_rgb(levels)[None], 9, axis=0) if mode else None
    dz1 = m.imgrad_batch(np.array(px), Z, rgb).astype(np.float64)
    inv = np.float64(np.float32(1) / np.float32(3))                            # the float32 value of one third
    ref = sum((np.float64(wn[p // 3, p % 3]) / inv) * dz1[p] for p in range(9))
    assert np.abs(ref).max() > 0
    for i in range(9):
        e = rel(dz[i], ref)
        print("linearity", arch, "mode", mode, "row", i, "rel", e)
        assert e < TOL_GRAD, (arch, mode, i, e)


# ---- 4. a tip that is zero on its right half is the rectangle on its left half -----------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_half_tip_is_the_half_rectangle(arch):
    (ma, A), (mb, B) = pools(arch)
    for mode in (1, 0):
        open_both(arch, [2], 45, flags=0)
        col, sign = ((10, 240, 90), -1.0) if mode else (None, 1.0)
        A.brush([2], (10, 20, 13, 24), col, None, 0.1, sign)                   # the left three columns
        B.brush([2], (10, 20, 16, 24), col, None, 0.1, sign, tips=5)           # th x tw = 4x6, weights of ones((4, 3)) | zeros
        da, db = latent_grads(ma, 1)[0], latent_grads(mb, 1)[0]
        e = rel(db, da)
        print("half tip", arch, "mode", mode, "rel", e, "bitwise", bool(np.array_equal(da, db)))
        assert np.abs(da).max() > 0 and e < TOL_GRAD, (arch, mode, e)


# ---- 5. a path is the loop of tip events -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
@pytest.mark.parametrize("brush_pass,mark", [(256, False), (1, False), (256, True)])
def test_path_tip_equals_the_loop_of_brush_tip_calls(arch, brush_pass, mark):
    (ma, A), (mb, B) = pools(arch)
    ids, tips = [1, 5], [3, 6]
    paths = [np.array([N.tip_rect(x, y, 5, 3) for x, y in ((10, 12), (14, 13), (63, 63))]), np.array([N.tip_rect(30, 2, 9, 9)])]
    open_both(arch, ids, 46)
    for m in (ma, mb):
        m.handle.set_option("brush_pass", brush_pass)
    try:
        got = A.stroke(ids, paths, COLOURS[:2], None, 0.2, -1.0, mark=mark, tips=tips)
        if mark:
            B.mark(ids)
        first = B.brush(ids, [paths[0][0], paths[1][0]], COLOURS[:2], None, 0.2, -1.0, tips=tips)
        B.brush(ids[:1], [paths[0][1]], COLOURS[:1], None, 0.2, -1.0, tips=tips[:1])
        last = B.brush(ids[:1], [paths[0][2]], COLOURS[:1], None, 0.2, -1.0, tips=tips[:1])
    finally:
        for m in (ma, mb):
            m.handle.set_option("brush_pass", 256)
    assert np.array_equal(got[0], last[0]) and np.array_equal(got[1], first[1]), (arch, brush_pass, mark)
    assert_same(A, B, ids, (arch, brush_pass, mark), history=True)
    assert A.history(1) == {"depth": 4, "undo": 1 if mark else 0, "redo": 0}
    # the caller's order is kept when the library's is another: the one-point stroke first
    open_both(arch, ids, 47)
    got = A.stroke(ids[::-1], paths[::-1], COLOURS[:2][::-1], None, 0.2, -1.0, tips=tips[::-1])
    want = B.stroke(ids, paths, COLOURS[:2], None, 0.2, -1.0, tips=tips)
    assert np.array_equal(got[::-1], want)
    assert_same(A, B, ids, (arch, "reversed"))


# ---- 6. windows ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_paint_with_a_view_and_a_tip_is_paint_with_the_tip_then_render(arch):
    (_, A), (_, B) = pools(arch)
    ids, boxes = [0, 6], [N.tip_rect(20, 40, 9, 9), N.tip_rect(63, 0, 5, 3)]
    open_both(arch, ids, 48)
    view = ([(32, 40), (64, 0)], (64, 48))
    shown, out = A.paint(ids, boxes, COLOURS[:2], 0.3, view=view, tips=[6, 3])
    want = B.paint(ids, boxes, COLOURS[:2], 0.3, tips=[6, 3])
    assert np.array_equal(shown, want) and out.shape == (2, 3, 48, 64)
    assert np.array_equal(out, B.render(ids, *view))
    assert_same(A, B, ids, arch)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_item_and_change_nothing():
    import torch
    (m, A), _ = pools("IAN_simple")
    h = m.handle
    ids = [3, 4]
    open_both("IAN_simple", ids, 49)
    A.paint(ids, (10, 10, 30, 30), (200, 100, 50), weight=0.3)
    before = [A.read(i) for i in ids]
    tip1 = A.tip(1)
    shown = np.full((2, 3, 64, 64), 7, np.uint8)

    def events(boxes):
        ev = H.session_events(ids)
        for e, b in zip(ev, boxes):
            e.c1, e.r1, e.c2, e.r2 = b
        return ev

    fit = [(59, 61, 64, 64), (0, 0, 5, 3)]                                     # both 5 wide, 3 high: tips 1 and 3

    def brush(tips, boxes=fit):
        return lambda: h.session_brush_tip(events(boxes), np.array(tips, np.int32), shown)

    def path(tips, boxes):
        st = (L.SessionStroke * 1)()
        st[0].session, st[0].first, st[0].count, st[0].mode, st[0].coef = ids[0], 0, len(boxes), 1, -0.3
        bx = (L.StrokeBox * len(boxes))()
        for b, r in zip(bx, boxes):
            b.c1, b.r1, b.c2, b.r2 = r
            b.gscale = 6.0
        return lambda: h.session_path_tip(st, np.array(tips, np.int32), bx, 0, shown[:1])

    def device_tips():
        dev = torch.zeros(2, dtype=torch.int32, device="cuda")
        h._check(h.lib.ian_session_brush_tip(h._h, 2, events(fit), C.c_void_p(dev.data_ptr()), L._ptr(shown), None, 0, 0, None, C.c_void_p(0)))

    def null_tips():
        h._check(h.lib.ian_session_brush_tip(h._h, 2, events(fit), None, L._ptr(shown), None, 0, 0, None, C.c_void_p(0)))

    def device_weights():
        dev = torch.ones(15, dtype=torch.float32, device="cuda")
        h._check(h.lib.ian_sessions_set_tip(h._h, 1, 5, 3, C.c_void_p(dev.data_ptr())))

    def weights(value):
        w = np.ones((3, 5), np.float32)
        w[2, 4] = value                                                        # the last one
        return lambda: h.sessions_set_tip(1, w)

    def size(tw, th):
        w = np.ones(65 * 65, np.float32)
        return lambda: h._check(h.lib.ian_sessions_set_tip(h._h, 1, tw, th, L._ptr(w)))

    bad = [
        (r"item 1: tip 8 outside -1\.\.7", brush([1, NTIPS])),
        (r"item 0: tip -2 outside -1\.\.7", brush([-2, 1])),
        ("item 1: tip 7 has never been set", brush([1, 7])),
        (r"item 1: patch \(0,0,5,3\) is not the 9 x 9 of tip 6", brush([1, 6])),
        (r"item 0: patch \(59,61,64,63\) is not the 5 x 3 of tip 1", brush([1, -1], [(59, 61, 64, 63), (0, 0, 5, 3)])),
        (r"item 0: patch \(61,59,64,64\) is not the 5 x 3 of tip 3", brush([3, -1], [(61, 59, 64, 64), (0, 0, 5, 3)])),   # transposed
        (r"item 0: point 1: patch \(0,0,5,4\) is not the 5 x 3 of tip 1", path([1], [(0, 0, 5, 3), (0, 0, 5, 4)])),
        ("item 0: point 0: tip 7 has never been set", path([7], [(0, 0, 5, 3)])),
        ("the tips must be a host array", device_tips),
        ("null tips array", null_tips),
        ("item 1: session 3 already appears as item 0",                        # what the plain call refuses
         lambda: h.session_brush_tip(H.session_events([3, 3], (0, 0, 5, 3)), np.array([1, 1], np.int32), shown)),
        (r"weight \[2\]\[4\] = -1 is not a finite number >= 0", weights(-1.0)),
        (r"weight \[2\]\[4\] = nan", weights(np.nan)),
        (r"weight \[2\]\[4\] = inf", weights(np.inf)),
        ("wn must be a host array", device_weights),
        (r"size 65 x 3", size(65, 3)), (r"size 5 x 0", size(5, 0)),
        ("tip 8 outside the reservation", lambda: h.sessions_set_tip(NTIPS, np.ones((2, 2), np.float32))),
        ("tip 7 has never been set", lambda: h.sessions_tip(7)),
        (r"count 65 outside 0\.\.64", lambda: h.sessions_reserve_tips(65)),
    ]

    def unchanged(needle):
        assert np.all(shown == 7), needle
        for i, b in zip(ids, before):
            got = A.read(i)
            assert set(got) == set(b)
            for k in b:
                assert np.array_equal(got[k], b[k]), (needle, i, k)

    for needle, c in bad:
        refused(c, needle, -7)
        unchanged(needle)
        assert np.array_equal(A.tip(1), tip1), needle
    # without the reservation: -6, from every call that needs it
    try:
        A.reserve_tips(0)
        for c in (brush([1, 3]), brush([-1, -1]), path([1], [(0, 0, 5, 3)]), weights(1.0), lambda: h.sessions_tip(1)):
            refused(c, "no tip reservation", -6)
        unchanged("no reservation")
        h.session_brush(events(fit), shown)                                    # and the plain call goes on without it
        assert not np.any(np.all(shown.reshape(2, -1) == 7, axis=1))
    finally:
        set_tips(A)
    # the handle still works: the same events, with their tips, are accepted; an all-zero tip moves nothing
    z = [A.read(i)["Z"] for i in ids]
    A.set_tip(7, np.zeros((3, 5)), normalise=False)
    try:
        brush([7, 1])()
        assert np.array_equal(A.read(ids[0])["Z"], z[0]) and not np.array_equal(A.read(ids[1])["Z"], z[1])
    finally:
        A.reserve_tips(0)                                                      # a new reservation forgets tip 7
        set_tips(A)
    refused(lambda: h.sessions_tip(7), "tip 7 has never been set", -7)


# ---- 8. residency --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_tip_and_plain_events_share_the_resident_activations(arch):
    (_, A), (_, B) = pools(arch)
    ids, boxes = [2, 7], [N.tip_rect(20, 40, 9, 9), N.tip_rect(50, 10, 9, 9)]
    open_both(arch, ids, 50)

    def three(pool):
        return [pool.paint(ids, boxes, COLOURS[:2], 0.2, tips=6), pool.paint(ids, boxes, COLOURS[:2], 0.2),
                pool.paint(ids, boxes, COLOURS[:2], 0.2, tips=[6, -1])]

    got = three(A)                                                             # the second and third call hit the residency
    assert "IAN_NO_DEC_CACHE" not in os.environ
    os.environ["IAN_NO_DEC_CACHE"] = "1"
    try:
        want = three(B)                                                        # every call gathers and runs the forward
    finally:
        del os.environ["IAN_NO_DEC_CACHE"]
    for k in range(3):
        assert np.array_equal(got[k], want[k]), (arch, k)
    assert_same(A, B, ids, arch)

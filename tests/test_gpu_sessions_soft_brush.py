"""Soft brushes end to end, on the device: the weighted clone (EditSessions.clone / restore with tips=), the user mask
shaped by the tip (EditSessions.tip_footprint) and tips on a whole photo (brush_compose with tips=).  Two models with the same
parameters, each with its own pool of 9 sessions carrying every reservation (full resolution, local edits, history, tips), get the
same photos; what one side does by the new means the other does by the means the library had before, or the numpy specification of
npe_ops says what must come out.  The comparisons are np.array_equal on shown and on every field read() returns -- except where two
different seeds are compared (linearity, the half tip), which hold the latents' gradient rows to TOL_GRAD."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from neural_photo_editor_amd import api
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
TABLE, GAUSS, THRESH = N.local_falloff_table(), N.gaussian_half_kernel(), 0.75

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


@contextlib.contextmanager
def footprint(*on):
    """The tip-shaped user mask switched on for these pools, and off again whatever happens: the pools are shared."""
    try:
        for p in on:
            assert p.tip_footprint(True) is True
        yield
    finally:
        for p in on:
            p.tip_footprint(False)


def assert_same(pa, pb, ids, tag, history=False, ids_b=None):
    for i, j in zip(ids, ids_b or ids):
        want, got = pa.read(i), pb.read(j)
        assert set(want) == set(got) and {"FIELD", "UMASK", "SOURCE"} <= set(want), (tag, i)
        for k in want:
            assert np.array_equal(got[k], want[k]), (tag, i, k)
        if history:
            assert pa.history(i) == pb.history(j), (tag, i)


def latent_grads(m, n):
    """The latents' gradient rows the last backward sweep left: dz before the fused update (dense_bwd_gemv_batch_kernel stores it first)."""
    return m.handle.read_slot_grad(m.lowered.z_slot, n).reshape(n, -1).astype(np.float64)


def moved_sources(arch, ids, seed):
    """Sessions `ids` opened and painted once on both sides, so that their GIM, IM and RECON are three different pictures."""
    open_both(arch, ids, seed, flags=0)
    for _, p in pools(arch):
        p.paint(ids, (8, 8, 56, 56), COLOURS[:len(ids)], weight=0.5)
    (_, A), _ = pools(arch)
    g = A.read(ids[0])
    assert not np.array_equal(g["IM"], g["GIM"]) and not np.array_equal(g["RECON"], g["GIM"])


# ==== the weighted clone ==================================================================================================================
# ---- 1. an all-ones tip is the plain clone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_ones_tip_clone_is_the_plain_clone_bit_for_bit(arch):
    (_, A), (_, B) = pools(arch)
    ids, src = [0, 4, 8], [1, 5, 7]
    offsets = [(3, 2), (-7, -20), (0, 0)]                                      # the whole picture has nowhere to shift to
    moved_sources(arch, src, 60)
    for field in ("GIM", "IM", "RECON"):
        for steps in (1, 3):
            open_both(arch, ids, 61)
            before = [A.read(i)["Z"] for i in ids]
            sa = A.clone(ids, BOXES, src, offsets, field, steps, 0.1)
            sb = B.clone(ids, BOXES, src, offsets, field, steps, 0.1, tips=[0, 1, 2])
            assert np.array_equal(sa, sb), (arch, field, steps)
            assert_same(A, B, ids, (arch, field, steps))
            for i, z in zip(ids, before):
                assert not np.array_equal(A.read(i)["Z"], z), (arch, field, steps, i)   # the events did move the latents
            assert all(B.read(i)["UMASK"].any() for i in ids)                  # the rectangle's footprint, on both sides


# ---- 2. tip -1 is the plain clone event --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_items_without_a_tip_are_the_plain_clone_at_the_same_n(arch):
    (_, A), (_, B) = pools(arch)
    ids, src = [1, 2, 3], [6, 6, 7]
    boxes = [(5, 6, 20, 30), (59, 61, 64, 64), (40, 0, 64, 9)]
    offs = [(-3, 1), (-3, -1), (-3, 1)]
    moved_sources(arch, [6, 7], 62)
    open_both(arch, ids, 63)
    sa = A.clone(ids, boxes, src, offs, "RECON", 2, 0.2)
    sb = B.clone(ids, boxes, src, offs, "RECON", 2, 0.2, tips=[-1, 3, -1])
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[2], sb[2])
    assert_same(A, B, [1, 3], arch)
    assert not np.array_equal(A.read(2)["Z"], B.read(2)["Z"])                  # and the item between them did use its tip


# ---- 3. linearity against the existing gradient ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_clone_tip_gradient_is_the_weighted_sum_of_the_one_pixel_gradients(arch):
    """Nine sessions on one photo, the same 3x3 clone event with the ASYM tip on all nine, each from its own GIM shifted by (-5, 7); the
    reference is ian_grad_batch at n = 9 on the nine 1x1 boxes of that square at the same latents with rgb = clone_target of the source.
    A 1x1 box seeds with inv = 1.f / 3.f where the tip seeds with wn[p], the same expression otherwise, so in float64
    dz_tip = sum_p (wn[p] / inv) * dz_1x1[p].  Catches a transposed tip, a wrong origin, stride, shift or normalisation."""
    (m, A), _ = pools(arch)
    ids = list(range(9))
    open_both(arch, ids, 64, flags=0, same_photo=True)
    Z = np.stack([A.read(i)["Z"] for i in ids])
    assert np.array_equal(Z, np.repeat(Z[:1], 9, axis=0))                      # one photo: one latent
    c1, r1, off = 61, 0, (-5, 7)                                               # touches the top and right edges
    box = (c1, r1, c1 + 3, r1 + 3)
    gim = A.read(0)["GIM"]
    A.clone(ids, box, ids, off, "GIM", 1, 0.1, tips=4)
    dz = latent_grads(m, 9)
    wn = N.tip_weights(ASYM)
    assert np.array_equal(A.tip(4), wn)
    px = [(c1 + p % 3, r1 + p // 3, c1 + p % 3 + 1, r1 + p // 3 + 1) for p in range(9)]
    rgb = np.repeat(N.clone_target(gim, box, off)[None], 9, axis=0)
    dz1 = m.imgrad_batch(np.array(px), Z, rgb).astype(np.float64)
    inv = np.float64(np.float32(1) / np.float32(3))                            # the float32 value of one third
    ref = sum((np.float64(wn[p // 3, p % 3]) / inv) * dz1[p] for p in range(9))
    assert np.abs(ref).max() > 0
    for i in range(9):
        e = rel(dz[i], ref)
        print("clone linearity", arch, "row", i, "rel", e)
        assert e < TOL_GRAD, (arch, i, e)


# ---- 4. a tip that is zero on its right half is the plain clone of its left half ---------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_half_tip_clone_is_the_clone_of_the_half_rectangle(arch):
    (ma, A), (mb, B) = pools(arch)
    moved_sources(arch, [4], 65)
    open_both(arch, [2], 66, flags=0)
    A.clone([2], (10, 20, 13, 24), [4], (5, -3), "IM", 1, 0.1)                 # the left three columns
    B.clone([2], (10, 20, 16, 24), [4], (5, -3), "IM", 1, 0.1, tips=5)         # th x tw = 4x6, weights of ones((4, 3)) | zeros
    da, db = latent_grads(ma, 1)[0], latent_grads(mb, 1)[0]
    e = rel(db, da)
    print("half tip clone", arch, "rel", e, "bitwise", bool(np.array_equal(da, db)))
    assert np.abs(da).max() > 0 and e < TOL_GRAD, (arch, e)


# ---- 5. steps = K is K calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
@pytest.mark.parametrize("brush_pass", [256, 1])
def test_four_steps_with_a_round_tip_are_four_calls(arch, brush_pass):
    (ma, A), (mb, B) = pools(arch)
    ids, src, tips = [1, 5], [7, 7], [6, 3]
    boxes = [N.tip_rect(20, 40, 9, 9), N.tip_rect(63, 63, 5, 3)]
    moved_sources(arch, [7], 67)
    open_both(arch, ids, 68)
    for m in (ma, mb):
        m.handle.set_option("brush_pass", brush_pass)
    try:
        got = A.clone(ids, boxes, src, (-2, -1), "IM", 4, 0.2, tips=tips)
        for _ in range(4):
            want = B.clone(ids, boxes, src, (-2, -1), "IM", 1, 0.2, tips=tips)
    finally:
        for m in (ma, mb):
            m.handle.set_option("brush_pass", 256)
    assert np.array_equal(got, want), (arch, brush_pass)
    assert_same(A, B, ids, (arch, brush_pass), history=True)


# ---- 6. restore ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_restore_with_tips_is_the_clone_from_the_sessions_own_photo(arch):
    (_, A), (_, B) = pools(arch)
    ids, boxes = [0, 6], [N.tip_rect(20, 40, 9, 9), N.tip_rect(63, 0, 5, 3)]
    open_both(arch, ids, 69)
    for _, p in pools(arch):
        p.paint(ids, (10, 0, 50, 60), COLOURS[:2], weight=0.5)
    z = [A.read(i)["Z"] for i in ids]
    sa = A.restore(ids, boxes, 2, 0.3, tips=[6, 3])
    sb = B.clone(ids, boxes, ids, (0, 0), "GIM", 2, 0.3, -1.0, tips=[6, 3])
    assert np.array_equal(sa, sb)
    assert_same(A, B, ids, arch)
    assert all(not np.array_equal(A.read(i)["Z"], q) for i, q in zip(ids, z))


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_item_and_change_nothing():
    import torch
    (m, A), _ = pools("IAN_simple")
    h = m.handle
    ids = [3, 4]
    open_both("IAN_simple", ids + [8], 70)
    A.paint(ids, (10, 10, 30, 30), (200, 100, 50), weight=0.3)
    before = [A.read(i) for i in ids]
    shown = np.full((2, 3, 64, 64), 7, np.uint8)
    fit = [(59, 61, 64, 64), (0, 0, 5, 3)]                                     # both 5 wide, 3 high: tips 1 and 3

    def events(boxes=fit):
        return api.pack_session_clones(ids, boxes, [8, 8], (0, 0), "GIM", 0.05, -1.0, capacity=CAP)

    def clone(tips, boxes=fit, steps=1):
        return lambda: h.session_clone_tip(events(boxes), np.array(tips, np.int32), steps, shown)

    def device_tips():
        dev = torch.zeros(2, dtype=torch.int32, device="cuda")
        h._check(h.lib.ian_session_stamp_soft(h._h, 2, events(), C.c_void_p(dev.data_ptr()), 1, L._ptr(shown), C.c_void_p(0)))

    def null_tips():
        h._check(h.lib.ian_session_stamp_soft(h._h, 2, events(), None, 1, L._ptr(shown), C.c_void_p(0)))

    bad = [
        (r"ian_session_stamp_soft: item 1: tip 8 outside -1\.\.7", clone([1, NTIPS])),
        (r"item 0: tip -2 outside -1\.\.7", clone([-2, 1])),
        ("item 1: tip 7 has never been set", clone([1, 7])),
        (r"item 1: patch \(0,0,5,3\) is not the 9 x 9 of tip 6", clone([1, 6])),
        (r"item 0: patch \(59,61,64,63\) is not the 5 x 3 of tip 1", clone([1, -1], [(59, 61, 64, 63), (0, 0, 5, 3)])),
        ("the tips must be a host array", device_tips),
        ("null tips array", null_tips),
        (r"steps = 65 outside 1\.\.64", clone([1, 3], steps=65)),              # what the plain call refuses
        (r"on = 2", lambda: h._check(h.lib.ian_sessions_set_soft_mask(h._h, 2))),
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
        assert A.tip_footprint() is False and h.sessions_tip_footprint() is False
    # without the reservation: -6, from the calls that need it; and the setting goes with the tips
    try:
        A.tip_footprint(True)
        assert h.sessions_tip_footprint() is True
        A.reserve_tips(0)
        assert h.sessions_tip_footprint() is False and A.tip_footprint() is False
        for c in (clone([1, 3]), clone([-1, -1]), lambda: h.sessions_set_tip_footprint(True)):
            refused(c, "no tip reservation", -6)
        with pytest.raises(ValueError, match="no tip reservation"):
            A.tip_footprint(True)
        unchanged("no reservation")
        h.session_clone(events(), 1, shown)                                    # and the plain call goes on without it
        assert not np.any(np.all(shown.reshape(2, -1) == 7, axis=1))
    finally:
        set_tips(A)
    clone([1, 3])()                                                            # the handle still works


# ==== the tip-shaped user mask ================================================================================================================
ROUND_AT = N.tip_rect(63, 0, 9, 9)                                              # (55, 0, 64, 9): touches the top and right edges
ASYM_AT = (0, 61, 3, 64)                                                        # touches the left and bottom edges


# ---- 8. off: today's behaviour ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_setting_off_a_round_tip_leaves_the_rectangles_footprint(arch):
    (_, A), _ = pools(arch)
    assert A.tip_footprint() is False
    open_both(arch, [2], 71)
    A.paint([2], ROUND_AT, COLOURS[0], 0.3, tips=6)
    assert np.array_equal(A.read(2)["UMASK"], N.umask_paint(np.zeros((64, 64)), ROUND_AT, TABLE))


# ---- 9. on, all-ones tips: nothing changes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_setting_on_ones_tips_change_nothing(arch):
    (_, A), (_, B) = pools(arch)
    ids = [0, 4, 8]
    open_both(arch, ids, 72)
    with footprint(A):
        sa = A.brush(ids, BOXES, COLOURS, None, 0.1, -1.0, tips=[0, 1, 2])
        sb = B.brush(ids, BOXES, COLOURS, None, 0.1, -1.0, tips=[0, 1, 2])
        assert np.array_equal(sa, sb)
        assert_same(A, B, ids, arch)
        for i, b in zip(ids, BOXES):
            assert np.array_equal(A.read(i)["UMASK"], N.umask_paint(np.zeros((64, 64)), b, TABLE))


# ---- 10. on: the specification ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_setting_on_umask_and_blend_are_the_specifications(arch):
    (_, A), (mb, _) = pools(arch)
    ids, boxes, tips = [2, 6], [ROUND_AT, ASYM_AT], [6, 4]
    open_both(arch, ids, 73)
    A.paint(ids, (20, 24, 36, 40), COLOURS[:2], weight=0.5)                    # an earlier, plain stroke: U_before is not zero
    st = [A.read(i) for i in ids]
    assert all(np.array_equal(s["UMASK"], N.umask_paint(np.zeros((64, 64)), (20, 24, 36, 40), TABLE)) for s in st)
    with footprint(A):
        shown = A.paint(ids, boxes, COLOURS[:2], 0.5, tips=tips)
    got = [A.read(i) for i in ids]
    xs = mb.sample_at(np.stack([g["Z"] for g in got]))                          # the model's own forward at the new latents, same batch
    for k, i in enumerate(ids):
        wn = A.tip(tips[k])
        U = N.umask_paint_tip(st[k]["UMASK"], wn, boxes[k][0], boxes[k][1], TABLE)
        rect = N.umask_paint(st[k]["UMASK"], boxes[k], TABLE)
        assert np.all(U <= rect) and np.any(U < rect), (arch, i)               # the corners the brush never touched stay out
        assert got[k]["UMASK"].dtype == np.float64 and np.array_equal(got[k]["UMASK"], U), (arch, i)
        im, _, field = N.photo_blend_local(xs[k], st[k]["RECON"], st[k]["ERROR"], U, GAUSS, False, THRESH)
        assert np.array_equal(shown[k], im) and np.array_equal(got[k]["IM"], im), (arch, i)
        assert np.array_equal(got[k]["FIELD"], field) and got[k]["FIELD_KIND"] == 0, (arch, i)


# ---- 11. on: a path is the loop of tip events ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
@pytest.mark.parametrize("mark", [False, True])
def test_setting_on_a_path_is_the_loop_of_events(arch, mark):
    """Five points, one repeated, one touching two edges, beside an untipped stroke of two points in the same call: the tipped stroke is
    the footprint kernel's, the plain one the stroke kernel's."""
    (_, A), (_, B) = pools(arch)
    ids, tips = [1, 5], [6, -1]
    pts = [(10, 12), (14, 13), (10, 12), (63, 63), (40, 30)]
    paths = [np.array([N.tip_rect(x, y, 9, 9) for x, y in pts]), np.array([(3, 50, 7, 54), (5, 52, 9, 56)])]
    open_both(arch, ids, 74)
    with footprint(A, B):
        got = A.stroke(ids, paths, COLOURS[:2], None, 0.2, -1.0, mark=mark, tips=tips)
        if mark:
            B.mark(ids)
        for k in range(5):
            act = [j for j in range(2) if k < len(paths[j])]
            last = B.brush([ids[j] for j in act], [paths[j][k] for j in act], COLOURS[act], None, 0.2, -1.0, tips=[tips[j] for j in act])
            if k == 1:
                second = last
    assert np.array_equal(got[0], last[0]) and np.array_equal(got[1], second[1]), (arch, mark)
    assert_same(A, B, ids, (arch, mark), history=True)
    U = np.zeros((64, 64))
    for c1, r1, _, _ in paths[0]:
        U = N.umask_paint_tip(U, A.tip(6), c1, r1, TABLE)
    assert np.array_equal(A.read(1)["UMASK"], U)
    assert np.array_equal(A.read(5)["UMASK"], N.stroke_footprint(np.zeros((64, 64)), paths[1], TABLE))
    assert A.history(1) == {"depth": 4, "undo": 1 if mark else 0, "redo": 0}


# ---- 12. on: the clone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_setting_on_a_tipped_clone_leaves_the_tips_shape(arch):
    (_, A), (_, B) = pools(arch)
    moved_sources(arch, [7], 75)
    open_both(arch, [2, 3], 76)
    with footprint(A):
        sa = A.clone([2, 3], [ROUND_AT, (5, 6, 20, 30)], [7, 7], [(-9, 11), (3, 11)], "IM", 3, 0.2, tips=[6, -1])
    sb = B.clone([2, 3], [ROUND_AT, (5, 6, 20, 30)], [7, 7], [(-9, 11), (3, 11)], "IM", 3, 0.2, tips=[6, -1])
    assert np.array_equal(A.read(2)["UMASK"], N.umask_paint_tip(np.zeros((64, 64)), A.tip(6), ROUND_AT[0], ROUND_AT[1], TABLE))
    assert np.array_equal(A.read(2)["Z"], B.read(2)["Z"])                      # the setting moves the mask, not the latent
    assert np.array_equal(B.read(2)["UMASK"], N.umask_paint(np.zeros((64, 64)), ROUND_AT, TABLE))
    assert np.array_equal(sa[1], sb[1])                                        # the item without a tip keeps its rectangle
    assert_same(A, B, [3], arch)


# ---- 13. on: who adds no footprint ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_setting_on_light_events_samples_and_unflagged_sessions_add_none(arch):
    (_, A), (_, B) = pools(arch)
    ids = [0, 4, 8]
    open_both(arch, ids, 77, flags=[1, 1, 2])
    z = O.make_latents(1, seed=78)
    for _, p in pools(arch):
        p.paint(ids, (20, 24, 36, 40), COLOURS, weight=0.5)
        p.sample([4], z)
    before = [A.read(i)["UMASK"] for i in ids]
    assert before[0].any() and not before[2].any()
    with footprint(A):
        sa = A.brush(ids, [ROUND_AT] * 3, COLOURS, [0, 1, 1], 0.2, [1.0, -1.0, -1.0], tips=6)   # a light event; sample mode; bit 0 clear
    sb = B.brush(ids, [ROUND_AT] * 3, COLOURS, [0, 1, 1], 0.2, [1.0, -1.0, -1.0], tips=6)
    assert np.array_equal(sa, sb)
    assert_same(A, B, ids, arch)
    for i, u in zip(ids, before):
        assert np.array_equal(A.read(i)["UMASK"], u), (arch, i)


# ---- 14. on: save and load --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_a_session_painted_under_the_setting_round_trips(arch):
    (_, A), _ = pools(arch)
    open_both(arch, [2, 6], 79)
    with footprint(A):
        A.mark([2])
        A.paint([2], ROUND_AT, COLOURS[0], 0.4, tips=6)
        rec = A.save([2])
        A.load([6], rec)
        assert_same(A, A, [2], (arch, "loaded"), history=True, ids_b=[6])
        assert np.array_equal(A.read(6)["UMASK"], N.umask_paint_tip(np.zeros((64, 64)), A.tip(6), ROUND_AT[0], ROUND_AT[1], TABLE))
        for i in (2, 6):                                                       # and it goes on as the saved one
            A.paint([i], ASYM_AT, COLOURS[1], 0.4, tips=4)
        assert_same(A, A, [2], (arch, "went on"), history=True, ids_b=[6])
    assert A.tip_footprint() is False


# ---- 15. on a whole photo ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_brush_compose_with_tips_is_brush_with_tips_then_compose(arch):
    (_, A), (_, B) = pools(arch)
    ids, boxes, tips = [3, 4], [N.tip_rect(20, 40, 9, 9), N.tip_rect(63, 0, 5, 3)], [6, 3]
    rs = np.random.RandomState(80)
    canvas = np.uint8(rs.randint(0, 256, (3, 128, 192)))
    win = ([0, 0], [(0, 0), (64, 16)], (128, 112))
    try:
        for _, p in pools(arch):
            p.reserve_canvases(1, 192, 128)
            p.canvas_put(0, canvas)
            p.place(ids, 0, [(0, 0), (64, 0)], [1, 2])                         # two placements, side 64 and side 128
            p.set_local(ids, flags=1)
        with footprint(A, B):
            shown, out = A.brush_compose(ids, boxes, COLOURS[:2], None, 0.5, -1.0, windows=win, tips=tips)
            want = B.brush(ids, boxes, COLOURS[:2], None, 0.5, -1.0, tips=tips)
            assert np.array_equal(shown, want) and out.shape == (2, 3, 112, 128)
            assert np.array_equal(out, B.compose(*win))
            assert not np.array_equal(out[0], canvas[:, :112, :128])            # the edit shows in the window
        for i in ids:
            want, got = B.read(i), A.read(i)
            for k in want:
                assert np.array_equal(got[k], want[k]), (arch, i, k)
        assert np.array_equal(A.read(3)["UMASK"], N.umask_paint_tip(np.zeros((64, 64)), A.tip(6), boxes[0][0], boxes[0][1], TABLE))
    finally:
        for _, p in pools(arch):
            p.reserve_canvases(0)


# ---- 16. windows --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_setting_on_paint_with_a_view_is_paint_then_render(arch):
    (_, A), (_, B) = pools(arch)
    ids, boxes = [0, 6], [N.tip_rect(20, 40, 9, 9), N.tip_rect(63, 0, 5, 3)]
    open_both(arch, ids, 81)
    view = ([(32, 40), (64, 0)], (64, 48))
    with footprint(A, B):
        shown, out = A.paint(ids, boxes, COLOURS[:2], 0.3, view=view, tips=[6, 3])
        want = B.paint(ids, boxes, COLOURS[:2], 0.3, tips=[6, 3])
        assert np.array_equal(shown, want) and out.shape == (2, 3, 48, 64)
        assert np.array_equal(out, B.render(ids, *view))
    assert_same(A, B, ids, arch)
    assert np.array_equal(A.read(0)["UMASK"], N.umask_paint_tip(np.zeros((64, 64)), A.tip(6), boxes[0][0], boxes[0][1], TABLE))

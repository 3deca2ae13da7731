"""The clone brush (ian_session_clone; EditSessions.clone / restore): a paint event whose target is a rectangle of another picture of the
pool.  The yardstick is always existing code: the stateless IAN.brush_step_batch(boxes, z, RGB=T, photo=(RECON, ERROR)) with T from
npe_ops.clone_target on the host-held copies of the pictures, at the same batch size and item order, driven as model_brush in
test_gpu_sessions.py drives it; for steps > 1 the loop of steps = 1 calls on a second range of ids of the same pool.  Every comparison
is np.array_equal, on `shown` and on every field read() returns."""
import ctypes as C
import os

import numpy as np
import pytest

from neural_photo_editor_amd import lib as L
from neural_photo_editor_amd import npe_ops as N
from oracle import ian_oracle as O
import session_helpers as H
from session_helpers import assert_fields, const_rgb, model_pool, refused

pytestmark = pytest.mark.gpu

CAP = 18                # ids 16 and 17 are never opened
GIM, IM, RECON = (L.SESSION_FIELDS[k][0] for k in ("GIM", "IM", "RECON"))

_cache = {}


def pool_of(arch="IAN_simple"):
    """(model, pool): one per architecture; a test that needs a reservation makes it and frees it again."""
    if arch not in _cache:
        _cache[arch] = model_pool(arch, capacity=CAP)
    return _cache[arch]


def host_open(m, ph):
    """NPE.infer (NPE.py:257-264) through the stateless calls at batch n -> list of session dicts."""
    Z = m.encode_images(np.float32(N.to_tanh(ph)))
    R = m.sample_at_uint8(Z)
    return [dict(Z=Z[i].copy(), RECON=R[i], ERROR=N.to_tanh(np.float32(ph[i])) - N.to_tanh(np.float32(R[i])), IM=ph[i].copy(),
                 GIM=ph[i].copy(), MODE=0) for i in range(len(ph))]


def open_both(m, pool, ids, seed):
    """The sessions on the device and their host-held twins M[id]."""
    ph = H.sources(len(ids), 1, seed)
    pool.open(ids, ph)
    return dict(zip(ids, host_open(m, ph)))


def model_step(m, M, ids, boxes, rgb, weight, sign=-1.0):
    """One stateless paint call on the host-held state of sessions `ids`, in that order, towards the images rgb -> shown; M is updated
    as NPE.py updates its globals."""
    n = len(ids)
    z = np.stack([M[i]["Z"] for i in ids])
    recon = np.stack([M[i]["RECON"] for i in ids])
    error = np.stack([M[i]["ERROR"] for i in ids])
    z_new, x, im, _ = m.brush_step_batch(np.asarray(boxes), z, rgb, weight=weight, sign=sign, modes=[1] * n, photo=(recon, error))
    shown = np.empty((n, 3, 64, 64), np.uint8)
    for k, i in enumerate(ids):
        M[i]["Z"] = z_new[k].copy()
        M[i]["X"] = x[k].copy()                            # sample_at(z_new) as this call computed it (no field of a session)
        if M[i]["MODE"] == 0:                              # NPE.paint in photo mode: the blend becomes IM
            M[i]["IM"] = im[k].copy()
            shown[k] = im[k]
        else:                                              # sample mode: update_photo(None)
            shown[k] = np.uint8(N.from_tanh(x[k]))
    return shown


def model_clone(m, M, ids, boxes, sources, offsets, fields, weight, steps=1):
    """`steps` stateless calls with the target images a caller would build on the host.  The targets are built anew for every step from
    the host-held pictures, as the library reads them anew: the call refuses the one case in which they would change."""
    shown = None
    for _ in range(steps):
        T = np.stack([N.clone_target(M[s][f], b, o) for s, f, b, o in zip(sources, fields, boxes, offsets)])
        shown = model_step(m, M, ids, boxes, T, weight)
    return shown


def assert_pool_equals_model(pool, M, ids, tag):
    for i in ids:
        assert_fields(pool.read(i), M[i], tag=(tag, i))


# ---- 1. steps = 1 against the stateless call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_one_step_equals_the_stateless_call_on_the_target_image(arch):
    """Three destinations in one call: another session's GIM at (+5, -3); the own GIM at offset 0 in a corner; another session's RECON
    with the source rectangle in the opposite corner."""
    m, pool = pool_of(arch)
    ids = [3, 9, 1, 12]
    M = open_both(m, pool, ids, 51)
    dst, boxes = [3, 9, 1], [(10, 20, 14, 24), (60, 0, 64, 4), (0, 0, 6, 3)]
    src, offs, fields = [12, 9, 3], [(5, -3), (0, 0), (58, 61)], ["GIM", "GIM", "RECON"]
    want = model_clone(m, M, dst, boxes, src, offs, fields, 0.3)
    got = pool.clone(dst, boxes, src, offs, fields, steps=1, weight=0.3)
    assert got.dtype == np.uint8 and np.array_equal(got, want), arch
    assert_pool_equals_model(pool, M, ids, arch)
    for k, i in enumerate(dst):
        assert np.array_equal(got[k], pool.read(i)["IM"]), (arch, i)                               # a photo-mode destination stores its blend


# ---- 2. the whole picture -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_the_whole_picture_from_another_session(arch):
    m, pool = pool_of(arch)
    ids = [2, 7]
    M = open_both(m, pool, ids, 52)
    want = model_clone(m, M, [2], [(0, 0, 64, 64)], [7], [(0, 0)], ["GIM"], 0.3)
    got = pool.clone([2], (0, 0, 64, 64), 7, weight=0.3)
    assert np.array_equal(got, want), arch
    assert_pool_equals_model(pool, M, ids, arch)


# ---- 3. IM as the source --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_im_of_a_painted_session_as_the_source(arch):
    m, pool = pool_of(arch)
    ids = [4, 11]
    M = open_both(m, pool, ids, 53)
    box, off = (20, 18, 30, 28), (4, 6)
    want = model_step(m, M, [11], [(16, 16, 44, 44)], const_rgb((250, 20, 20))[None], 0.5)      # paint the source
    assert np.array_equal(pool.paint([11], (16, 16, 44, 44), (250, 20, 20), weight=0.5), want)
    s = pool.read(11)
    assert_fields(s, M[11], tag=(arch, "painted"))
    assert not np.array_equal(s["IM"][:, 24:34, 24:34], s["GIM"][:, 24:34, 24:34])                # inside the source rectangle
    other = {i: {k: np.copy(v) for k, v in M[i].items()} for i in ids}
    want = model_clone(m, M, [4], [box], [11], [off], ["IM"], 0.3)
    model_clone(m, other, [4], [box], [11], [off], ["GIM"], 0.3)
    got = pool.clone([4], box, 11, off, "IM", weight=0.3)
    assert np.array_equal(got, want), arch
    assert_pool_equals_model(pool, M, ids, arch)
    assert not np.array_equal(M[4]["Z"], other[4]["Z"])                                           # and not the one on GIM


# ---- 4. steps = 3 against three calls of steps = 1 --------------------------------------------------------------------------------------
def assert_sessions_equal(pool, ids_o, ids_s, tag):
    for a, b in zip(ids_o, ids_s):
        want, got = pool.read(a), pool.read(b)
        assert set(want) == set(got), (tag, a, b)
        for k in want:
            assert np.array_equal(got[k], want[k]), (tag, k, a, b)


@pytest.mark.parametrize("arch", O.ARCHS)
def test_three_steps_equal_three_calls_with_every_reservation(arch):
    """Two id ranges opened from the same full-resolution photos in a pool with the hires (scale 2), local and history reservations; LOCAL
    bit 0 on one session of each range, the other with flags 0; one destination reads the GIM of a third session, one its own RECON at
    an offset.  Then the same from an undone state."""
    _, pool = pool_of(arch)
    pool.reserve_hires(2)
    pool.reserve_local()
    pool.reserve_history(4)
    try:
        ids_o, ids_s = [0, 1, 2], [8, 9, 10]
        ph = H.sources(3, 2, 54)
        for ids in (ids_o, ids_s):
            pool.open_hires(ids, ph)
            pool.set_local(ids[:2], flags=[1, 0])
            pool.mark(ids[:2])
        boxes, offs, fields = [(10, 20, 22, 30), (30, 5, 38, 17)], [(7, -4), (-20, 30)], ["GIM", "RECON"]
        src = lambda ids: [ids[2], ids[1]]
        want = [pool.clone(ids_o[:2], boxes, src(ids_o), offs, fields, steps=1, weight=0.3) for _ in range(3)]
        got = pool.clone(ids_s[:2], boxes, src(ids_s), offs, fields, steps=3, weight=0.3)
        assert np.array_equal(got, want[2]) and not np.array_equal(want[2], want[0]), arch
        assert_sessions_equal(pool, ids_o, ids_s, arch)                                         # UMASK, LOCAL, FIELD, FIELD_KIND, SOURCE among them
        st = pool.read(ids_s[0])
        assert np.array_equal(st["UMASK"], N.umask_paint(np.zeros((64, 64)), boxes[0], N.local_falloff_table())) and st["FIELD_KIND"] == 0
        assert not pool.read(ids_s[1])["UMASK"].any() and st["FIELD"].any()
        assert np.array_equal(pool.render(ids_s[:2], (32, 40), (64, 48)), pool.render(ids_o[:2], (32, 40), (64, 48)))
        hist = lambda ids: [pool.history(i) for i in ids[:2]]
        assert hist(ids_s) == hist(ids_o) == [{"depth": 4, "undo": 1, "redo": 0}] * 2
        assert np.array_equal(pool.undo(ids_s[:2]), pool.undo(ids_o[:2]))
        assert hist(ids_s) == hist(ids_o) == [{"depth": 4, "undo": 0, "redo": 1}] * 2
        # from the undone state: `edited` once on one side, three times on the other
        want = [pool.clone(ids_o[:2], boxes, src(ids_o), offs, fields, steps=1, weight=0.2) for _ in range(3)]
        got = pool.clone(ids_s[:2], boxes, src(ids_s), offs, fields, steps=3, weight=0.2)
        assert np.array_equal(got, want[2]) and hist(ids_s) == hist(ids_o)
        assert_sessions_equal(pool, ids_o, ids_s, (arch, "edited"))
    finally:
        pool.reserve_history(0)
        pool.reserve_local(False)
        pool.reserve_hires(0)


# ---- 5. several passes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_brush_pass_2_runs_three_items_as_batches_of_two_and_one(arch):
    """brush_pass = 2, n = 3, steps = 2: bitwise the stateless calls under the same option (batch 2, then batch 1), each pass through both
    its steps; the third item reads the first one's GIM."""
    m, pool = pool_of(arch)
    ids = [0, 5, 13]
    M = open_both(m, pool, ids, 55)
    boxes, src, offs, fields = [(4, 4, 12, 9), (40, 30, 47, 41), (20, 50, 31, 60)], [5, 5, 0], [(20, 20), (-3, 2), (1, -40)], ["GIM", "RECON", "GIM"]
    m.handle.set_option("brush_pass", 2)
    try:
        want = model_clone(m, M, ids, boxes, src, offs, fields, 0.3, steps=2)
        got = pool.clone(ids, boxes, src, offs, fields, steps=2, weight=0.3)
        assert np.array_equal(got, want), arch
        assert_pool_equals_model(pool, M, ids, arch)
    finally:
        m.handle.set_option("brush_pass", 256)


# ---- 6. an empty rectangle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_an_empty_rectangle_leaves_the_latent_and_shows_the_blend_at_it(arch):
    m, pool = pool_of(arch)
    ids = [6, 14]
    M = open_both(m, pool, ids, 56)
    z0 = M[14]["Z"].copy()
    boxes, offs = [(10, 10, 20, 20), (20, 20, 20, 30)], [(3, 3), (500, -500)]           # an empty one may be shifted anywhere
    want = model_clone(m, M, ids, boxes, [14, 6], [offs[0], (0, 0)], ["GIM", "GIM"], 0.3, steps=2)
    got = pool.clone(ids, boxes, [14, 6], offs, steps=2, weight=0.3)
    assert np.array_equal(got, want), arch
    assert_pool_equals_model(pool, M, ids, arch)
    st = pool.read(14)
    assert np.array_equal(st["Z"], z0)
    assert np.array_equal(got[1], N.photo_blend_host(M[14]["X"], st["RECON"], st["ERROR"])[0])


# ---- 7. a sample-mode destination -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_a_sample_mode_destination_shows_the_plain_sample_and_keeps_im(arch):
    m, pool = pool_of(arch)
    ids = [3, 8]
    M = open_both(m, pool, ids, 57)
    z = O.make_latents(1, seed=9)
    rec = pool.sample([3], z)
    M[3].update(Z=z[0].copy(), RECON=rec[0], ERROR=N.to_tanh(np.float32(M[3]["IM"])) - N.to_tanh(np.float32(rec[0])), MODE=1)
    assert_fields(pool.read(3), M[3], tag=(arch, "sampled"))
    im0 = M[3]["IM"].copy()
    want = model_clone(m, M, [3], [(12, 12, 40, 36)], [8], [(-6, 9)], ["GIM"], 0.3)
    got = pool.clone([3], (12, 12, 40, 36), 8, (-6, 9), weight=0.3)
    st = pool.read(3)
    assert np.array_equal(got, want) and np.array_equal(got[0], np.uint8(N.from_tanh(M[3]["X"]))), arch
    assert_pool_equals_model(pool, M, ids, arch)
    assert st["MODE"] == 1 and np.array_equal(st["IM"], im0) and not np.array_equal(st["Z"], z[0])


# ---- 8. residency --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_clone_brush_clone_on_the_same_ids_pass_the_residency_on(arch):
    """Nothing but the three calls on the pool's side: the second and third skip their gather and forward."""
    m, pool = pool_of(arch)
    ids = [2, 10, 15]
    M = open_both(m, pool, ids, 58)
    dst, boxes = [2, 10], [(8, 30, 20, 41), (33, 12, 45, 20)]
    cols = np.array([(250, 20, 20), (10, 240, 90)])
    want = [model_clone(m, M, dst, boxes, [15, 2], [(9, -9), (0, 5)], ["GIM", "RECON"], 0.3, steps=2),
            model_step(m, M, dst, boxes, np.stack([const_rgb(c) for c in cols]), 0.3),
            model_clone(m, M, dst, boxes, [15, 10], [(-4, 2), (6, 6)], ["RECON", "GIM"], 0.3)]
    got = [pool.clone(dst, boxes, [15, 2], [(9, -9), (0, 5)], ["GIM", "RECON"], steps=2, weight=0.3),
           pool.brush(dst, np.array(boxes), cols, weight=0.3),
           pool.clone(dst, boxes, [15, 10], [(-4, 2), (6, 6)], ["RECON", "GIM"], weight=0.3)]
    for k in range(3):
        assert np.array_equal(got[k], want[k]), (arch, k)
    assert_pool_equals_model(pool, M, ids, arch)


# ---- 9. refusals through the library --------------------------------------------------------------------------------------------------------
def raw_events(rows):
    """ctypes events straight for the library: rows = (session, box, source, field, dc, dr)."""
    ev = (L.SessionCloneEvent * len(rows))()
    for e, (sid, box, src, field, dc, dr) in zip(ev, rows):
        e.session, e.source, e.field, e.dc, e.dr, e.coef, e.gscale = sid, src, field, dc, dr, -0.3, 5.0
        e.c1, e.r1, e.c2, e.r2 = box
    return ev


def test_refusals_name_the_item_and_change_nothing():
    import torch
    m, pool = pool_of()
    h = m.handle
    ids = [4, 5, 6]
    pool.open(ids, H.sources(3, 1, 59))
    pool.paint(ids, (10, 10, 30, 30), (200, 100, 50), weight=0.5)
    before = [pool.read(i) for i in ids]
    shown = np.full((2, 3, 64, 64), 7, np.uint8)
    B = (8, 8, 12, 12)
    ok = (4, B, 6, GIM, 0, 0)

    def call(rows, steps=1):
        ev = raw_events(rows)
        return lambda: h.session_clone(ev, steps, shown)

    def device_events():
        dev = torch.zeros(C.sizeof(L.SessionCloneEvent), dtype=torch.uint8, device="cuda")
        h._check(h.lib.ian_session_clone(h._h, 1, C.cast(dev.data_ptr(), C.POINTER(L.SessionCloneEvent)), 1, L._ptr(shown), C.c_void_p(0)))

    bad = [
        (r"item 1: source session 18 outside the pool \(capacity 18\)", call([ok, (5, B, CAP, GIM, 0, 0)])),
        ("item 1: source session -1 outside the pool", call([ok, (5, B, -1, GIM, 0, 0)])),
        ("item 1: source session 16 has not been opened", call([ok, (5, B, 16, GIM, 0, 0)])),
        ("item 1: field 2 ", call([ok, (5, B, 6, L.SESSION_FIELDS["ERROR"][0], 0, 0)])),
        ("item 0: field 0 ", call([(4, B, 6, L.SESSION_FIELDS["Z"][0], 0, 0)])),
        (r"item 1: patch \(8,8,12,12\) shifted by \(-9,0\) leaves", call([ok, (5, B, 6, GIM, -9, 0)])),
        (r"item 1: patch \(8,8,12,12\) shifted by \(53,0\) leaves", call([ok, (5, B, 6, GIM, 53, 0)])),
        (r"item 0: patch \(8,8,12,12\) shifted by \(0,-9\) leaves", call([(4, B, 6, RECON, 0, -9)])),
        (r"item 0: patch \(8,8,12,12\) shifted by \(0,53\) leaves", call([(4, B, 6, RECON, 0, 53)])),
        (r"item 0: patch \(8,8,12,12\) shifted by \(2147483647,0\) leaves", call([(4, B, 6, GIM, 2 ** 31 - 1, 0)])),
        ("item 1: source session 4 is read from IM, which item 0 of this call writes", call([ok, (5, B, 4, IM, 0, 0)])),
        ("item 0: source session 4 is read from IM, which item 0", call([(4, B, 4, IM, 0, 0)])),
        (r"steps = 0 outside 1\.\.64", call([ok], 0)),
        (r"steps = 65 outside 1\.\.64", call([ok], 65)),
        ("must be a host array", device_events),
        ("item 1: session 4 already appears as item 0", call([ok, ok])),                     # what the brush checks for the destination
        ("item 1: session 16 has not been opened", call([ok, (16, B, 6, GIM, 0, 0)])),
        ("item 0: session 18 outside the pool", call([(CAP, B, 6, GIM, 0, 0)])),
        (r"item 1: patch \(8,8,65,12\) outside the 64x64 image", call([ok, (5, (8, 8, 65, 12), 6, GIM, 0, 0)])),
        ("n = 0", call([])),
    ]
    for needle, c in bad:
        refused(c, needle, -7)
        assert np.all(shown == 7), needle
        for i, b in zip(ids, before):
            got = pool.read(i)
            assert set(got) == set(b)
            for k in b:
                assert np.array_equal(got[k], b[k]), (needle, i, k)
    # and the handle still works: an IM source that is no destination, the same source for both items
    call([(4, B, 6, IM, 3, 3), (5, B, 6, IM, -3, -3)])()
    assert not np.any(np.all(shown.reshape(2, -1) == 7, axis=1))


def test_minus_6_until_the_blend_is_set():
    """On a raw handle of its own: a pool and an opened session, but no ian_sessions_set_blend."""
    from neural_photo_editor_amd import IAN
    m = IAN(os.path.join(H.ROOT, "neural_photo_editor_amd", "configs", "IAN_simple.py"), True, params=O.make_params("IAN_simple", 1))
    h = m.handle
    ev = raw_events([(0, (8, 8, 12, 12), 0, GIM, 2, 2)])
    refused(lambda: h.session_clone(ev, 1, None), "no session pool", -6)
    h.sessions_reserve(2)
    h.session_open(np.asarray([0], np.int32), H.sources(1, 1, 60))
    refused(lambda: h.session_clone(ev, 1, None), "Gaussian is not set", -6)
    h.sessions_set_blend(N.gaussian_half_kernel(0.7, 3))
    shown = np.full((1, 3, 64, 64), 7, np.uint8)
    h.session_clone(ev, 2, shown)
    assert not np.all(shown == 7)


# ---- 10. restore -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", O.ARCHS)
def test_restore_is_clone_from_the_own_photo_at_offset_0(arch):
    m, pool = pool_of(arch)
    a, b = [1, 2], [9, 10]
    ph = H.sources(2, 1, 61)
    boxes = np.array([(10, 10, 30, 30), (25, 30, 50, 44)])
    for ids in (a, b):
        pool.open(ids, ph)
        pool.paint(ids, (8, 8, 52, 52), (250, 250, 10), weight=0.5)
    M = dict(zip(a, host_open(m, ph)))
    model_step(m, M, a, [(8, 8, 52, 52)] * 2, np.stack([const_rgb((250, 250, 10))] * 2), 0.5)
    want = model_clone(m, M, a, boxes, a, [(0, 0)] * 2, ["GIM"] * 2, 0.2, steps=2)
    got_a = pool.clone(a, boxes, a, (0, 0), "GIM", steps=2, weight=0.2)
    got_b = pool.restore(b, boxes, steps=2, weight=0.2)
    assert np.array_equal(got_a, want) and np.array_equal(got_b, want), arch
    assert_pool_equals_model(pool, M, a, arch)
    assert_sessions_equal(pool, a, b, arch)

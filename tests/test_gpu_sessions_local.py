"""Local edits in edit sessions (ian_sessions_reserve_local, ian_sessions_set_local, ian_session_local; EditSessions.reserve_local /
set_local).  Every comparison is np.array_equal: the numpy functions of npe_ops (local_falloff_table, local_footprint, umask_paint,
photo_blend_local) specify the arithmetic and the device matches them bit for bit.  The host model of a brush call is the stateless
brush_step_batch on a SECOND model (for x and the new latents) followed by those numpy functions; sessions with flags 0 are held
against a second pool WITHOUT the reservation, which shows that nothing that exists has changed."""
import numpy as np
import pytest

from oracle import ian_oracle as O
import session_helpers as H
from session_helpers import KEYS64, assert_fields, const_rgb, model_pool, refused, session_events as events

pytestmark = pytest.mark.gpu

CAP = 16
IDS = [9, 2, 14]
THRESH = 0.75

_cache = {}


def pools(arch="IAN_simple"):
    """Two models with the same synthetic parameters, one pool each: (model, pool with the local reservation, model, plain pool).  The
    stateless calls of a test go to the SECOND model, so that the first handle sees session calls only."""
    if arch not in _cache:
        _cache[arch] = model_pool(arch) + model_pool(arch)
        _cache[arch][1].reserve_local()
    return _cache[arch]


def sources(n, seed):
    """Smooth pictures plus noise, every byte value present: the bright pixels (level 224 and above) are what make dampen fire."""
    return H.sources(n, 1, seed)


def dampened_count(x, recon, error, mask_l):
    """How many values dampen replaces, from the spec's own terms."""
    from neural_photo_editor_amd import npe_ops as N
    t32 = N.to_tanh(np.float32(recon))
    D = mask_l * (np.asarray(x, np.float32) - t32) + (1 - mask_l) * error
    return int(((np.float64(t32) + D) > THRESH).sum())


def model_brush(mp, M, ids, boxes, colours, modes, weight, sign, stats):
    """The stateless call on the host-held state of sessions `ids` for x and the new latents, then umask_paint and photo_blend_local as
    the sessions' flags ask -> shown; M is updated as the pool updates its rows."""
    from neural_photo_editor_amd import npe_ops as N
    n = len(ids)
    table, half = N.local_falloff_table(), N.gaussian_half_kernel()
    z = np.stack([M[i]["Z"] for i in ids])
    rgb = np.stack([const_rgb(colours[k]) if modes[k] else np.zeros((3, 64, 64), np.float32) for k in range(n)])
    z_new, x = mp.brush_step_batch(np.asarray(boxes), z, rgb, weight=weight, sign=sign, modes=modes)
    shown = np.empty((n, 3, 64, 64), np.uint8)
    for k, i in enumerate(ids):
        S = M[i]
        S["Z"] = z_new[k].copy()
        S["X"] = x[k].copy()
        if S["MODE"] == 0 and modes[k] == 1:
            fl = S["LOCAL"]
            if fl & 1:
                S["UMASK"] = N.umask_paint(S["UMASK"], boxes[k], table)
            im, mask_l, _ = N.photo_blend_local(x[k], S["RECON"], S["ERROR"], S["UMASK"] if fl & 1 else None, half, bool(fl & 2), THRESH)
            S["IM"] = im
            shown[k] = im
            stats["differs"] += int((im != N.photo_blend_host(x[k], S["RECON"], S["ERROR"])[0]).any())
            if fl & 2:
                stats["dampened"].append(dampened_count(x[k], S["RECON"], S["ERROR"], mask_l))
        else:
            shown[k] = np.uint8(N.from_tanh(x[k]))
    return shown


# ---- 1. flags 0 ------------------------------------------------------------------------------------------------------------------
def test_sessions_with_flags_0_give_the_results_of_a_pool_without_the_reservation():
    _, sl, _, sp = pools()
    ph = sources(3, 1)
    z = O.make_latents(3, seed=3)
    boxes = np.array([(0, 0, 4, 4), (23, 30, 40, 47), (60, 60, 64, 64)])
    boxes2 = np.array([(30, 35, 47, 52), (5, 9, 6, 10), (10, 10, 10, 20)])
    colours = np.array([(250, 20, 20), (10, 240, 90), (30, 30, 200)])
    script = [
        ("open", lambda s: s.open(IDS, ph)),
        ("paint", lambda s: s.paint(IDS, boxes, colours, weight=0.5)),
        ("paint", lambda s: s.paint(IDS, boxes2, colours, weight=0.5)),
        ("scroll", lambda s: s.scroll(IDS, boxes, [1.0, -1.0, 1.0], weight=0.3)),
        ("set_latent", lambda s: s.set_latent(IDS, z)),
        ("sample", lambda s: s.sample([14], z[:1])),
        ("paint", lambda s: s.paint(IDS, boxes, colours, weight=0.5)),
        ("reset", lambda s: s.reset(IDS)),
        ("commit", lambda s: s.commit(IDS)),
    ]
    for step, (name, call) in enumerate(script):
        got, want = call(sl), call(sp)
        if name == "open":
            sl.set_local(IDS, flags=0)
        assert np.array_equal(got, want), (step, name)
        for i in IDS:
            a, b = sl.read(i), sp.read(i)
            assert_fields(a, b, KEYS64, (step, name, i))
            assert a["LOCAL"] == 0 and not a["UMASK"].any() and "UMASK" not in b


# ---- 2. the brush script -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("arch", O.ARCHS)
def test_brush_script_equals_the_host_model(arch, flags):
    _, sl, mp, _ = pools(arch)
    ph = sources(3, 20 + flags)
    sl.open(IDS, ph)
    sl.set_local(IDS, flags=flags)
    sl.sample([14], O.make_latents(1, seed=7))                           # session 14 goes to sample mode
    M = {i: dict(sl.read(i)) for i in IDS}
    for i in IDS:
        assert M[i]["LOCAL"] == flags and not M[i]["UMASK"].any() and M[i]["MODE"] == (1 if i == 14 else 0)
    colours = np.array([(250, 20, 20), (10, 240, 90), (30, 30, 200)])
    empty = (10, 10, 10, 20)
    calls = [   # boxes per session, modes, weight, sign
        ([(23, 30, 40, 47), (0, 0, 4, 4), (60, 60, 64, 64)], [1, 1, 1], 0.5, -1.0),
        ([(0, 0, 4, 4), (23, 30, 40, 47), (5, 9, 6, 10)], [1, 1, 1], 0.5, -1.0),       # a second stroke on sessions 9 and 2
        ([(60, 60, 64, 64), (5, 9, 6, 10), empty], [0, 1, 1], [0.3, 0.5, 0.5], [1.0, -1.0, -1.0]),
        ([(5, 9, 6, 10), empty, (0, 0, 4, 4)], [1, 1, 0], [0.5, 0.5, 0.3], [-1.0, -1.0, -1.0]),
    ]
    stats = {"differs": 0, "dampened": []}
    umask_after = []
    for step, (boxes, modes, weight, sign) in enumerate(calls):
        want = model_brush(mp, M, IDS, boxes, colours, modes, weight, sign, stats)
        shown = sl.brush(IDS, boxes, colours, modes, weight, sign)
        assert np.array_equal(shown, want), (arch, flags, step)
        for i in IDS:
            got = sl.read(i)
            assert_fields(got, M[i], ("IM", "UMASK", "Z", "MODE", "LOCAL", "RECON", "ERROR", "GIM"), (arch, flags, step, i))
        umask_after.append(M[9]["UMASK"].copy())
    # what keeps the comparisons above from passing vacuously, on the numpy side
    assert stats["differs"] > 0
    if flags & 2:
        assert stats["dampened"] and all(0 < c < 3 * 64 * 64 for c in stats["dampened"]), stats["dampened"]
    if flags & 1:
        assert umask_after[0].any() and not np.array_equal(umask_after[1], umask_after[0])
        assert np.array_equal(umask_after[2], umask_after[1])            # a lighten event adds no footprint
        assert not M[14]["UMASK"].any()                                  # nor does anything on a sample-mode session
    else:
        assert not any(u.any() for u in umask_after)                     # dampen alone leaves UMASK untouched


# ---- 3. set_latent ---------------------------------------------------------------------------------------------------------------
def test_set_latent_shows_the_edit_only_where_the_user_has_brushed():
    from neural_photo_editor_amd import npe_ops as N
    _, sl, mp, _ = pools()
    ids = [3, 11]
    sl.open(ids, sources(2, 31))
    sl.set_local(ids, flags=[1, 3])
    st = [sl.read(i) for i in ids]
    half, table = N.gaussian_half_kernel(), N.local_falloff_table()
    z = O.make_latents(2, seed=41)
    xs = mp.sample_at(z)
    shown = sl.set_latent(ids, z)
    for k, i in enumerate(ids):
        got = sl.read(i)
        want = N.photo_blend_local(xs[k], st[k]["RECON"], st[k]["ERROR"], np.zeros((64, 64)), half, k == 1, THRESH)[0]
        assert np.array_equal(shown[k], want), i
        assert np.array_equal(got["Z"], z[k]) and np.array_equal(got["IM"], st[k]["IM"]) and not got["UMASK"].any()
    with np.errstate(invalid="ignore"):                                  # UMASK == 0 without dampen: the byte image of RECON + ERROR
        assert np.array_equal(shown[0], np.uint8(N.from_tanh(N.to_tanh(st[0]["RECON"]) + np.float64(st[0]["ERROR"]))))
    # after a stroke: the blend with that UMASK, and no footprint added by set_latent
    box = (20, 24, 36, 40)
    sl.paint(ids, box, (250, 20, 20), weight=0.5)
    U = N.umask_paint(np.zeros((64, 64)), box, table)
    z2 = O.make_latents(2, seed=42)
    xs2 = mp.sample_at(z2)
    shown = sl.set_latent(ids, z2)
    from_zero = from_plain = 0
    for k, i in enumerate(ids):
        got = sl.read(i)
        assert np.array_equal(got["UMASK"], U), i
        want = N.photo_blend_local(xs2[k], st[k]["RECON"], st[k]["ERROR"], U, half, k == 1, THRESH)[0]
        assert np.array_equal(shown[k], want), i
        from_zero += int((want != N.photo_blend_local(xs2[k], st[k]["RECON"], st[k]["ERROR"], np.zeros((64, 64)), half, k == 1, THRESH)[0]).any())
        from_plain += int((want != N.photo_blend_host(xs2[k], st[k]["RECON"], st[k]["ERROR"])[0]).any())
    assert from_zero > 0 and from_plain > 0                              # the stroke shows, and the rest of the picture does not


# ---- 4. clearing -----------------------------------------------------------------------------------------------------------------
def test_open_reset_commit_and_set_local_clear_umask_and_keep_local():
    _, sl, _, _ = pools()
    ids = [1, 6]
    ph = sources(2, 51)

    def stroke():
        sl.paint(ids, (8, 8, 30, 30), (10, 200, 30), weight=0.5)
        for i in ids:
            assert sl.read(i)["UMASK"].any()

    def assert_cleared(tag):
        for i, f in zip(ids, (1, 3)):
            got = sl.read(i)
            assert not got["UMASK"].any() and got["LOCAL"] == f, (tag, i)

    sl.open(ids, ph)
    sl.set_local(ids, flags=[1, 3])
    for tag, call in (("open", lambda: sl.open(ids, ph)), ("reset", lambda: sl.reset(ids)), ("commit", lambda: sl.commit(ids)),
                      ("set_local", lambda: sl.set_local(ids, flags=[1, 3]))):
        stroke()
        call()
        assert_cleared(tag)
    # set_local clears whichever flags are given, and only the sessions it names
    stroke()
    keep = sl.read(6)["UMASK"]
    sl.set_local([1], flags=0)
    assert not sl.read(1)["UMASK"].any() and sl.read(1)["LOCAL"] == 0
    assert np.array_equal(sl.read(6)["UMASK"], keep) and sl.read(6)["LOCAL"] == 3
    # growing the pool keeps UMASK and LOCAL of the sessions that remain; new rows start at zero
    sl.set_local([1], flags=1)
    stroke()
    before = [sl.read(i) for i in ids]
    try:
        sl.reserve(CAP + 4)
        for i, b in zip(ids, before):
            got = sl.read(i)
            assert_fields(got, b, KEYS64 + ("UMASK", "LOCAL"), ("grown", i))
        sl.open([CAP + 3], ph[:1])
        got = sl.read(CAP + 3)
        assert got["LOCAL"] == 0 and not got["UMASK"].any()
        sl.set_local([CAP + 3], flags=3)
        sl.paint([CAP + 3, 6], (40, 40, 50, 50), (200, 10, 10), weight=0.5)
        assert sl.read(CAP + 3)["UMASK"].any() and sl.read(CAP + 3)["LOCAL"] == 3
    finally:
        sl.reserve(CAP)
    got = sl.read(1)
    assert_fields(got, before[0], KEYS64 + ("UMASK", "LOCAL"), "shrunk")


# ---- 5. full resolution ----------------------------------------------------------------------------------------------------------
def test_full_resolution_field_and_windows():
    from neural_photo_editor_amd import npe_ops as N
    s = 2
    _, sl, mp, _ = pools()
    sl.reserve_hires(s)
    try:
        ids = [4, 5]
        rs = np.random.RandomState(61)
        src = np.repeat(np.repeat(sources(2, 62), s, axis=2), s, axis=3)
        src = np.uint8(np.clip(src.astype(int) + rs.randint(-3, 4, src.shape), 0, 255))
        sl.open_hires(ids, src)
        sl.set_local(ids, flags=1)
        M = {i: dict(sl.read(i)) for i in ids}
        box, colours = (8, 8, 20, 20), np.array([(250, 20, 20), (10, 240, 90)])
        stats = {"differs": 0, "dampened": []}
        want = model_brush(mp, M, ids, [box, box], colours, [1, 1], 0.5, -1.0, stats)
        near, far = (8, 12, 64, 40), (96, 100, 32, 28)                   # (x, y, vw, vh): over the stroke, and the far corner
        shown, out_near = sl.paint(ids, box, colours, weight=0.5, view=((near[0], near[1]), (near[2], near[3])))
        assert np.array_equal(shown, want) and stats["differs"] >= 1
        out_far = sl.render(ids, (far[0], far[1]), (far[2], far[3]))
        table, half = N.local_falloff_table(), N.gaussian_half_kernel()
        for k, i in enumerate(ids):
            got = sl.read(i)
            field = N.photo_blend_local(M[i]["X"], M[i]["RECON"], M[i]["ERROR"], M[i]["UMASK"], half, False, THRESH)[2]
            assert field.any()
            assert got["FIELD_KIND"] == 0 and got["FIELD"].dtype == np.float32
            assert np.array_equal(got["FIELD"], field), i
            assert np.array_equal(got["UMASK"], N.umask_paint(np.zeros((64, 64)), box, table))
            assert np.array_equal(out_near[k], N.hires_render(src[k], field, 0, s, *near)), i
            assert (out_near[k] != src[k][:, near[1]:near[1] + near[3], near[0]:near[0] + near[2]]).any()
            # the far window: the reference's own field rounds to nothing there, so the source bytes come back
            cells = field[:, far[1] // s - 1:, far[0] // s - 1:]
            assert np.all(np.rint(np.float32(127.5) * np.abs(cells)) == 0)
            crop = src[k][:, far[1]:far[1] + far[3], far[0]:far[0] + far[2]]
            assert np.array_equal(N.hires_render(src[k], field, 0, s, *far), crop)
            assert np.array_equal(out_far[k], crop), i
        # open_hires clears the stroke's UMASK in its own submission and keeps LOCAL
        sl.open_hires(ids, src)
        for i in ids:
            got = sl.read(i)
            assert M[i]["UMASK"].any() and not got["UMASK"].any() and got["LOCAL"] == 1, i
    finally:
        sl.reserve_hires(0)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_change_nothing():
    from neural_photo_editor_amd import npe_ops as N
    from neural_photo_editor_amd.lib import IanError
    ml, sl, mp, sp = pools()
    hl, hp = ml.handle, mp.handle
    ids = [0, 1, 2]
    for pool in (sl, sp):
        pool.open(ids, sources(3, 71))
    sl.set_local(ids, flags=[1, 2, 3])
    sl.paint(ids, (10, 10, 30, 30), (200, 100, 50), weight=0.5)
    keys = KEYS64 + ("UMASK", "LOCAL")
    before = [sl.read(i) for i in ids]
    before_p = [sp.read(i) for i in ids]

    def unchanged(tag):
        for i, b in zip(ids, before):
            got = sl.read(i)
            assert_fields(got, b, keys, (tag, i))

    good = N.local_falloff_table()

    def table(**change):
        t = good.copy()
        for k, v in change.items():
            t[int(k[1:])] = v
        return t

    bad = [
        ("item 1", lambda: hl.session_local([0, 1], [1, 4])),                                   # flags outside 0..3
        ("item 0", lambda: hl.session_local([0, 1], [-1, 1])),
        ("item 2", lambda: hl.session_local([0, 1, 0], [1, 1, 1])),                             # an id given twice
        ("item 1", lambda: hl.session_local([0, 13], [1, 1])),                                  # a session not opened
        ("item 1", lambda: hl.session_local([0, CAP], [1, 1])),                                 # an id outside the pool
        ("n = 0", lambda: hl.session_local([], [])),
        ("n = 257", lambda: hl.session_local(list(range(257)), [1] * 257)),
        (r"falloff64\[0\]", lambda: hl.sessions_set_local(table(d0=0.5), THRESH)),              # entry 0 is not 1.0
        (r"falloff64\[7\]", lambda: hl.sessions_set_local(table(d7=1.5), THRESH)),              # an entry outside [0,1]
        (r"falloff64\[63\]", lambda: hl.sessions_set_local(table(d63=-1e-3), THRESH)),
        (r"falloff64\[9\]", lambda: hl.sessions_set_local(table(d9=float("nan")), THRESH)),     # a NaN
    ]
    for needle, call in bad:
        refused(call, needle, -7)
        unchanged(needle)
    # the table that was set is still the one in use
    sl.paint([0], (40, 40, 44, 44), (200, 100, 50), weight=0.5)
    want = N.umask_paint(before[0]["UMASK"], (40, 40, 44, 44), good)
    assert np.array_equal(sl.read(0)["UMASK"], want) and not np.array_equal(want, before[0]["UMASK"])
    # -6: a pool without the reservation
    shown = np.full((1, 3, 64, 64), 7, np.uint8)
    for call in (lambda: hp.session_local([0, 1], [1, 1]), lambda: hp.sessions_set_local(good, THRESH),
                 lambda: hp.session_read(0, "UMASK"), lambda: hp.session_read(0, "LOCAL")):
        refused(call, "no local reservation", -6)
    # -6: a session with flags, but no falloff table yet (the reservation made through the C ABI alone)
    try:
        hp.sessions_reserve_local(True)
        hp.session_local([0, 2], [1, 0])
        z = np.ascontiguousarray(O.make_latents(1, seed=5), np.float32)
        for call in (lambda: hp.session_brush(events([1, 0]), shown), lambda: hp.session_set_latent(np.asarray([0], np.int32), z, 0, shown)):
            refused(call, "falloff table is not set", -6)
            assert np.all(shown == 7)
        for i, b in zip(ids, before_p):
            got = sp.read(i)
            assert_fields(got, b, KEYS64, i)
            assert not hp.session_read(i, "UMASK").any() and int(hp.session_read(i, "LOCAL")[0]) == (1 if i == 0 else 0)
        hp.session_brush(events([2, 1]), None)                            # sessions with flags 0 need no table
        assert not np.array_equal(sp.read(2)["Z"], before_p[2]["Z"]) and np.array_equal(sp.read(0)["Z"], before_p[0]["Z"])
    finally:
        hp.sessions_reserve_local(False)
    with pytest.raises(IanError, match="no local reservation"):
        hp.session_read(0, "UMASK")
    # the Python surface refuses the same before the library is called, and the pool still works
    with pytest.raises(ValueError):
        sl.set_local([0, 0])
    with pytest.raises(ValueError):
        sl.set_local([0], flags=4)
    with pytest.raises(ValueError, match="no local reservation"):
        sp.set_local([0])
    sl.set_local(ids, flags=0)
    for i in ids:
        assert sl.read(i)["LOCAL"] == 0


# ---- 7. both reservations through a resize: all eleven arrays move together -------------------------------------------------------
def test_resize_with_both_reservations_keeps_every_field_and_window():
    s, ids = 2, [1, 3]
    ml, sl, _, _ = pools()
    keys = KEYS64 + ("FIELD", "FIELD_KIND", "SOURCE", "UMASK", "LOCAL")
    try:
        sl.reserve(4)
        sl.reserve_hires(s)
        sl.open_hires(ids, H.sources(2, s, 81))
        sl.set_local(ids, flags=[1, 3])
        sl.paint(ids, (8, 8, 30, 30), (10, 200, 30), weight=0.5)
        before = [sl.read(i) for i in ids]
        assert all(set(b) == set(keys) and b["UMASK"].any() and b["FIELD"].any() for b in before)
        windows = sl.render(ids, (40, 36), 8)
        sl.reserve(7)
        for i, b in zip(ids, before):
            got = sl.read(i)
            assert_fields(got, b, keys, ("grown", i))
        assert np.array_equal(sl.render(ids, (40, 36), 8), windows)
        sl.open([6], sources(1, 82))
        got = sl.read(6)
        assert not got["UMASK"].any() and got["LOCAL"] == 0 and not got["FIELD"].any() and got["FIELD_KIND"] == 0
        sl.reserve(3)
        got = sl.read(1)
        assert_fields(got, before[0], keys, "shrunk")
        assert np.array_equal(sl.render([1], (40, 36), 8), windows[:1])
        refused(lambda: ml.handle.session_read(3, "Z"), "outside the pool", -7)
    finally:
        sl.reserve_hires(0)
        sl.reserve(CAP)

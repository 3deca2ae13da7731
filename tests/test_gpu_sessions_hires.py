"""Full-resolution edit sessions (ian_sessions_reserve_hires, ian_session_open_hires, ian_session_render, ian_session_brush_view;
EditSessions.reserve_hires / open_hires / render / brush_view).  Every comparison is np.array_equal: the numpy functions of npe_ops
(hires_downsample, edit_field, hires_axis_taps, hires_render) specify the arithmetic and the device matches them bit for bit; the
64x64 state is held against a second pool WITHOUT the reservation, driven by the existing calls, which shows they are unchanged."""
import numpy as np
import pytest

from oracle import ian_oracle as O
from session_helpers import KEYS64, assert_fields, const_rgb, model_pool, refused, session_events as events, session_views as views, sources

pytestmark = pytest.mark.gpu

CAP = 16

_cache = {}


def pools(arch="IAN_simple"):
    """Two models with the same synthetic parameters, one pool each: (model, full-resolution pool, model, plain pool).  The
    stateless calls of a test go to the SECOND model, so that the first handle sees session calls only (its residency survives)."""
    if arch not in _cache:
        _cache[arch] = model_pool(arch) + model_pool(arch)
    mh, sh, mp, sp = _cache[arch]
    if sh.capacity != CAP:
        sh.reserve(CAP)
    return mh, sh, mp, sp


def windows(S):
    """(x, y, vw, vh): interior, touching each of the four edges, vw = 4 / vh = 1, the whole picture (S >= 128)."""
    return [(40, 37, 64, 50), (0, 50, 32, 21), (S - 32, 60, 32, 21), (64, 0, 36, 9), (64, S - 11, 36, 11), (100, 77, 4, 1), (0, 0, S, S)]


def assert_renders(sh, ids, want, s, tag):
    """want[id] = (SOURCE, FIELD, KIND): every window of every session, n views per call, against npe_ops.hires_render."""
    from neural_photo_editor_amd import npe_ops as N
    for (x, y, vw, vh) in windows(64 * s):
        out = sh.render(ids, (x, y), (vw, vh))
        assert out.shape == (len(ids), 3, vh, vw) and out.dtype == np.uint8
        for k, i in enumerate(ids):
            src, field, kind = want[i]
            assert np.array_equal(out[k], N.hires_render(src, field, kind, s, x, y, vw, vh)), (tag, i, (x, y, vw, vh))


def assert_same64(a, b, tag):
    assert_fields(a, b, KEYS64, tag)


# ---- 1. open --------------------------------------------------------------------------------------------------------------------
def check_open_hires(s, n):
    """open_hires of n photos at scale s against the specification -> (the pool, ids, photos, what read() gave per session)."""
    from neural_photo_editor_amd import npe_ops as N
    _, sh, _, sp = pools()
    sh.reserve_hires(s)
    ids = [9, 2, 14][:n]
    src = sources(n, s, 10 * s + n)
    down = np.stack([N.hires_downsample(p, s) for p in src])
    shown = sh.open_hires(ids, src)
    shown_p = sp.open(ids, down)
    assert np.array_equal(shown, shown_p) and np.array_equal(shown, down)
    S = 64 * s
    state = []
    for k, i in enumerate(ids):
        got = sh.read(i)
        assert_same64(got, sp.read(i), (s, n, i))
        assert np.array_equal(got["GIM"], down[k])
        assert got["SOURCE"].shape == (3, S, S) and np.array_equal(got["SOURCE"], src[k])
        assert got["FIELD"].dtype == np.float32 and not got["FIELD"].any() and got["FIELD_KIND"] == 0
        state.append(got)
    whole = sh.render(ids, (0, 0), S)
    assert np.array_equal(whole, src)
    return sh, ids, src, state


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 3])
def test_open_hires_is_open_of_the_box_mean(s, n):
    check_open_hires(s, n)


def test_open_hires_at_scale_5_and_the_same_photo_placed_on_a_canvas():
    """s = 5: 80 lanes in a 128-lane workgroup, and a lane's four bytes straddle two 64x64 pixels at every phase (neither holds at
    1, 2, 3, 16).  Then the same photos as canvases, placed at (0, 0) and scale 5: the box mean's other entry leaves the same state."""
    from neural_photo_editor_amd import npe_ops as N
    s, n = 5, 2
    sh, ids, src, opened = check_open_hires(s, n)
    for p in src:                                                              # what the second half rests on, on the CPU
        assert np.array_equal(N.hires_downsample(p, s), N.canvas_crop_mean(p, 0, 0, s))
    sh.reserve_canvases(n, 64 * s, 64 * s, 0)
    try:
        for c, p in enumerate(src):
            sh.canvas_put(c, p)
        shown = sh.place(ids, list(range(n)), [(0, 0)] * n, s)
        for k, i in enumerate(ids):
            got = sh.read(i)
            assert np.array_equal(shown[k], opened[k]["IM"])
            for key in ("GIM", "IM", "Z"):
                assert np.array_equal(got[key], opened[k][key]), (key, i)
    finally:
        sh.reserve_canvases(0)


# ---- 2. the brush script ---------------------------------------------------------------------------------------------------------
def expected_fields(mp, M, ids, boxes, colours, modes, weight, sign):
    """The stateless call on the host-held state of sessions `ids` (as test_gpu_sessions.model_brush) -> {id: (FIELD, KIND)}; M's
    latents move on."""
    from neural_photo_editor_amd import npe_ops as N
    n = len(ids)
    z = np.stack([M[i]["Z"] for i in ids])
    rgb = np.stack([const_rgb(colours[k]) if modes[k] else np.zeros((3, 64, 64), np.float32) for k in range(n)])
    recon = np.stack([M[i]["RECON"] for i in ids])
    error = np.stack([M[i]["ERROR"] for i in ids])
    z_new, x, _, mask = mp.brush_step_batch(np.asarray(boxes), z, rgb, weight=weight, sign=sign, modes=modes, photo=(recon, error),
                                            want_mask=True)
    out = {}
    for k, i in enumerate(ids):
        M[i]["Z"] = z_new[k].copy()
        if M[i]["MODE"] == 0 and modes[k] == 1:
            out[i] = (N.edit_field(x[k], recon[k], error[k], mask[k]), 0)
        else:
            out[i] = (x[k].copy(), 1)
    return out


@pytest.mark.parametrize("arch", O.ARCHS)
def test_brush_script_fields_renders_and_unchanged_64_state(arch):
    from neural_photo_editor_amd import npe_ops as N
    s = 3
    _, sh, mp, sp = pools(arch)
    sh.reserve_hires(s)
    ids = [3, 11, 6, 0]
    src = sources(4, s, 77)
    down = np.stack([N.hires_downsample(p, s) for p in src])
    zs = O.make_latents(1, seed=5)
    rs = np.random.RandomState(31)

    def events(n, kind):
        c1, r1 = rs.randint(0, 50, n), rs.randint(0, 50, n)
        boxes = np.stack([c1, r1, c1 + rs.randint(4, 14, n), r1 + rs.randint(4, 14, n)], 1)
        modes = [1] * n if kind == "paint" else [0] * n
        weight = np.where(np.array(modes) == 1, 0.5, 0.3)               # large steps: fields well away from zero
        sign = np.where(np.array(modes) == 1, -1.0, rs.choice([-1.0, 1.0], n))
        return boxes, rs.randint(0, 256, (n, 3)), modes, weight, sign

    script = [("paint", ids), ("paint", ids), ("scroll", ids)]
    if arch == "IAN_simple":
        script += [("set_latent", ids), ("paint", [0, 3, 11])]           # a subset in another order
    for pool, first in ((sh, lambda: sh.open_hires(ids, src)), (sp, lambda: sp.open(ids, down))):
        first()
        pool.sample([6], zs)                                             # session 6 goes to sample mode
    M = {i: sp.read(i) for i in ids}
    want = {i: (src[k], np.zeros((3, 64, 64), np.float32), 0) for k, i in enumerate(ids)}
    want[6] = (src[2], sh.read(6)["FIELD"], 1)
    assert sh.read(6)["FIELD_KIND"] == 1
    for step, (kind, sel) in enumerate(script):
        if kind == "set_latent":
            z = O.make_latents(len(sel), seed=40 + step)
            xs = mp.sample_at(z)
            shown, shown_p = sh.set_latent(sel, z), sp.set_latent(sel, z)
            fields = {}
            for k, i in enumerate(sel):
                M[i]["Z"] = z[k].copy()
                if M[i]["MODE"] == 0:
                    mask = N.photo_blend_host(xs[k], M[i]["RECON"], M[i]["ERROR"])[1]
                    fields[i] = (N.edit_field(xs[k], M[i]["RECON"], M[i]["ERROR"], mask), 0)
                else:
                    fields[i] = (xs[k].copy(), 1)
        else:
            arg = events(len(sel), kind)
            fields = expected_fields(mp, M, sel, *arg)
            shown, shown_p = sh.brush(sel, *arg), sp.brush(sel, *arg)
        assert np.array_equal(shown, shown_p), (arch, step, kind)
        for i in sel:
            got, plain = sh.read(i), sp.read(i)
            assert np.array_equal(got["Z"], plain["Z"]) and np.array_equal(got["IM"], plain["IM"]), (arch, step, kind, i)
            assert np.array_equal(got["Z"], M[i]["Z"]), (arch, step, kind, i)
            assert got["FIELD_KIND"] == fields[i][1], (arch, step, kind, i)
            assert np.array_equal(got["FIELD"], fields[i][0]), (arch, step, kind, i)
            assert np.array_equal(got["SOURCE"], want[i][0])
            want[i] = (want[i][0], fields[i][0], fields[i][1])
        if kind == "paint":
            assert any(want[i][1].any() and want[i][2] == 0 for i in sel)
        assert_renders(sh, ids, want, s, (arch, step, kind))


def test_sample_sets_field_to_x_and_renders_the_upsampled_sample():
    s = 2
    _, sh, mp, _ = pools()
    sh.reserve_hires(s)
    ids = [4, 5]
    src = sources(2, s, 3)
    sh.open_hires(ids, src)
    z = O.make_latents(2, seed=8)
    sh.sample(ids, z)
    xs = mp.sample_at(z)
    want = {}
    for k, i in enumerate(ids):
        got = sh.read(i)
        assert got["FIELD_KIND"] == 1 and np.array_equal(got["FIELD"], xs[k])
        want[i] = (src[k], xs[k], 1)
    assert_renders(sh, ids, want, s, "sample")


# ---- 3. one submission -----------------------------------------------------------------------------------------------------------
def test_brush_view_is_brush_then_render():
    s = 3
    _, sh, _, _ = pools()
    sh.reserve_hires(s)
    A, B = [1, 7], [8, 2]
    src = sources(2, s, 13)
    sh.open_hires(A, src)
    sh.open_hires(B, src)
    boxes, colours = np.array([(10, 12, 30, 28), (33, 5, 50, 20)]), np.array([(250, 20, 20), (10, 240, 90)])
    origins, size = np.array([(40, 36), (96, 100)]), (88, 57)
    got = [sh.brush_view(A, boxes, colours, None, 0.5, -1.0, origins, size) for _ in range(2)]      # the second call hits residency
    got.append(sh.scroll(A, boxes, [1.0, -1.0], weight=0.3, view=(origins, size)))
    want = []
    for call in (lambda: sh.paint(B, boxes, colours, weight=0.5), lambda: sh.paint(B, boxes, colours, weight=0.5),
                 lambda: sh.scroll(B, boxes, [1.0, -1.0], weight=0.3)):
        shown = call()
        want.append((shown, sh.render(B, origins, size)))                 # a render keeps the residency: the second paint hits too
    for step, ((shown, out), (shown_w, out_w)) in enumerate(zip(got, want)):
        assert np.array_equal(shown, shown_w), step
        assert out.shape == (2, 3, 57, 88) and np.array_equal(out, out_w), step
    assert (got[0][1] != src[:, :, 36:36 + 57, 40:40 + 88][0]).any()       # the window shows an edit
    for a, b in zip(A, B):
        ga, gb = sh.read(a), sh.read(b)
        assert_fields(ga, gb, KEYS64 + ("FIELD", "FIELD_KIND", "SOURCE"))


# ---- 4. commit -------------------------------------------------------------------------------------------------------------------
def test_commit_renders_into_the_source():
    from neural_photo_editor_amd import npe_ops as N
    s = 3
    S = 64 * s
    _, sh, _, sp = pools()
    sh.reserve_hires(s)
    ids = [12, 5]
    src = sources(2, s, 21)
    down = np.stack([N.hires_downsample(p, s) for p in src])
    sh.open_hires(ids, src)
    sp.open(ids, down)
    for pool in (sh, sp):
        pool.paint(ids, (18, 20, 44, 40), (250, 10, 10), weight=0.5)
    before = sh.render(ids, (0, 0), S)
    assert (before != src).any()
    shown, shown_p = sh.commit(ids), sp.commit(ids)
    assert np.array_equal(shown, shown_p)
    for k, i in enumerate(ids):
        got = sh.read(i)
        assert np.array_equal(got["SOURCE"], before[k])
        assert not got["FIELD"].any() and got["FIELD_KIND"] == 0
        assert_same64(got, sp.read(i), ("commit", i))
    assert np.array_equal(sh.render(ids, (0, 0), S), before)
    # Reset re-opens from the stored GIM: the source stays
    sh.paint(ids, (5, 5, 20, 20), (10, 10, 250), weight=0.5)
    sh.reset(ids)
    for k, i in enumerate(ids):
        got = sh.read(i)
        assert np.array_equal(got["SOURCE"], before[k]) and not got["FIELD"].any()


# ---- 5. the largest scale ----------------------------------------------------------------------------------------------------------
def test_scale_16_whole_picture():
    from neural_photo_editor_amd import npe_ops as N
    s = 16
    _, sh, _, sp = pools()
    sh.reserve_hires(s)
    try:
        src = sources(1, s, 16)
        shown = sh.open_hires([15], src)
        assert np.array_equal(shown[0], N.hires_downsample(src[0], s))
        assert np.array_equal(sh.render([15], (0, 0), 1024)[0], src[0])
        sp.open([15], shown)
        shown, out = sh.paint([15], (20, 20, 44, 44), (240, 30, 30), weight=0.5, view=((0, 0), 1024))
        assert np.array_equal(shown, sp.paint([15], (20, 20, 44, 44), (240, 30, 30), weight=0.5))
        got = sh.read(15)
        assert got["FIELD"].any() and got["FIELD_KIND"] == 0 and np.array_equal(got["SOURCE"], src[0])
        assert np.array_equal(out[0], N.hires_render(src[0], got["FIELD"], 0, s, 0, 0, 1024, 1024))
        assert (out[0] != src[0]).any()
        # the last band of a window whose height is no multiple of the band, at the bottom edge
        assert np.array_equal(sh.render([15], (512, 1024 - 13), (256, 13))[0], out[0][:, 1024 - 13:, 512:768])
    finally:
        sh.reserve_hires(0)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_change_nothing():
    s = 2
    S = 64 * s
    mh, sh, mp, sp = pools()
    sh.reserve_hires(s)
    h = mh.handle
    ids = [0, 1, 2]
    sh.open_hires(ids, sources(3, s, 55))
    sh.paint(ids, (10, 10, 30, 30), (200, 100, 50), weight=0.5)
    sh.open([3], sources(1, 1, 56))                                       # opened, but without a source
    before = [sh.read(i) for i in ids]
    out = np.full((2, 3, 16, 16), 7, np.uint8)
    shown = np.full((2, 3, 64, 64), 7, np.uint8)

    ok = [(0, 0, 0), (1, 0, 0)]
    bad = [
        ("n = 0", lambda: h.session_render(views([]), 16, 16, out)),                              # n outside 1..256
        ("n = 257", lambda: h.session_render(views([(0, 0, 0)] * 257), 16, 16, out)),
        ("item 1", lambda: h.session_render(views([(0, 0, 0), (CAP, 0, 0)]), 16, 16, out)),       # an id outside the pool
        ("item 1", lambda: h.session_render(views([(0, 0, 0), (-1, 0, 0)]), 16, 16, out)),
        ("item 1", lambda: h.session_render(views([(0, 0, 0), (13, 0, 0)]), 16, 16, out)),        # a session not opened
        ("item 0", lambda: h.session_render(views([(3, 0, 0), (0, 0, 0)]), 16, 16, out)),         # a session without a source
        ("at least 1", lambda: h.session_render(views(ok), 0, 16, out)),                          # vw < 1
        ("at least 1", lambda: h.session_render(views(ok), 16, 0, out)),                          # vh < 1
        ("at least 1", lambda: h.session_render(views(ok), -4, 16, out)),
        ("item 1", lambda: h.session_render(views([(0, 0, 0), (1, S - 12, 0)]), 16, 16, out)),    # a window not inside S x S
        ("item 1", lambda: h.session_render(views([(0, 0, 0), (1, 0, S - 15)]), 16, 16, out)),
        ("item 0", lambda: h.session_render(views([(0, -4, 0), (1, 0, 0)]), 16, 16, out)),
        ("item 0", lambda: h.session_render(views([(0, 0, -1), (1, 0, 0)]), 16, 16, out)),
        ("item 0", lambda: h.session_render(views(ok), S + 4, 16, out)),
        ("item 1", lambda: h.session_render(views([(0, 0, 0), (1, 2, 0)]), 16, 16, out)),         # x not a multiple of 4
        ("multiple of 4", lambda: h.session_render(views(ok), 18, 16, out)),                      # vw not a multiple of 4
        ("item 1", lambda: h.session_brush_view(events([0, 1]), views([(0, 0, 0), (2, 0, 0)]), 16, 16, out, shown)),   # view != event
        ("item 1", lambda: h.session_brush_view(events([0, 3]), views([(0, 0, 0), (3, 0, 0)]), 16, 16, out, shown)),   # no source
        ("item 0", lambda: h.session_brush_view(events([0, 1]), views([(0, 2, 0), (1, 0, 0)]), 16, 16, out, shown)),
        ("item 1", lambda: h.session_brush_view(events([0, 0]), views([(0, 0, 0), (0, 0, 0)]), 16, 16, out, shown)),   # the event's checks
    ]
    for needle, call in bad:
        refused(call, needle, -7)
        assert np.all(out == 7) and np.all(shown == 7)
        for i, b in zip(ids, before):
            got = sh.read(i)
            assert_fields(got, b, ("SOURCE", "FIELD", "Z"), (needle, i))
    # -6: a pool without the reservation
    hp = mp.handle
    sp.open([0, 1], sources(2, 1, 57))
    no_res = [
        lambda: hp.session_render(views(ok), 16, 16, out),
        lambda: hp.session_brush_view(events([0, 1]), views(ok), 16, 16, out, shown),
        lambda: hp.session_open_hires(np.asarray([0], np.int32), sources(1, 1, 58), None),
        lambda: hp.session_read(0, "FIELD"),
        lambda: hp.session_read(0, "SOURCE", scale=1),
    ]
    z0 = sp.read(0)["Z"]
    for call in no_res:
        refused(call, "no full-resolution reservation", -6)
    assert np.all(out == 7) and np.array_equal(sp.read(0)["Z"], z0)
    # the Python surface refuses the same before the library is called, and the handle still works
    with pytest.raises(ValueError):
        sh.render([0, 3], (0, 0), 16)
    got = sh.render(ids, (16, 16), 16)
    assert got.shape == (3, 3, 16, 16) and (got != 7).any()


# ---- 7. pool upkeep --------------------------------------------------------------------------------------------------------------
def test_pool_upkeep_keeps_sources_and_fields():
    from neural_photo_editor_amd.lib import IanError
    s = 2
    S = 64 * s
    mh, sh, _, _ = pools()
    sh.reserve_hires(s)
    ids = [1, 6]
    src = sources(2, s, 71)
    sh.open_hires(ids, src)
    sh.paint(ids, (8, 8, 30, 30), (10, 200, 30), weight=0.5)
    before = [sh.read(i) for i in ids]
    whole = sh.render(ids, (0, 0), S)
    one = views([(6, 0, 0)])
    out = np.empty((1, 3, 8, 8), np.uint8)
    try:
        sh.reserve(40)                                                        # growing keeps the rows
        for i, b in zip(ids, before):
            got = sh.read(i)
            assert_fields(got, b, KEYS64 + ("SOURCE", "FIELD", "FIELD_KIND"), ("grown", i))
        sh.open_hires([39], src[:1])
        assert np.array_equal(sh.render([39, 1], (0, 0), S), np.stack([src[0], whole[0]]))
        sh.reserve(4)                                                         # shrinking keeps the ids that remain
        got = sh.read(1)
        assert_fields(got, before[0], KEYS64 + ("SOURCE", "FIELD", "FIELD_KIND"), "shrunk")
        assert np.array_equal(sh.render([1], (0, 0), S)[0], whole[0])
        refused(lambda: mh.handle.session_render(one, 8, 8, out), "outside the pool", -7)
    finally:
        sh.reserve(CAP)
    # a plain open clears the source flag
    sh.open_hires([6], src[1:])
    mh.handle.session_render(one, 8, 8, out)
    assert np.array_equal(out[0], src[1][:, :8, :8])
    sh.open([6], src[1:, :, :64, :64].copy())
    refused(lambda: mh.handle.session_render(one, 8, 8, out), "no full-resolution source", -7)
    assert "SOURCE" not in sh.read(6) and not sh.read(6)["FIELD"].any()
    # reserve_hires(0) frees; the 64x64 state stays
    z1 = sh.read(1)["Z"]
    sh.reserve_hires(0)
    one[0].session = 1
    refused(lambda: mh.handle.session_render(one, 8, 8, out), "no full-resolution reservation", -6)
    got = sh.read(1)
    assert np.array_equal(got["Z"], z1) and "FIELD" not in got
    # and back: a new reservation starts without sources
    sh.reserve_hires(s)
    with pytest.raises(IanError, match="no full-resolution source"):
        mh.handle.session_render(one, 8, 8, out)


# ---- 8. another scale, and the whole pool freed -------------------------------------------------------------------------------------
def test_scale_change_keeps_fields_and_drops_sources():
    mh, sh, _, _ = pools()
    sh.reserve_hires(1)
    sh.open_hires([5], sources(1, 1, 91))
    sh.paint([5], (8, 8, 30, 30), (10, 200, 30), weight=0.5)
    before = sh.read(5)
    assert before["FIELD"].any() and "SOURCE" in before
    sh.reserve_hires(2)
    got = sh.read(5)
    assert "SOURCE" not in got
    assert_fields(got, before, KEYS64 + ("FIELD", "FIELD_KIND"))
    refused(lambda: mh.handle.session_render(views([(5, 0, 0)]), 8, 8, np.empty((1, 3, 8, 8), np.uint8)), "no full-resolution source", -7)
    big = sources(1, 2, 92)
    sh.open_hires([5], big)
    assert np.array_equal(sh.render([5], (0, 0), 128), big)


def test_free_and_come_back_keeps_the_blend_and_drops_both_reservations():
    """On the raw handle: ian_sessions_reserve(0), then a pool again without ian_sessions_set_blend."""
    mh, sh, mp, sp = pools()
    h, ids, ph = mh.handle, np.asarray([2], np.int32), sources(1, 1, 95)
    sh.reserve_hires(2)
    sh.reserve_local()
    try:
        h.sessions_reserve(0)
        refused(lambda: h.session_read(2, "Z"), "no session pool", -6)
        h.sessions_reserve(4)
        shown, want = np.empty((1, 3, 64, 64), np.uint8), np.empty((1, 3, 64, 64), np.uint8)
        for hd, out in ((h, shown), (mp.handle, want)):
            hd.session_open(ids, ph, 0, out)
            hd.session_brush(events([2], box=(8, 8, 30, 30)), out)
        assert np.array_equal(shown, want)
        refused(lambda: h.session_read(2, "FIELD"), "no full-resolution reservation", -6)
        refused(lambda: h.session_read(2, "UMASK"), "no local reservation", -6)
    finally:
        _cache["IAN_simple"] = (mh, mh.sessions(CAP), mp, sp)

"""The edge-aware compose (ian_sessions_reserve_edges, ian_sessions_edges; EditSessions.reserve_canvas_guide / canvas_guide).  Every
comparison is np.array_equal against npe_ops.canvas_compose_guided, whose inputs (the canvas, and FIELD, FIELD_KIND and GIM of every
placed session) are read back from the pool after paint events that leave non-zero fields: the numpy function specifies the
arithmetic and the device matches it bit for bit.  A second, plain pool renders the crop under ian_sessions_reserve_guide with the
same table.  The canvas is 268 x 203 in a 272 x 210 reservation, so a row's stride is not its width."""
import numpy as np
import pytest

from neural_photo_editor_amd import npe_ops as N
from oracle import ian_oracle as O
from session_helpers import KEYS64, assert_fields, model_pool, refused

pytestmark = pytest.mark.gpu

CAP = 16
W, H = 268, 203
MAXW, MAXH = 272, 210
KEYS = KEYS64 + ("FIELD", "FIELD_KIND")

_cache = {}


def picture(w, h, seed):
    """A smooth picture plus noise, as session_helpers.sources makes them, at any size."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127.5 + 100.0 * np.sin(xx / 9.0 + rs.uniform(0, 6, (3, 1, 1))) * np.cos(yy / 11.0 + rs.uniform(0, 6, (3, 1, 1)))
    return np.uint8(np.clip(base + rs.randint(-40, 41, (3, h, w)), 0, 255))


def pools(f=4, count=1, max_w=MAXW, max_h=MAXH, sigma=8.0):
    """Two models with the same synthetic parameters: (the pool with canvases, a plain pool, the table).  Every test starts from a fresh
    canvas reservation with the edge-aware compose on (sigma None: off), and a plain pool without reservations."""
    if "p" not in _cache:
        _cache["p"] = model_pool("IAN_simple") + model_pool("IAN_simple")
    mh, sh, mp, sp = _cache["p"]
    if sh.canvases:
        sh.reserve_canvases(0)
    if not sh.scale:
        sh.reserve_hires(1)
    sh.reserve_canvases(count, max_w, max_h, f)
    assert sh.canvas_guide() is None and not sh.canvas_guided               # a new reservation starts with the plain compose
    table = None
    if sigma is not None:
        table = N.guide_table(sigma)
        sh.reserve_canvas_guide(table=table)
    if sp.scale:
        sp.reserve_guide()
        sp.reserve_hires(0)
    return sh, sp, table


def placed_fields(sh, cid=0):
    """What canvas_compose_guided takes for one canvas, read back from the sessions placed on it."""
    out = []
    for (i, x, y, s) in sh.placements(cid):
        got = sh.read(i)
        out.append((x, y, s, got["FIELD"], int(got["FIELD_KIND"]), got["GIM"]))
    return out


def plain(placed):
    return [p[:5] for p in placed]


def windows(ox, oy, S, w=W, h=H):
    """test_gpu_canvas's list, (x, y, vw, vh) around the square (ox, oy) + S: its interior, across each of its four edges, a strip at the
    top right, vw = 4 / vh = 1, a height that is no multiple of the band, the canvas's last row and last 4 columns, the whole canvas."""
    a = (ox + 3) // 4 * 4
    return [(a + 8, oy + 9, 40, 30), (max(a - 12, 0), oy + 20, 24, 10), (min((ox + S) // 4 * 4 - 8, w - 24), oy + 20, 24, 10),
            (a + 4, max(oy - 5, 0), 36, 11), (a + 4, min(oy + S - 6, h - 11), 36, 11), (240, 0, 28, 5), (a + 16, oy + 31, 4, 1),
            (a, oy + 2, 64, 13), (w - 4, h - 1, 4, 1), (0, 0, w, h)]


def paint_all(sh, ids, seed=0):
    """One paint event per session that leaves a non-zero field."""
    n = len(ids)
    boxes = np.array([(6 + 5 * (k % 4), 8 + 3 * (k % 5), 34 + 3 * (k % 6), 40 + 2 * (k % 7)) for k in range(n)])
    colours = np.random.RandomState(seed).randint(0, 256, (n, 3))
    shown = sh.paint(ids, boxes, colours, weight=0.5)
    for i in ids:
        assert sh.read(i)["FIELD"].any(), i
    return boxes, colours, shown


def assert_composes(sh, c, table, wins, tag):
    """Every window against npe_ops.canvas_compose_guided of the whole canvas, computed once (a window is its crop: the host test)."""
    want = placed_fields(sh)
    whole = N.canvas_compose_guided(c, want, sh.feather, 0, 0, c.shape[2], c.shape[1], table)
    for (x, y, vw, vh) in sorted(set(wins)):
        out = sh.compose([0], (x, y), (vw, vh))
        assert out.shape == (1, 3, vh, vw) and out.dtype == np.uint8
        assert np.array_equal(out[0], whole[:, y:y + vh, x:x + vw]), (tag, (x, y, vw, vh))
    return want, whole


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 4])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_every_alignment_and_window_matches_the_specification(s, f):
    sh, _, table = pools(f=f)
    S = 64 * s
    c = picture(W, H, 100 + s)
    sh.canvas_put(0, c)
    origins = [(4, 3), (1, 0), (2, H - S), (W - S - 1, 1)]                     # ox % 4 = 0, 1, 2, 3; squares at the canvas's edges
    assert [ox % 4 for ox, _ in origins] == [0, 1, 2, 3]
    ids = [9, 2, 14, 0]
    sh.place(ids, 0, origins, s)
    paint_all(sh, ids, s)
    wins = [w for (ox, oy) in origins[1::2] for w in windows(ox, oy, S)]
    want, whole = assert_composes(sh, c, table, wins, (s, f))
    assert (whole != c).any()
    old = N.canvas_compose(c, plain(want), f, 0, 0, W, H)
    if s >= 2:                                                                # at scale 1 only one tap has spatial weight
        assert (whole != old).any()                                           # in numpy first: these inputs tell the two composes apart
        assert (sh.compose([0], (0, 0), (W, H))[0] != old).any()              # ... and the guided kernel ran
    assert np.array_equal(sh.canvas_read(0), c)                               # a compose stores nothing


def test_a_photo_mode_and_a_sample_mode_placement_overlapping():
    sh, _, table = pools()
    c = picture(W, H, 77)
    sh.canvas_put(0, c)
    squares = {3: (5, 7, 2), 11: (70, 40, 2), 6: (47, 9, 3)}                   # 3 and 11 overlap; 6 covers both and goes to sample mode
    ids = list(squares)
    sh.place(ids, 0, [squares[i][:2] for i in ids], [squares[i][2] for i in ids])
    sh.sample([6], O.make_latents(1, seed=5))
    paint_all(sh, [3, 11], 1)
    wins = [w for (ox, oy, s) in squares.values() for w in windows(ox, oy, 64 * s)]
    want, whole = assert_composes(sh, c, table, wins, "mixed")
    assert [p[4] for p in want] == [0, 1, 0] and (whole != N.canvas_compose(c, plain(want), 4, 0, 0, W, H)).any()
    inside = np.zeros((H, W), bool)
    for (ox, oy, s) in squares.values():
        inside[oy:oy + 64 * s, ox:ox + 64 * s] = True
    assert np.array_equal(whole[:, ~inside], c[:, ~inside])


def test_eight_placements_in_one_band():
    """Eight scale-1 squares stepped 25 pixels along one row: every band of rows 40..103 keeps all 8, the kernel's whole LDS budget."""
    sh, _, table = pools()
    c = picture(W, H, 31)
    sh.canvas_put(0, c)
    ids = [1, 3, 4, 7, 8, 10, 12, 15]
    origins = [(3 + 25 * k, 40) for k in range(8)]
    sh.place(ids, 0, origins, 1)
    paint_all(sh, ids, 2)
    assert len(sh.placements(0)) == 8
    want, whole = assert_composes(sh, c, table, [(0, 0, W, H), (0, 60, W, 9), (100, 38, 64, 7), (176, 101, 92, 6)], "eight")
    assert (whole[:, 40:104, 178:242] != c[:, 40:104, 178:242]).any()         # the eighth square shows its edit
    # scale 1: one tap, (w*f)/w -- not promised to be f, so no equality with canvas_compose is asserted; it is close to it
    old = N.canvas_compose(c, plain(want), 4, 0, 0, W, H)
    assert np.abs(whole.astype(int) - old.astype(int)).max() <= 1


def test_scale_16():
    w, h, s, ox, oy = 1100, 1040, 16, 75, 15                                  # ox % 4 = 3; the square ends at column 1098 and row 1038
    sh, _, table = pools(max_w=w, max_h=h)
    c = picture(w, h, 116)
    sh.canvas_put(0, c)
    sh.place([15], 0, (ox, oy), s)
    paint_all(sh, [15], 3)
    wins = [(w - 256, h - 13, 256, 13), (w - 24, 500, 24, 10), (0, 0, w, h)]   # across the square's right edge; the whole canvas
    want, whole = assert_composes(sh, c, table, wins, "scale 16")
    assert (whole != N.canvas_compose(c, plain(want), 4, 0, 0, w, h)).any()
    assert np.array_equal(whole[:, :, ox + 1024:], c[:, :, ox + 1024:]) and np.array_equal(whole[:, :oy], c[:, :oy])


# ---- 2. the render kernel gives the same bytes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 4])
def test_the_compose_of_a_lone_placement_is_the_guided_render_of_the_crop(f):
    s, S, ox, oy, i = 2, 128, 75, 10, 4                                       # ox % 4 = 3
    sh, sp, table = pools(f=f)
    c = picture(W, H, 50)
    sh.canvas_put(0, c)
    crop = np.ascontiguousarray(c[:, oy:oy + S, ox:ox + S])
    sp.reserve_hires(s)
    sp.reserve_guide(table=table)
    try:
        shown = sh.place([i], 0, (ox, oy), s)
        assert np.array_equal(shown, sp.open_hires([i], crop[None]))
        boxes, colours, shown = paint_all(sh, [i], 4)
        assert np.array_equal(shown, sp.paint([i], boxes, colours, weight=0.5))
        assert_fields(sh.read(i), sp.read(i), KEYS)
        render = sp.render([i], (0, 0), S)[0]
        whole = sh.compose([0], (0, 0), (W, H))[0]
        m = f * s
        assert np.array_equal(whole[:, oy + m:oy + S - m, ox + m:ox + S - m], render[:, m:S - m, m:S - m])
        assert (render != crop).any()
        if f:
            assert not np.array_equal(whole[:, oy:oy + S, ox:ox + S], render)   # the rim is feathered
    finally:
        sp.reserve_guide()
        sp.reserve_hires(0)


# ---- 3. the reservation -----------------------------------------------------------------------------------------------------------
def two_overlapping(sh, c, seed):
    ids = [2, 9]
    sh.canvas_put(0, c)
    sh.place(ids, 0, [(5, 7), (70, 40)], [2, 2])
    paint_all(sh, ids, seed)
    return ids


def test_zero_fields_return_the_canvas_bytes():
    sh, _, table = pools()
    c = picture(W, H, 8)
    sh.canvas_put(0, c)
    sh.place([2, 9, 5], 0, [(5, 7), (70, 40), (47, 9)], [2, 2, 3])
    assert np.array_equal(sh.canvas_guide(), table)
    assert np.array_equal(sh.compose([0], (0, 0), (W, H))[0], c)
    assert np.array_equal(sh.compose([0], (44, 3), (100, 9))[0], c[:, 3:12, 44:144])


def test_replacing_the_table_and_switching_the_guide_off():
    sh, _, _ = pools(sigma=None)
    c = picture(W, H, 5)
    two_overlapping(sh, c, 5)
    want = placed_fields(sh)
    win = (40, 37, 64, 50)
    off = N.canvas_compose(c, plain(want), 4, *win)
    assert sh.canvas_guide() is None
    assert np.array_equal(sh.compose([0], win[:2], win[2:])[0], off)
    outs = {}
    for sigma in (4.0, 16.0):                                                 # the second call replaces the table
        sh.reserve_canvas_guide(sigma)
        t = sh.canvas_guide()
        assert t.dtype == np.float32 and np.array_equal(t, N.guide_table(sigma)) and sh.canvas_guided
        outs[sigma] = sh.compose([0], win[:2], win[2:])[0]
        assert np.array_equal(outs[sigma], N.canvas_compose_guided(c, want, 4, *win, t)), sigma
    assert (outs[4.0] != outs[16.0]).any() and (outs[4.0] != off).any()
    custom = np.linspace(1.0, 0.25, 766).astype(np.float32)                   # any positive table, not only a Gaussian
    sh.reserve_canvas_guide(table=custom)
    assert np.array_equal(sh.canvas_guide(), custom)
    out = sh.compose([0], win[:2], win[2:])[0]
    assert np.array_equal(out, N.canvas_compose_guided(c, want, 4, *win, custom)) and (out != outs[4.0]).any()
    sh.reserve_canvas_guide()
    assert sh.canvas_guide() is None and not sh.canvas_guided
    assert np.array_equal(sh.compose([0], win[:2], win[2:])[0], off)          # back to npe_ops.canvas_compose's bytes
    for k, (i, _, _, _) in enumerate(sh.placements(0)):                        # a compose, guided or not, changes no session
        got = sh.read(i)
        assert np.array_equal(got["FIELD"], want[k][3]) and np.array_equal(got["GIM"], want[k][5])


def test_brush_compose_is_brush_then_compose():
    sh, _, table = pools(count=2)
    c = picture(W, H, 13)
    sh.canvas_put(0, c)
    sh.canvas_put(1, c)
    X, Y = [1, 7], [2, 8]
    origins, scales = [(5, 7), (70, 40)], [2, 2]
    sh.place(X, 0, origins, scales)
    sh.place(Y, 1, origins, scales)
    boxes, colours = np.array([(10, 12, 30, 28), (33, 5, 50, 20)]), np.array([(250, 20, 20), (10, 240, 90)])
    win0 = ([0, 0], [(0, 0), (132, 100)], (136, 103))
    win1 = ([1, 1], [(0, 0), (132, 100)], (136, 103))
    shown, out = sh.brush_compose(X, boxes, colours, None, 0.5, -1.0, windows=win0)
    shown_w = sh.paint(Y, boxes, colours, weight=0.5)
    out_w = sh.compose(*win1)
    assert np.array_equal(shown, shown_w) and out.shape == (2, 3, 103, 136) and np.array_equal(out, out_w)
    for a, b in zip(X, Y):
        assert_fields(sh.read(a), sh.read(b), KEYS)
    want = placed_fields(sh, 0)
    for k, (x, y) in enumerate(win0[1]):
        assert np.array_equal(out[k], N.canvas_compose_guided(c, want, 4, x, y, 136, 103, table)), k
    assert (out[0] != N.canvas_compose(c, plain(want), 4, 0, 0, 136, 103)).any()


def test_canvas_commit_composes_the_guided_picture_in_place():
    sh, _, table = pools()
    c = picture(W, H, 21)
    ids = two_overlapping(sh, c, 6)
    placed = placed_fields(sh)
    want = N.canvas_compose_guided(c, placed, 4, 0, 0, W, H, table)
    assert (want != N.canvas_compose(c, plain(placed), 4, 0, 0, W, H)).any()
    shown = sh.canvas_commit(0)
    assert np.array_equal(sh.canvas_read(0), want)                            # in place: every lane stored what the compose gives
    down = np.stack([N.canvas_crop_mean(want, x, y, s) for (x, y, s, _, _, _) in placed])
    assert np.array_equal(shown, down)
    for k, i in enumerate(sorted(ids)):
        got = sh.read(i)
        assert np.array_equal(got["GIM"], down[k]) and np.array_equal(got["IM"], down[k]), i
        assert not got["FIELD"].any() and got["FIELD_KIND"] == 0
    assert np.array_equal(sh.compose([0], (0, 0), (W, H))[0], want)           # zero fields on the new canvas
    assert np.array_equal(sh.canvas_guide(), table)


def test_refusals_return_their_code_and_leave_the_table_in_force():
    sh, sp, table = pools()
    mh, _, mp, _ = _cache["p"]
    h = mh.handle
    c = picture(W, H, 55)
    two_overlapping(sh, c, 7)
    before = sh.compose([0], (0, 0), (W, H))[0]
    bad_zero, bad_nan, bad_neg, bad_inf = (table.copy() for _ in range(4))
    bad_zero[700], bad_nan[0], bad_neg[765], bad_inf[3] = 0.0, np.nan, -1.0, np.inf
    refused(lambda: h.sessions_reserve_edges(np.ones(5, np.float32)), "count 5", -7)
    refused(lambda: h.sessions_reserve_edges(np.ones(767, np.float32)), "count 767", -7)
    refused(lambda: h.sessions_reserve_edges(bad_zero), r"table\[700\]", -7)
    refused(lambda: h.sessions_reserve_edges(bad_nan), r"table\[0\]", -7)
    refused(lambda: h.sessions_reserve_edges(bad_neg), r"table\[765\]", -7)
    refused(lambda: h.sessions_reserve_edges(bad_inf), r"table\[3\]", -7)
    refused(lambda: h._check(h.lib.ian_sessions_reserve_edges(h._h, None, 766)), "null table", -7)
    assert np.array_equal(sh.canvas_guide(), table) and np.array_equal(sh.compose([0], (0, 0), (W, H))[0], before)
    refused(lambda: h.sessions_reserve_guide(table), "canvases are reserved", -6)   # the two older refusals stand as they were
    assert np.array_equal(sh.canvas_guide(), table)
    # -6: a pool without canvases
    hp = mp.handle
    refused(lambda: hp.sessions_reserve_edges(table), "no canvas reservation", -6)
    refused(lambda: hp.sessions_reserve_edges(None), "no canvas reservation", -6)
    refused(lambda: hp.sessions_edges(), "no canvas reservation", -6)
    with pytest.raises(ValueError, match="no canvas"):
        sp.reserve_canvas_guide(4.0)
    sp.reserve_hires(1)
    sp.reserve_guide(table=table)
    try:
        refused(lambda: hp.sessions_reserve_canvas(1, 128, 128, 0), "a guide is reserved", -6)
        refused(lambda: hp.sessions_reserve_edges(table), "no canvas reservation", -6)
    finally:
        sp.reserve_guide()
        sp.reserve_hires(0)
    # a new reservation of any count, and the end of the pool's canvases, free the table
    sh.reserve_canvases(1, MAXW, MAXH, 4)
    assert sh.canvas_guide() is None and h.sessions_edges() is None
    sh.reserve_canvas_guide(table=table)
    sh.reserve_canvases(0)
    refused(lambda: h.sessions_edges(), "no canvas reservation", -6)


def test_the_table_is_no_session_state():
    sh, _, table = pools()
    c = picture(W, H, 91)
    ids, other = two_overlapping(sh, c, 8), [10, 1]
    info = sh.record_info()
    before = sh.compose([0], (0, 0), (W, H))[0]
    got = {i: sh.read(i) for i in ids}
    rec = sh.save(ids)
    sh.load(other, rec)                                                       # into ids that are not placed: a load un-places
    assert sh.record_info() == info and np.array_equal(sh.canvas_guide(), table)
    for a, b in zip(ids, other):
        assert_fields(sh.read(b), got[a], KEYS)
        assert_fields(sh.read(a), got[a], KEYS)
    assert np.array_equal(sh.compose([0], (0, 0), (W, H))[0], before)
    sh.reserve_canvas_guide()
    assert sh.record_info() == info                                           # the layout does not know the table either
    assert np.array_equal(sh.compose([0], (0, 0), (W, H))[0], N.canvas_compose(c, plain(placed_fields(sh)), 4, 0, 0, W, H))

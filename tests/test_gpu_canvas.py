"""Canvases (ian_sessions_reserve_canvas, ian_canvas_put / _place / _compose / _brush / _commit / _read / _placements;
EditSessions.reserve_canvases / canvas_put / place / compose / brush_compose / canvas_commit).  Every comparison is np.array_equal:
the numpy functions of npe_ops (canvas_crop_mean, canvas_ramp, canvas_compose) specify the arithmetic and the device matches them
bit for bit; the 64x64 state is held against a second, plain pool driven by the existing calls, which shows they are unchanged.
The canvas is 268 x 203 in a 272 x 210 reservation, so a row's stride is not its width."""
import numpy as np
import pytest

from neural_photo_editor_amd import lib as L
from neural_photo_editor_amd import npe_ops as N
from oracle import ian_oracle as O
from session_helpers import KEYS64, assert_fields, model_pool, refused, session_events as events

pytestmark = pytest.mark.gpu

CAP = 16
W, H = 268, 203
MAXW, MAXH = 272, 210

_cache = {}


def picture(w, h, seed):
    """A smooth picture plus noise, as session_helpers.sources makes them, at any size."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127.5 + 100.0 * np.sin(xx / 9.0 + rs.uniform(0, 6, (3, 1, 1))) * np.cos(yy / 11.0 + rs.uniform(0, 6, (3, 1, 1)))
    return np.uint8(np.clip(base + rs.randint(-40, 41, (3, h, w)), 0, 255))


def pools(f=4, count=1, max_w=MAXW, max_h=MAXH, depth=0):
    """Two models with the same synthetic parameters: (model, the pool with canvases, model, a plain pool).  Every test starts from a
    fresh canvas reservation; the stateless calls of a test go to the SECOND model."""
    if "p" not in _cache:
        _cache["p"] = model_pool("IAN_simple") + model_pool("IAN_simple")
    mh, sh, mp, sp = _cache["p"]
    if sh.capacity != CAP:
        sh.reserve(CAP)
    if sh.canvases:
        sh.reserve_canvases(0)
    if not sh.scale:
        sh.reserve_hires(1)
    for p in (sh, sp):
        if p.history_depth != depth:
            p.reserve_history(depth)
    sh.reserve_canvases(count, max_w, max_h, f)
    return mh, sh, mp, sp


def placed_fields(sh, cid):
    """What canvas_compose takes for one canvas, read back from the sessions placed on it."""
    return [(x, y, s, sh.read(i)["FIELD"], sh.read(i)["FIELD_KIND"]) for (i, x, y, s) in sh.placements(cid)]


def windows(ox, oy, S):
    """(x, y, vw, vh) on the 268 x 203 canvas around the square (ox, oy) + S: its interior, across each of its four edges, a strip that
    meets no square of the brush script, vw = 4 / vh = 1, a height that is no multiple of the band, the canvas's last row and last 4
    columns, the whole canvas."""
    a = (ox + 3) // 4 * 4
    return [(a + 8, oy + 9, 40, 30), (max(a - 12, 0), oy + 20, 24, 10), (min((ox + S) // 4 * 4 - 8, W - 24), oy + 20, 24, 10),
            (a + 4, max(oy - 5, 0), 36, 11), (a + 4, min(oy + S - 6, H - 11), 36, 11), (240, 0, 28, 5), (a + 16, oy + 31, 4, 1),
            (a, oy + 2, 64, 13), (W - 4, H - 1, 4, 1), (0, 0, W, H)]


def assert_composes(sh, c, squares, tag, cid=0):
    """Every window of every square in `squares` [(ox, oy, S)] against npe_ops.canvas_compose of the fields read back."""
    want = placed_fields(sh, cid)
    wins = sorted({w for (ox, oy, S) in squares for w in windows(ox, oy, S)})
    for (x, y, vw, vh) in wins:
        out = sh.compose([cid], (x, y), (vw, vh))
        assert out.shape == (1, 3, vh, vw) and out.dtype == np.uint8
        assert np.array_equal(out[0], N.canvas_compose(c, want, sh.feather, x, y, vw, vh)), (tag, (x, y, vw, vh))


# ---- 1. place --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3])
def test_place_is_open_of_the_box_mean_at_every_alignment(s):
    mh, sh, _, sp = pools()
    S = 64 * s
    c = picture(W, H, 100 + s)
    sh.canvas_put(0, c)
    assert np.array_equal(sh.canvas_read(0), c)
    # ox % 4 = 0, 1, 2, 3, 0; squares touching the left, top, bottom and right edges of the canvas
    origins = [(0, 3), (1, 0), (2, H - S), (W - S - 1, 1), (W - S, min(7, H - S))]
    ids = [9, 2, 14, 0, 5]
    down = np.stack([N.canvas_crop_mean(c, ox, oy, s) for (ox, oy) in origins])
    shown = sh.place(ids, 0, origins, s)
    shown_p = sp.open(ids, down)
    assert np.array_equal(shown, down) and np.array_equal(shown, shown_p)
    for k, i in enumerate(ids):
        got = sh.read(i)
        assert np.array_equal(got["GIM"], down[k]), (s, i)
        assert_fields(got, sp.read(i), KEYS64, (s, i))
        assert got["FIELD"].dtype == np.float32 and not got["FIELD"].any() and got["FIELD_KIND"] == 0 and "SOURCE" not in got
    assert mh.handle.canvas_placements(0) == sh.placements(0) == sorted((i, ox, oy, s) for i, (ox, oy) in zip(ids, origins))
    assert np.array_equal(sh.compose([0], (0, 0), (W, H))[0], c)                # zero fields: the canvas's own bytes
    assert np.array_equal(sh.canvas_read(0), c)
    refused(lambda: mh.handle.session_render((L.SessionView * 1)(L.SessionView(9, 0, 0)), 8, 8, np.empty((1, 3, 8, 8), np.uint8)),
            "no full-resolution source", -7)                                    # placed: opened, without a source


def test_place_at_scale_16_off_alignment_needs_257_lanes():
    mh, sh, _, sp = pools(max_w=1100, max_h=1040)
    w, h, s = 1100, 1040, 16
    c = picture(w, h, 116)
    sh.canvas_put(0, c)
    ox, oy = 75, 15                                                           # ox % 4 = 3; the square ends at column 1099 and row 1039
    down = N.canvas_crop_mean(c, ox, oy, s)
    shown = sh.place([15], 0, (ox, oy), s)
    assert np.array_equal(shown[0], down) and np.array_equal(sh.read(15)["GIM"], down)
    sp.open([15], down[None])
    assert_fields(sh.read(15), sp.read(15), KEYS64)
    assert np.array_equal(sh.compose([0], (0, 0), (w, h))[0], c)
    shown, out = sh.brush_compose([15], (20, 20, 44, 44), (240, 30, 30), None, 0.5, -1.0, windows=([0], (0, 0), (w, h)))
    assert np.array_equal(shown, sp.paint([15], (20, 20, 44, 44), (240, 30, 30), weight=0.5))
    got = sh.read(15)
    assert got["FIELD"].any() and got["FIELD_KIND"] == 0
    want = N.canvas_compose(c, [(ox, oy, s, got["FIELD"], 0)], 4, 0, 0, w, h)
    assert np.array_equal(out[0], want) and (want != c).any()
    # the last band of a window whose height is no multiple of the band, at the canvas's bottom right corner
    assert np.array_equal(sh.compose([0], (w - 256, h - 13), (256, 13))[0], want[:, h - 13:, w - 256:])


# ---- 2. the brush script ---------------------------------------------------------------------------------------------------------
A, B, C_ = 3, 11, 6
SQUARES = {A: (5, 7, 2), B: (70, 40, 2), C_: (47, 9, 3)}                       # A and B overlap; C covers both and goes to sample mode


def place_three(sh, sp, c):
    ids = [A, B, C_]
    origins, scales = [SQUARES[i][:2] for i in ids], [SQUARES[i][2] for i in ids]
    sh.place(ids, 0, origins, scales)
    sp.open(ids, np.stack([N.canvas_crop_mean(c, *SQUARES[i]) for i in ids]))
    z = O.make_latents(1, seed=5)
    for p in (sh, sp):
        p.sample([C_], z)
    return ids


def brush_script(sh, sp, c, ids, check):
    """paint, paint, scroll, set_latent, mark, paint, undo on both pools; check(step, kind) after every step."""
    rs = np.random.RandomState(31)

    def args(n, kind):
        c1, r1 = rs.randint(0, 50, n), rs.randint(0, 50, n)
        boxes = np.stack([c1, r1, c1 + rs.randint(4, 14, n), r1 + rs.randint(4, 14, n)], 1)
        if kind == "paint":
            return boxes, rs.randint(0, 256, (n, 3)), None, 0.5, -1.0
        return boxes, None, None, 0.3, rs.choice([-1.0, 1.0], n)

    for step, kind in enumerate(["paint", "paint", "scroll", "set_latent", "mark", "paint", "undo"]):
        if kind in ("paint", "scroll"):
            a = args(len(ids), kind)
            shown, shown_p = sh.brush(ids, *a), sp.brush(ids, *a)
        elif kind == "set_latent":
            z = O.make_latents(len(ids), seed=40 + step)
            shown, shown_p = sh.set_latent(ids, z), sp.set_latent(ids, z)
        elif kind == "mark":
            sh.mark(ids)
            sp.mark(ids)
            shown = shown_p = None
        else:
            shown, shown_p = sh.undo(ids), sp.undo(ids)
        assert shown is None or np.array_equal(shown, shown_p), (step, kind)
        for i in ids:
            assert_fields(sh.read(i), sp.read(i), KEYS64, (step, kind, i))
        check(step, kind)


def test_brush_script_composes_and_leaves_the_64_state_unchanged():
    _, sh, _, sp = pools(depth=4)
    c = picture(W, H, 77)
    sh.canvas_put(0, c)
    ids = place_three(sh, sp, c)
    assert sh.read(C_)["FIELD_KIND"] == 1 and sh.read(A)["FIELD_KIND"] == 0
    squares = [(ox, oy, 64 * s) for (ox, oy, s) in SQUARES.values()]
    seen = []

    def check(step, kind):
        assert_composes(sh, c, squares, (step, kind))
        seen.append(sh.compose([0], (0, 0), (W, H))[0])

    assert_composes(sh, c, squares, "placed")
    brush_script(sh, sp, c, ids, check)
    assert any(sh.read(i)["FIELD"].any() and sh.read(i)["FIELD_KIND"] == 0 for i in (A, B))
    assert (seen[0] != c).any() and not np.array_equal(seen[0], seen[1]) and np.array_equal(seen[3], seen[4])   # a mark shows nothing new
    assert np.array_equal(sh.canvas_read(0), c)                               # the stored picture is untouched until a commit
    inside = np.zeros((H, W), bool)
    for (ox, oy, S) in squares:
        inside[oy:oy + S, ox:ox + S] = True
    assert np.array_equal(seen[-1][:, ~inside], c[:, ~inside])


# ---- 3. one submission -----------------------------------------------------------------------------------------------------------
def test_brush_compose_is_brush_then_compose():
    _, sh, _, _ = pools(count=2)
    c = picture(W, H, 13)
    sh.canvas_put(0, c)
    sh.canvas_put(1, c)
    X, Y = [1, 7], [2, 8]                                                     # ascending both: the squares overlap, and the order is by id
    origins, scales = [(5, 7), (70, 40)], [2, 2]
    sh.place(X, 0, origins, scales)
    sh.place(Y, 1, origins, scales)
    boxes, colours = np.array([(10, 12, 30, 28), (33, 5, 50, 20)]), np.array([(250, 20, 20), (10, 240, 90)])
    win0 = ([0, 0], [(0, 0), (132, 100)], (136, 103))
    win1 = ([1, 1], [(0, 0), (132, 100)], (136, 103))
    got = [sh.brush_compose(X, boxes, colours, None, 0.5, -1.0, windows=win0)]
    sh.compose([0], (0, 0), (W, H))                                           # a compose in between keeps the residency of the brush
    got.append(sh.brush_compose(X, boxes, colours, None, 0.5, -1.0, windows=win0))
    got.append(sh.brush_compose(X, boxes, None, None, 0.3, [1.0, -1.0], windows=win0))
    want = []
    for call in (lambda: sh.paint(Y, boxes, colours, weight=0.5), lambda: sh.paint(Y, boxes, colours, weight=0.5),
                 lambda: sh.scroll(Y, boxes, [1.0, -1.0], weight=0.3)):
        shown = call()
        want.append((shown, sh.compose(*win1)))
    for step, ((shown, out), (shown_w, out_w)) in enumerate(zip(got, want)):
        assert np.array_equal(shown, shown_w), step
        assert out.shape == (2, 3, 103, 136) and np.array_equal(out, out_w), step
    assert (got[0][1][0] != c[:, :103, :136]).any()                           # the window shows an edit
    for a, b in zip(X, Y):
        assert_fields(sh.read(a), sh.read(b), KEYS64 + ("FIELD", "FIELD_KIND"))
    # the events' sessions need not be placed, the windows need not show them
    sh.open([4], c[None, :, :64, :64].copy())
    shown, out = sh.brush_compose([4], boxes[0], colours[0], None, 0.5, -1.0, windows=([1], (0, 0), (W, H)))
    assert np.array_equal(out, sh.compose([1], (0, 0), (W, H))) and np.array_equal(shown[0], sh.read(4)["IM"])
    # device buffers: the same bytes
    import torch
    dev = torch.zeros((2, 3, 103, 136), dtype=torch.uint8, device="cuda")
    win, vw, vh = sh._windows(*win1)
    sh._h.canvas_compose(win, vw, vh, dev, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), sh.compose(*win1))


# ---- 4. commit -------------------------------------------------------------------------------------------------------------------
def test_canvas_commit_composes_in_place_and_places_again():
    _, sh, _, sp = pools()
    c = picture(W, H, 21)
    sh.canvas_put(0, c)
    ids = place_three(sh, sp, c)
    for p in (sh, sp):
        p.paint([A, B], [(18, 20, 44, 40), (5, 8, 30, 33)], [(250, 10, 10), (10, 250, 40)], weight=0.5)
    want = N.canvas_compose(c, placed_fields(sh, 0), 4, 0, 0, W, H)
    assert (want != c).any()
    before = sh.compose([0], (0, 0), (W, H))[0]
    assert np.array_equal(before, want)
    shown = sh.canvas_commit(0)
    assert np.array_equal(sh.canvas_read(0), want)
    order = sorted(ids)
    down = np.stack([N.canvas_crop_mean(want, *SQUARES[i]) for i in order])
    assert np.array_equal(shown, down)
    sp.open(order, down)                                                      # a fresh place on the new canvas: open of its box mean
    for i in order:
        got = sh.read(i)
        assert_fields(got, sp.read(i), KEYS64, ("commit", i))
        assert not got["FIELD"].any() and got["FIELD_KIND"] == 0
    assert sh.placements(0) == sorted((i,) + SQUARES[i] for i in ids)
    assert np.array_equal(sh.compose([0], (0, 0), (W, H))[0], want)           # a second compose returns the new canvas bytes
    # a session commit on a placed session is refused and names this call; Reset works as always
    refused(lambda: sh._h.session_open(np.asarray([A], np.int32), None, 1, None), "ian_canvas_commit", -7)
    sh.paint([A], (5, 5, 20, 20), (10, 10, 250), weight=0.5)
    sh.reset([A])
    assert not sh.read(A)["FIELD"].any() and sh.placements(0) == sorted((i,) + SQUARES[i] for i in ids)
    assert np.array_equal(sh.compose([0], (0, 0), (W, H))[0], want)


# ---- 5. feather ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 4])
def test_the_core_of_a_lone_placement_is_the_render_of_the_crop(f):
    _, sh, _, sp = pools(f=f)
    c = picture(W, H, 50)
    sh.canvas_put(0, c)
    for kind, (i, ox, oy, s) in enumerate([(4, 5, 7, 2), (4, 74, 10, 3)]):     # the second round in sample mode, at another square
        S, m = 64 * s, f * s
        sh.place([i], 0, (ox, oy), s)
        if kind:
            sh.sample([i], O.make_latents(1, seed=9))
        else:
            sh.paint([i], (10, 12, 40, 44), (250, 20, 20), weight=0.5)
        got = sh.read(i)
        assert got["FIELD_KIND"] == kind and got["FIELD"].any()
        whole = sh.compose([0], (0, 0), (W, H))[0]
        assert np.array_equal(whole, N.canvas_compose(c, [(ox, oy, s, got["FIELD"], kind)], f, 0, 0, W, H))
        crop = np.ascontiguousarray(c[:, oy:oy + S, ox:ox + S])
        want = N.hires_render(crop, got["FIELD"], kind, s, 0, 0, S, S)
        assert np.array_equal(whole[:, oy + m:oy + S - m, ox + m:ox + S - m], want[:, m:S - m, m:S - m])
        if f:
            assert not np.array_equal(whole[:, oy:oy + S, ox:ox + S], want)   # the rim is feathered
        outside = np.ones((H, W), bool)
        outside[oy:oy + S, ox:ox + S] = False
        assert np.array_equal(whole[:, outside], c[:, outside])
        assert_composes(sh, c, [(ox, oy, S)], (f, kind))


def test_the_brush_script_at_feather_0():
    _, sh, _, sp = pools(f=0, depth=4)
    c = picture(W, H, 78)
    sh.canvas_put(0, c)
    ids = place_three(sh, sp, c)
    squares = [(ox, oy, 64 * s) for (ox, oy, s) in SQUARES.values()]
    brush_script(sh, sp, c, ids, lambda step, kind: assert_composes(sh, c, squares[:1], (0, step, kind)))


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def placements_of(items):
    out = (L.CanvasPlacement * len(items))()
    for d, (sid, cv, x, y, s) in zip(out, items):
        d.session, d.canvas, d.x, d.y, d.scale = sid, cv, x, y, s
    return out


def windows_of(items):
    out = (L.CanvasWindow * len(items))()
    for d, (cv, x, y) in zip(out, items):
        d.canvas, d.x, d.y = cv, x, y
    return out


def test_refusals_return_their_code_and_change_nothing():
    mh, sh, mp, sp = pools(count=3)
    h = mh.handle
    sh.reserve(1)                                                             # ids 1.. come back unopened
    sh.reserve(CAP)
    c = picture(W, H, 55)
    sh.canvas_put(0, c)
    sh.canvas_put(1, c[:, :64, :64].copy())
    ids = [0, 1, 2]
    sh.place(ids, 0, [(5, 7), (70, 40), (140, 75)], [2, 2, 1])
    sh.paint(ids, (10, 10, 30, 30), (200, 100, 50), weight=0.5)
    sh.place(list(range(3, 11)), 1, (0, 0), 1)                                # canvas 1 is full
    before = [sh.read(i) for i in ids]
    table = sh.placements(0)
    out = np.full((2, 3, 16, 16), 7, np.uint8)
    shown = np.full((2, 3, 64, 64), 7, np.uint8)
    P, Wn = placements_of, windows_of
    ok = [(0, 0, 0), (0, 16, 16)]
    bad = [
        ("n = 0", lambda: h.canvas_place(P([]), shown)),                                              # n outside 1..256
        ("n = 257", lambda: h.canvas_place(P([(0, 0, 0, 0, 1)] * 257), shown)),
        ("item 1", lambda: h.canvas_place(P([(0, 0, 0, 0, 1), (CAP, 0, 0, 0, 1)]), shown)),           # an id outside the pool
        ("item 1", lambda: h.canvas_place(P([(0, 0, 0, 0, 1), (-1, 0, 0, 0, 1)]), shown)),
        ("item 1", lambda: h.canvas_place(P([(0, 0, 0, 0, 1), (1, 3, 0, 0, 1)]), shown)),             # a canvas outside its range
        ("item 0", lambda: h.canvas_place(P([(0, -1, 0, 0, 1), (1, 0, 0, 0, 1)]), shown)),
        ("item 1: canvas 2 holds no picture", lambda: h.canvas_place(P([(0, 0, 0, 0, 1), (1, 2, 0, 0, 1)]), shown)),   # never put
        ("item 1", lambda: h.canvas_place(P([(0, 0, 0, 0, 1), (1, 0, W - 63, 0, 1)]), shown)),        # a square outside the canvas
        ("item 1", lambda: h.canvas_place(P([(0, 0, 0, 0, 1), (1, 0, 0, H - 127, 2)]), shown)),
        ("item 0", lambda: h.canvas_place(P([(0, 0, -1, 0, 1), (1, 0, 0, 0, 1)]), shown)),
        ("item 0", lambda: h.canvas_place(P([(0, 0, 0, -1, 1), (1, 0, 0, 0, 1)]), shown)),
        ("item 1", lambda: h.canvas_place(P([(0, 0, 0, 0, 1), (1, 0, 0, 0, 0)]), shown)),             # scale outside 1..16
        ("item 1", lambda: h.canvas_place(P([(0, 0, 0, 0, 1), (1, 0, 0, 0, 17)]), shown)),
        ("item 1", lambda: h.canvas_place(P([(0, 0, 0, 0, 1), (0, 0, 4, 4, 1)]), shown)),             # an id given twice
        ("item 1: canvas 1 already holds 8", lambda: h.canvas_place(P([(0, 0, 0, 0, 1), (1, 1, 0, 0, 1)]), shown)),   # a ninth session
        ("0 windows", lambda: h.canvas_compose(Wn([]), 16, 16, out)),
        ("257 windows", lambda: h.canvas_compose(Wn([(0, 0, 0)] * 257), 16, 16, out)),
        ("item 1", lambda: h.canvas_compose(Wn([(0, 0, 0), (3, 0, 0)]), 16, 16, out)),                # a canvas outside its range
        ("item 1", lambda: h.canvas_compose(Wn([(0, 0, 0), (2, 0, 0)]), 16, 16, out)),                # ... never put
        ("at least 1", lambda: h.canvas_compose(Wn(ok), 0, 16, out)),
        ("at least 1", lambda: h.canvas_compose(Wn(ok), 16, 0, out)),
        ("item 1", lambda: h.canvas_compose(Wn([(0, 0, 0), (0, W - 12, 0)]), 16, 16, out)),           # a window not inside w x hgt
        ("item 1", lambda: h.canvas_compose(Wn([(0, 0, 0), (0, 0, H - 15)]), 16, 16, out)),
        ("item 1", lambda: h.canvas_compose(Wn([(0, 0, 0), (1, 52, 0)]), 16, 16, out)),               # ... of ITS canvas (64 x 64)
        ("item 0", lambda: h.canvas_compose(Wn([(0, -4, 0), (0, 0, 0)]), 16, 16, out)),
        ("item 0", lambda: h.canvas_compose(Wn([(0, 0, -1), (0, 0, 0)]), 16, 16, out)),
        ("item 1", lambda: h.canvas_compose(Wn([(0, 0, 0), (0, 2, 0)]), 16, 16, out)),                # x not a multiple of 4
        ("multiple of 4", lambda: h.canvas_compose(Wn(ok), 18, 16, out)),                             # vw not a multiple of 4
        ("item 1", lambda: h.canvas_brush(events([0, 1]), Wn([(0, 0, 0), (0, 2, 0)]), 16, 16, out, shown)),    # the windows' checks
        ("item 1", lambda: h.canvas_brush(events([0, 0]), Wn(ok), 16, 16, out, shown)),                        # the events' checks
        ("item 1", lambda: h.canvas_brush(events([0, 12]), Wn(ok), 16, 16, out, shown)),                       # a session not opened
        ("ian_canvas_commit", lambda: h.session_open(np.asarray([1], np.int32), None, 1, shown)),               # commit of a placed session
        ("canvas 3", lambda: h.canvas_commit(3, shown)),
        ("holds no picture", lambda: h.canvas_commit(2, shown)),
        ("holds no picture", lambda: h.canvas_read(2)),
        ("canvas -1", lambda: h.canvas_placements(-1)),
        ("multiple of 4", lambda: h.canvas_put(2, np.zeros((3, 64, 66), np.uint8))),
        ("outside", lambda: h.canvas_put(2, np.zeros((3, 64, MAXW + 4), np.uint8))),
        ("outside", lambda: h.canvas_put(2, np.zeros((3, MAXH + 1, 64), np.uint8))),
        ("outside", lambda: h.canvas_put(2, np.zeros((3, 60, 64), np.uint8))),
        ("canvas 3", lambda: h.canvas_put(3, np.zeros((3, 64, 64), np.uint8))),
        ("count 65", lambda: h.sessions_reserve_canvas(65, 64, 64, 0)),
        ("multiple of 4", lambda: h.sessions_reserve_canvas(1, 66, 64, 0)),
        ("must be in", lambda: h.sessions_reserve_canvas(1, 64, 8196, 0)),
        ("feather 17", lambda: h.sessions_reserve_canvas(1, 64, 64, 17)),
    ]
    for needle, call in bad:
        refused(call, needle, -7)
        assert np.all(out == 7) and np.all(shown == 7), needle
        for i, b in zip(ids, before):
            assert_fields(sh.read(i), b, KEYS64 + ("FIELD", "FIELD_KIND"), (needle, i))
        assert h.canvas_placements(0) == table and len(h.canvas_placements(1)) == 8, needle
        assert np.array_equal(sh.canvas_read(0), c), needle
    # -6: the one new refusal of an existing call, and it frees nothing
    refused(lambda: h.sessions_reserve_hires(0), "canvases are reserved", -6)
    assert sh.read(0)["FIELD"].any() and h.canvas_placements(0) == table
    # -6: a pool without the reservations
    hp = mp.handle
    sp.open([0, 1], c[None, :, :64, :64].repeat(2, 0))
    z0 = sp.read(0)["Z"]
    refused(lambda: hp.sessions_reserve_canvas(1, 64, 64, 0), "no full-resolution reservation", -6)
    no_res = [
        lambda: hp.canvas_put(0, c), lambda: hp.canvas_place(P([(0, 0, 0, 0, 1)]), shown), lambda: hp.canvas_compose(Wn(ok), 16, 16, out),
        lambda: hp.canvas_brush(events([0, 1]), Wn(ok), 16, 16, out, shown), lambda: hp.canvas_commit(0, shown), lambda: hp.canvas_read(0),
        lambda: hp.canvas_placements(0),
    ]
    for call in no_res:
        refused(call, "no canvas reservation", -6)
    assert np.all(out == 7) and np.all(shown == 7) and np.array_equal(sp.read(0)["Z"], z0)
    # the Python surface refuses the same before the library is called, and the handle still works
    with pytest.raises(ValueError):
        sh.compose([0, 2], (0, 0), 16)
    got = sh.compose([0, 0], [(0, 0), (16, 16)], 16)
    assert got.shape == (2, 3, 16, 16) and np.array_equal(got[0], N.canvas_compose(c, placed_fields(sh, 0), 4, 0, 0, 16, 16))


# ---- 7. upkeep -------------------------------------------------------------------------------------------------------------------
def test_put_open_load_and_the_pool_size_drop_placements():
    mh, sh, _, _ = pools(count=2)
    h = mh.handle
    c = picture(W, H, 61)
    sh.canvas_put(0, c)
    sh.canvas_put(1, c)
    sh.place([1, 6, 12, 13], [0, 0, 0, 1], [(5, 7), (70, 40), (140, 75), (9, 9)], [2, 2, 1, 1])
    sh.paint([1, 6, 12], (10, 10, 40, 40), (250, 20, 20), weight=0.5)
    f1 = sh.read(1)["FIELD"]
    rec = sh.save([6])
    try:
        sh.reserve(8)                                                         # 12 and 13 leave the pool
        assert h.canvas_placements(0) == sh.placements(0) == [(1, 5, 7, 2), (6, 70, 40, 2)] and h.canvas_placements(1) == []
    finally:
        sh.reserve(CAP)
    assert h.canvas_placements(0) == [(1, 5, 7, 2), (6, 70, 40, 2)]
    sh.load([6], rec)                                                         # a load un-places; so does an open with a photo
    assert h.canvas_placements(0) == sh.placements(0) == [(1, 5, 7, 2)]
    whole = sh.compose([0], (0, 0), (W, H))[0]
    assert np.array_equal(whole, N.canvas_compose(c, [(5, 7, 2, f1, 0)], 4, 0, 0, W, H)) and (whole != c).any()
    sh.place([6], 0, (70, 40), 2)
    sh.place([6], 1, (3, 3), 3)                                               # a move to another canvas
    assert h.canvas_placements(0) == [(1, 5, 7, 2)] and h.canvas_placements(1) == sh.placements(1) == [(6, 3, 3, 3)]
    sh.open([1], c[None, :, :64, :64].copy())
    assert h.canvas_placements(0) == sh.placements(0) == []
    assert np.array_equal(sh.compose([0], (0, 0), (W, H))[0], c)
    sh.canvas_put(1, c[:, :100, :128].copy())                                 # a put drops the canvas's placements, not the sessions
    assert h.canvas_placements(1) == sh.placements(1) == [] and sh.read(6)["MODE"] == 0
    assert sh.canvas_read(1).shape == (3, 100, 128) and np.array_equal(sh.canvas_read(1), c[:, :100, :128])
    refused(lambda: h.canvas_compose(windows_of([(1, 0, 0)]), 132, 8, np.empty((1, 3, 8, 132), np.uint8)), "outside the 128 x 100 canvas", -7)
    # a device photo, and the whole pool freed with its canvases
    import torch
    sh.canvas_put(1, torch.from_numpy(c).cuda())
    assert np.array_equal(sh.canvas_read(1), c)
    try:
        h.sessions_reserve(0)
        refused(lambda: h.canvas_read(1), "no session pool", -6)
    finally:
        _cache["p"] = (mh, mh.sessions(CAP)) + _cache["p"][2:]

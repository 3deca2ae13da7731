"""CPU tests of the canvases' host side (ian_sessions_reserve_canvas, ian_canvas_*): the numpy functions that specify the arithmetic
(npe_ops.canvas_crop_mean, canvas_ramp, canvas_compose), the two structs' layout against the header, the header / export list
agreement, the packers (every validation before any library call) and what EditSessions tracks about canvases and placements."""
import ctypes
import re
import shutil

import numpy as np
import pytest

from neural_photo_editor_amd import api
from neural_photo_editor_amd import lib as L
from neural_photo_editor_amd import npe_ops as N
from session_helpers import HEADER, StubHandle, header_code, run_c

NEW_EXPORTS = ("ian_sessions_reserve_canvas", "ian_canvas_put", "ian_canvas_place", "ian_canvas_compose", "ian_canvas_brush",
               "ian_canvas_commit", "ian_canvas_read", "ian_canvas_placements")
W, H = 268, 203


def canvas(seed=0, w=W, h=H):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127.5 + 100.0 * np.sin(xx / 9.0 + rs.uniform(0, 6, (3, 1, 1))) * np.cos(yy / 11.0 + rs.uniform(0, 6, (3, 1, 1)))
    return np.uint8(np.clip(base + rs.randint(-40, 41, (3, h, w)), 0, 255))


def field(seed, kind):
    rs = np.random.RandomState(seed)
    return np.float32(rs.uniform(-1, 1, (3, 64, 64)) * (1.0 if kind else 0.6))


def squares(c, out):
    """True where a pixel lies in some square of `placed`."""
    m = np.zeros(c.shape[1:], bool)
    for (ox, oy, s, _, _) in out:
        m[oy:oy + 64 * s, ox:ox + 64 * s] = True
    return m


# placements of scales 1..3 at offsets with ox % 4 = 1, 2, 3, 0; the first two overlap, the third is a sample (kind 1) over both
PLACED = [(5, 7, 2, field(1, 0), 0), (70, 40, 2, field(2, 0), 0), (47, 9, 3, field(3, 1), 1), (200, 139, 1, field(4, 0), 0)]


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 4])
def test_zero_fields_return_the_canvas_and_nothing_outside_the_squares_changes(f):
    c = canvas()
    zero = [(ox, oy, s, np.zeros((3, 64, 64), np.float32), 0) for (ox, oy, s, _, _) in PLACED]
    assert np.array_equal(N.canvas_compose(c, zero, f, 0, 0, W, H), c)
    assert np.array_equal(N.canvas_compose(c, [(ox, oy, s, -F, 0) for (ox, oy, s, F, _) in zero], f, 0, 0, W, H), c)   # fields of -0.0
    assert np.array_equal(N.canvas_compose(c, [], f, 0, 0, W, H), c)
    out = N.canvas_compose(c, PLACED, f, 0, 0, W, H)
    assert out.dtype == np.uint8 and out.shape == c.shape
    inside = squares(c, PLACED)
    assert np.array_equal(out[:, ~inside], c[:, ~inside]) and (out[:, inside] != c[:, inside]).any()


@pytest.mark.parametrize("f", [0, 4])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("s,ox,oy", [(1, 4, 0), (2, 5, 70), (3, 74, 11), (3, 3, 2), (2, 140, 75)])
def test_the_core_of_a_lone_placement_is_the_render_of_the_crop(f, kind, s, ox, oy):
    c = canvas(s)
    S = 64 * s
    F = field(10 * s + kind, kind)
    out = N.canvas_compose(c, [(ox, oy, s, F, kind)], f, 0, 0, W, H)
    crop = np.ascontiguousarray(c[:, oy:oy + S, ox:ox + S])
    want = N.hires_render(crop, F, kind, s, 0, 0, S, S)
    m = f * s
    assert np.array_equal(out[:, oy + m:oy + S - m, ox + m:ox + S - m], want[:, m:S - m, m:S - m])
    if f == 0:
        return
    rim = np.ones((S, S), bool)
    rim[m:S - m, m:S - m] = False
    assert (out[:, oy:oy + S, ox:ox + S][:, rim] != want[:, rim]).any()       # the rim is feathered


@pytest.mark.parametrize("f", [0, 4, 16])
def test_a_window_is_the_crop_of_the_whole_compose(f):
    c = canvas(7)
    whole = N.canvas_compose(c, PLACED, f, 0, 0, W, H)
    rs = np.random.RandomState(f)
    wins = [(0, 0, 4, 1), (W - 4, H - 1, 4, 1), (40, 3, 64, 13), (0, 100, W, 8), (132, 0, 136, H), (264, 0, 4, H)]
    for _ in range(12):
        vw, vh = 4 * rs.randint(1, W // 4 + 1), rs.randint(1, H + 1)
        wins.append((4 * rs.randint(0, (W - vw) // 4 + 1), rs.randint(0, H - vh + 1), vw, vh))
    for (vx, vy, vw, vh) in wins:
        assert np.array_equal(N.canvas_compose(c, PLACED, f, vx, vy, vw, vh), whole[:, vy:vy + vh, vx:vx + vw]), (vx, vy, vw, vh)


def test_list_order_matters_only_where_squares_overlap():
    c = canvas(8)
    a = N.canvas_compose(c, PLACED, 4, 0, 0, W, H)
    b = N.canvas_compose(c, PLACED[::-1], 4, 0, 0, W, H)
    count = np.zeros((H, W), int)
    for p in PLACED:
        count += squares(c, [p])
    assert np.array_equal(a[:, count < 2], b[:, count < 2]) and (a[:, count >= 2] != b[:, count >= 2]).any()


def test_compose_by_hand_at_scale_1():
    """s = 1: every tap has t = 0.5 - 0.5 = 0 .. the sample is the field itself; one pixel worked out with Python floats."""
    c = canvas(9, 64, 64)
    F = field(5, 0)
    out = N.canvas_compose(c, [(0, 0, 1, F, 0)], 4, 0, 0, 64, 64)
    for (y, x) in [(0, 0), (1, 2), (3, 40), (30, 31), (63, 5)]:
        ry = min(np.float32(1.0), np.float32(2 * min(y, 63 - y) + 1) / np.float32(8))
        rx = min(np.float32(1.0), np.float32(2 * min(x, 63 - x) + 1) / np.float32(8))
        for ch in range(3):
            acc = np.float32(c[ch, y, x]) + (np.float32(127.5) * F[ch, y, x]) * np.float32(ry * rx)
            assert out[ch, y, x] == np.uint8(np.clip(np.rint(acc), 0, 255))
    t = N.canvas_compose(c, [(0, 0, 1, F, 1)], 0, 0, 0, 64, 64)
    assert np.array_equal(t, np.uint8(np.clip(np.rint(np.float32(127.5) * (F + np.float32(1.0))), 0, 255)))


@pytest.mark.parametrize("s", [1, 2, 3, 16])
@pytest.mark.parametrize("f", [0, 1, 4, 16])
def test_ramp_is_float32_monotone_to_the_middle_symmetric_and_one_in_the_core(s, f):
    S = 64 * s
    r = N.canvas_ramp(s, f, 0, S)
    assert r.dtype == np.float32 and r.shape == (S,)
    if f == 0:
        assert np.all(r == 1.0)
        return
    assert np.all(np.diff(r[:S // 2]) >= 0) and np.array_equal(r, r[::-1])
    assert np.all(r[f * s:S - f * s] == 1.0) and np.all(r[:f * s] < 1.0) and np.all(r > 0)
    assert r[0] == np.float32(1.0) / np.float32(2 * f * s)
    assert np.array_equal(N.canvas_ramp(s, f, 5, 40), r[5:45])
    for bad in (lambda: N.canvas_ramp(s, 17, 0, 4), lambda: N.canvas_ramp(s, -1, 0, 4), lambda: N.canvas_ramp(s, f, S - 2, 4),
                lambda: N.canvas_ramp(17, f, 0, 4)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("s", [1, 2, 3])
def test_crop_mean_at_every_alignment(s):
    c = canvas(20 + s)
    S = 64 * s
    for ox in (0, 1, 2, 3, W - S):
        for oy in (0, 5, H - S):
            got = N.canvas_crop_mean(c, ox, oy, s)
            blk = c[:, oy:oy + S, ox:ox + S].astype(np.int64).reshape(3, 64, s, 64, s).sum(axis=(2, 4))
            assert got.dtype == np.uint8 and np.array_equal(got, (blk + (s * s) // 2) // (s * s)), (ox, oy)
    for bad in (lambda: N.canvas_crop_mean(c, W - S + 1, 0, s), lambda: N.canvas_crop_mean(c, 0, -1, s), lambda: N.canvas_crop_mean(c, 0.5, 0, s),
                lambda: N.canvas_crop_mean(c.astype(np.float32), 0, 0, s), lambda: N.canvas_crop_mean(c, 0, 0, 17)):
        with pytest.raises(ValueError):
            bad()


def test_compose_refuses_what_is_no_window_or_placement():
    c = canvas()
    for bad in (lambda: N.canvas_compose(c, PLACED, 4, 0, 0, W + 4, 8), lambda: N.canvas_compose(c, PLACED, 4, -4, 0, 8, 8),
                lambda: N.canvas_compose(c, PLACED, 4, 0, H, 8, 1), lambda: N.canvas_compose(c, PLACED, 17, 0, 0, 8, 8),
                lambda: N.canvas_compose(c, [(0, 0, 1, field(0, 0), 2)], 4, 0, 0, 8, 8),
                lambda: N.canvas_compose(c, [(W - 60, 0, 1, field(0, 0), 0)], 4, 0, 0, 8, 8),
                lambda: N.canvas_compose(c, [PLACED[0]] * 9, 4, 0, 0, 8, 8)):
        with pytest.raises(ValueError):
            bad()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(tmp_path):
    assert ctypes.sizeof(L.CanvasPlacement) == 20 and ctypes.sizeof(L.CanvasWindow) == 12
    assert [(f, getattr(L.CanvasPlacement, f).offset) for f, _ in L.CanvasPlacement._fields_] == \
        [("session", 0), ("canvas", 4), ("x", 8), ("y", 12), ("scale", 16)]
    assert [(f, getattr(L.CanvasWindow, f).offset) for f, _ in L.CanvasWindow._fields_] == [("canvas", 0), ("x", 4), ("y", 8)]
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    P, Wn = "ian_canvas_placement", "ian_canvas_window"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ian.h"', 'int main(void) {',
             '  printf("%%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(%s), offsetof(%s, session), offsetof(%s, canvas), offsetof(%s, x), '
             'offsetof(%s, y), offsetof(%s, scale));' % (P, P, P, P, P, P),
             '  printf("%%zu %%zu %%zu %%zu\\n", sizeof(%s), offsetof(%s, canvas), offsetof(%s, x), offsetof(%s, y));' % (Wn, Wn, Wn, Wn),
             '  printf("%d\\n", IAN_CANVAS_MAX_PLACED);', '  return 0;', '}']
    out = run_c(tmp_path, lines)
    assert out[0].split() == ["20", "0", "4", "8", "12", "16"]
    assert out[1].split() == ["12", "0", "4", "8"]
    assert int(out[2]) == L.CANVAS_MAX_PLACED == N.CANVAS_MAX_PLACED == 8


def test_header_and_export_list_declare_exactly_the_eight_canvas_names():
    declared = set(re.findall(r"\b(ian_[a-z_0-9]+)\s*\(", header_code()))
    assert {n for n in declared if "canvas" in n} == set(NEW_EXPORTS)
    assert {n for n in L.EXPORTS if "canvas" in n} == set(NEW_EXPORTS)
    for n in NEW_EXPORTS:       # the patterns the other session tests hold their own names to
        assert not ("hires" in n or "render" in n or "view" in n or n.endswith("_local")), n
    lib = L.load_library()
    protos = {name: argt for _, name, argt in L.parse_header_prototypes(HEADER)}
    for name in NEW_EXPORTS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == len(protos[name]), name


# ---- the packers and the class ----------------------------------------------------------------------------------------------------
def canvas_stub(count=2, put=((0, W, H), (1, 1100, 1040)), args=False):
    """EditSessions over a StubHandle with the full-resolution and the canvas reservation; sessions 0..3 opened."""
    h = StubHandle(args)
    s = api.EditSessions(h, 8, 100)
    s.reserve_hires(2)
    s._opened = {0, 1, 2, 3}
    if count:
        s.reserve_canvases(count, 1104, 1040, 4)
        for cid, w, hh in put:
            s.canvas_put(cid, np.zeros((3, hh, w), np.uint8))
    h.calls.clear()
    return s, h


def test_packers_broadcast_and_fill_the_structs():
    sizes = [(W, H), None, (1100, 1040)]
    items = api.pack_canvas_placements([3, 1], 0, [(5, 7), (140, 75)], [2, 1], sizes)
    assert [(p.session, p.canvas, p.x, p.y, p.scale) for p in items] == [(3, 0, 5, 7, 2), (1, 0, 140, 75, 1)]
    items = api.pack_canvas_placements([2], [2], (75, 15), 16, sizes)
    assert [(p.session, p.canvas, p.x, p.y, p.scale) for p in items] == [(2, 2, 75, 15, 16)]
    win, vw, vh = api.pack_canvas_windows([0, 0, 2], [(0, 0), (132, 5), (4, 1039)], (136, 1), sizes)
    assert (vw, vh) == (136, 1) and [(w.canvas, w.x, w.y) for w in win] == [(0, 0, 0), (0, 132, 5), (2, 4, 1039)]
    win, vw, vh = api.pack_canvas_windows(0, (8, 5), 64, sizes)
    assert (vw, vh) == (64, 64) and [(w.canvas, w.x, w.y) for w in win] == [(0, 8, 5)]
    # eight sessions fit on one canvas, a move does not count twice, the ninth is refused
    on0 = {i: 0 for i in range(8)}
    api.pack_canvas_placements([3], 0, (0, 0), 1, sizes, placed=on0)
    api.pack_canvas_placements([9], 2, (0, 0), 1, sizes, placed=on0)
    with pytest.raises(ValueError, match="item 0: canvas 0"):
        api.pack_canvas_placements([9], 0, (0, 0), 1, sizes, placed=on0)
    with pytest.raises(ValueError, match="item 1: canvas 1 holds no picture"):
        api.pack_canvas_placements([0, 1], [0, 1], (0, 0), 1, sizes)


BOX, COL = (0, 0, 4, 4), (1, 2, 3)
WIN = ([0], (0, 0), 64)


@pytest.mark.parametrize("call", [
    lambda s: s.place([0, 8], 0, (0, 0), 1),                                  # an id outside the pool
    lambda s: s.place([-1], 0, (0, 0), 1),
    lambda s: s.place([], 0, np.zeros((0, 2), int), 1),                        # n outside 1..256
    lambda s: s.place(list(range(257)), 0, (0, 0), 1),
    lambda s: s.place([0, 1, 0], 0, (0, 0), 1),                               # an id given twice
    lambda s: s.place([0], 2, (0, 0), 1),                                     # a canvas outside its range
    lambda s: s.place([0], -1, (0, 0), 1),
    lambda s: s.place([0, 1], [0], (0, 0), 1),                                # one canvas per item
    lambda s: s.place([0], 0.0, (0, 0), 1),                                   # canvas ids are integers
    lambda s: s.place([0], 0, (W - 63, 0), 1),                                # a square outside the canvas
    lambda s: s.place([0], 0, (0, H - 127), 2),
    lambda s: s.place([0], 0, (-1, 0), 1),
    lambda s: s.place([0], 0, (0, -1), 1),
    lambda s: s.place([0], 0, (0, 0), 4),
    lambda s: s.place([0], 0, (0.0, 0.0), 1),                                 # coordinates are integers
    lambda s: s.place([0, 1], 0, [(0, 0)], 1),                                # one origin per item
    lambda s: s.place([0], 0, (0, 0), 0),                                     # scale outside 1..16
    lambda s: s.place([0], 1, (0, 0), 17),
    lambda s: s.place([0], 0, (0, 0), 1.0),
    lambda s: s.place([0, 1], 0, (0, 0), [1]),
    lambda s: s.compose([2], (0, 0), 64),                                     # a canvas outside its range
    lambda s: s.compose([], np.zeros((0, 2), int), 64),                        # n outside 1..256
    lambda s: s.compose([0] * 257, (0, 0), 64),
    lambda s: s.compose([0], (0, 0), (0, 8)),                                 # vw < 1
    lambda s: s.compose([0], (0, 0), (8, 0)),                                 # vh < 1
    lambda s: s.compose([0], (0, 0), (-4, 8)),
    lambda s: s.compose([0], (0, 0), (W + 4, 8)),                             # a window not inside w x h
    lambda s: s.compose([0], (208, 0), (64, 8)),
    lambda s: s.compose([0], (0, H - 63), (64, 64)),
    lambda s: s.compose([0], (-4, 0), (64, 64)),
    lambda s: s.compose([0], (0, -1), (64, 64)),
    lambda s: s.compose([0], (2, 0), (64, 64)),                               # x not a multiple of 4
    lambda s: s.compose([0], (0, 0), (66, 64)),                               # vw not a multiple of 4
    lambda s: s.compose([0], (0.0, 0.0), (64, 64)),
    lambda s: s.compose([0, 1], [(0, 0)], 64),
    lambda s: s.brush_compose([0], BOX, COL, windows=([0], (2, 0), 64)),      # brush_compose: the windows' checks
    lambda s: s.brush_compose([0], BOX, COL, windows=([2], (0, 0), 64)),
    lambda s: s.brush_compose([0], BOX, COL),                                 # ... windows are required
    lambda s: s.brush_compose([4], BOX, COL, windows=WIN),                    # ... the events' own checks: a session not opened
    lambda s: s.brush_compose([0, 0], BOX, COL, windows=WIN),
    lambda s: s.brush_compose([0], (0, 0, 65, 4), COL, windows=WIN),
    lambda s: s.canvas_put(2, np.zeros((3, 64, 64), np.uint8)),               # put: a canvas outside its range
    lambda s: s.canvas_put(0, np.zeros((3, 64, 66), np.uint8)),               # a width that is no multiple of 4
    lambda s: s.canvas_put(0, np.zeros((3, 60, 64), np.uint8)),               # smaller than 64
    lambda s: s.canvas_put(0, np.zeros((3, 64, 1108), np.uint8)),             # larger than the reservation
    lambda s: s.canvas_put(0, np.zeros((3, 1044, 64), np.uint8)),
    lambda s: s.canvas_put(0, np.zeros((3, 64, 64), np.float32)),             # photos are uint8
    lambda s: s.canvas_put(0, np.zeros((64, 64, 3), np.uint8)),
    lambda s: s.canvas_commit(2),
    lambda s: s.canvas_read(-1),
    lambda s: s.placements(2),
    lambda s: s.reserve_canvases(65, 64, 64),                                 # the reservation's own ranges
    lambda s: s.reserve_canvases(-1, 64, 64),
    lambda s: s.reserve_canvases(1, 60, 64),
    lambda s: s.reserve_canvases(1, 64, 8196),
    lambda s: s.reserve_canvases(1, 66, 64),
    lambda s: s.reserve_canvases(1, 64, 64, feather=17),
    lambda s: s.reserve_canvases(1, 64, 64, feather=-1),
    lambda s: s.reserve_hires(0),                                             # the one new refusal of an existing call
])
def test_invalid_input_raises_before_any_library_call(call):
    s, h = canvas_stub()
    with pytest.raises(ValueError):
        call(s)
    assert h.calls == []


def test_a_canvas_never_put_and_a_ninth_session_are_refused_before_any_library_call():
    s, h = canvas_stub(count=2, put=((0, W, H),))
    for call in (lambda: s.place([0], 1, (0, 0), 1), lambda: s.compose([1], (0, 0), 64), lambda: s.canvas_commit(1), lambda: s.canvas_read(1),
                 lambda: s.brush_compose([0], BOX, COL, windows=([0, 1], (0, 0), 64))):
        with pytest.raises(ValueError, match="holds no picture"):
            call()
    assert h.calls == []
    s.reserve(16)
    s.place(list(range(8)), 0, (0, 0), 1)
    h.calls.clear()
    with pytest.raises(ValueError, match="canvas 0"):
        s.place([8], 0, (0, 0), 1)
    with pytest.raises(ValueError, match="item 1"):
        s.place([3, 9], 0, (4, 4), 1)
    assert h.calls == []
    s.place([3], 0, (4, 4), 2)                                                # one of the eight moves
    assert h.calls == ["canvas_place"] and (3, 4, 4, 2) in s.placements(0)


def test_without_the_reservations_every_canvas_call_is_refused():
    s, h = canvas_stub(count=0)
    for call in (lambda: s.place([0], 0, (0, 0), 1), lambda: s.compose([0], (0, 0), 64), lambda: s.canvas_commit(0), lambda: s.canvas_read(0),
                 lambda: s.placements(0), lambda: s.canvas_put(0, np.zeros((3, 64, 64), np.uint8)),
                 lambda: s.brush_compose([0], BOX, COL, windows=WIN)):
        with pytest.raises(ValueError, match="no canvas reservation"):
            call()
    s.reserve_hires(0)
    h.calls.clear()
    with pytest.raises(ValueError, match="no full-resolution reservation"):
        s.reserve_canvases(1, 64, 64)
    assert h.calls == []


def test_valid_calls_reach_the_library_in_order_and_track_placements():
    s, h = canvas_stub(args=True)
    shown = s.place([2, 0, 5], [0, 0, 1], [(5, 7), (140, 75), (75, 15)], [2, 1, 16])
    assert shown.shape == (3, 3, 64, 64)
    s.compose([0, 0, 1], [(0, 0), (132, 5), (4, 1027)], (136, 13))
    s.brush_compose([0, 3], BOX, COL, windows=([1], (0, 0), (1100, 1040)))
    assert s.canvas_commit(0).shape == (2, 3, 64, 64)
    s.canvas_read(1)
    assert [c[0] for c in h.calls] == ["canvas_place", "canvas_compose", "canvas_brush", "canvas_commit", "canvas_read"]
    items = h.calls[0][1][0]
    assert [(p.session, p.canvas, p.x, p.y, p.scale) for p in items] == [(2, 0, 5, 7, 2), (0, 0, 140, 75, 1), (5, 1, 75, 15, 16)]
    win, vw, vh = h.calls[1][1][:3]
    assert (vw, vh) == (136, 13) and [(w.canvas, w.x, w.y) for w in win] == [(0, 0, 0), (0, 132, 5), (1, 4, 1027)]
    ev, win, vw, vh, out, shown = h.calls[2][1]
    assert [e.session for e in ev] == [0, 3] and len(win) == 1 and out.shape == (1, 3, 1040, 1100) and shown.shape == (2, 3, 64, 64)
    assert s.placements(0) == [(0, 140, 75, 1), (2, 5, 7, 2)] and s.placements(1) == [(5, 75, 15, 16)]
    assert 5 in s._opened and 5 not in s._sourced                             # placed: opened, without a source
    with pytest.raises(ValueError, match="session 5 has no full-resolution source"):
        s.render([5], (0, 0), 64)
    # commit on a placed session is refused and names canvas_commit; reset works as always
    h.calls.clear()
    with pytest.raises(ValueError, match="item 1: session 2 is placed on canvas 0.*canvas_commit"):
        s.commit([3, 2])
    assert h.calls == []
    s.reset([2])
    s.commit([3])
    assert [c[0] for c in h.calls] == ["session_open", "session_open"] and s.placements(0) == [(0, 140, 75, 1), (2, 5, 7, 2)]
    # a session already placed moves, to another canvas too
    s.place([2], 1, (0, 0), 3)
    assert s.placements(0) == [(0, 140, 75, 1)] and s.placements(1) == [(2, 0, 0, 3), (5, 75, 15, 16)]
    # open, open_hires and load un-place
    s.open([2], np.zeros((1, 3, 64, 64), np.uint8))
    assert s.placements(1) == [(5, 75, 15, 16)]
    s.open_hires([5], np.zeros((1, 3, 128, 128), np.uint8))
    assert s.placements(1) == [] and 5 in s._sourced
    s.place([1], 0, (0, 0), 1)
    s.load([1], _record(s))
    assert s.placements(0) == [(0, 140, 75, 1)]
    # put drops the canvas's placements and keeps the others; the sessions stay opened
    s.place([1, 6], [0, 1], (0, 0), 1)
    s.canvas_put(0, np.zeros((3, 64, 64), np.uint8))
    assert s.placements(0) == [] and s.placements(1) == [(6, 0, 0, 1)] and {0, 1} <= s._opened
    with pytest.raises(ValueError, match="outside the 64 x 64 canvas"):
        s.place([0], 0, (4, 0), 1)
    # shrinking the pool drops the ids that left it
    s.place([7], 1, (8, 8), 2)
    s.reserve(7)
    assert s.placements(1) == [(6, 0, 0, 1)]
    # a new reservation starts from nothing; freeing it gives the old refusals back
    s.reserve_canvases(1, 64, 64, 0)
    assert s.placements(0) == [] and s.feather == 0
    with pytest.raises(ValueError, match="holds no picture"):
        s.compose([0], (0, 0), 64)
    s.reserve_canvases(0)
    with pytest.raises(ValueError, match="no canvas reservation"):
        s.compose([0], (0, 0), 64)
    s.reserve_hires(0)


def _record(s):
    """One zero record of the stub pool's layout with a valid meta block."""
    zl, scale, local, depth = s._layout()
    meta = np.zeros(1, N.SESSION_META_DTYPE)
    meta[0] = N.session_meta(zl, scale, local, depth)
    return api.SessionRecords(meta, np.zeros((1, N.session_record_layout(zl, scale, local, depth)[1]), np.uint8))

"""CPU tests of the zoomed views' host side (ian_session_zoom, ian_session_brush_zoom, ian_compose_zoom, ian_compose_brush_zoom;
DESIGN.md 4.14): the numpy functions that specify the arithmetic (npe_ops.zoom_box_mean and the four *_zoom functions, zoom_window),
the packers' refusals, which entries the class calls with which words, and the header / export list."""
import ctypes
import re

import numpy as np
import pytest

from neural_photo_editor_amd import api
from neural_photo_editor_amd import lib as L
from neural_photo_editor_amd import npe_ops as N

from session_helpers import HEADER, StubHandle, header_code, sources, stub_sessions

NEW_EXPORTS = ("ian_session_zoom", "ian_session_brush_zoom", "ian_compose_zoom", "ian_compose_brush_zoom")


def rand_field(seed, amp=0.3):
    return np.float32(np.random.RandomState(seed).uniform(-amp, amp, (3, 64, 64)))


def rand_canvas(w, h, seed):
    return np.uint8(np.random.RandomState(seed).randint(0, 256, (3, h, w)))


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
def test_box_mean_rounds_half_up_and_sums_exactly():
    a = np.zeros((3, 2, 2), np.uint8)
    a[:, 1, :] = 1                                           # the block 0,0,1,1: 2/4 rounds up
    assert np.array_equal(N.zoom_box_mean(a, 2), np.ones((3, 1, 1), np.uint8))
    a[:, 1, 1] = 0                                           # 1/4 rounds down
    assert np.array_equal(N.zoom_box_mean(a, 2), np.zeros((3, 1, 1), np.uint8))
    assert np.array_equal(N.zoom_box_mean(np.full((3, 32, 48), 255, np.uint8), 16), np.full((3, 2, 3), 255, np.uint8))
    rs = np.random.RandomState(0)
    for k, vh, vw in ((1, 5, 4), (3, 4, 8), (5, 7, 4), (16, 2, 4)):
        img = np.uint8(rs.randint(0, 256, (3, k * vh, k * vw)))
        want = np.empty((3, vh, vw), np.uint8)
        for c in range(3):
            for y in range(vh):
                for x in range(vw):
                    want[c, y, x] = (int(img[c, k * y:k * y + k, k * x:k * x + k].sum()) + (k * k) // 2) // (k * k)
        assert np.array_equal(N.zoom_box_mean(img, k), want), k
        assert np.array_equal(N.zoom_box_mean(img, 1), img)
    for bad in (lambda: N.zoom_box_mean(np.zeros((3, 5, 4), np.uint8), 2), lambda: N.zoom_box_mean(np.zeros((3, 4, 4), np.float32), 2),
                lambda: N.zoom_box_mean(np.zeros((3, 4, 4), np.uint8), 0), lambda: N.zoom_box_mean(np.zeros((3, 34, 34), np.uint8), 17),
                lambda: N.zoom_box_mean(np.zeros((3, 4, 4), np.uint8), 2.5), lambda: N.zoom_box_mean(np.zeros((4, 4), np.uint8), 2)):
        with pytest.raises(ValueError):
            bad()


def test_zoom_one_is_the_unzoomed_function():
    s = 3
    src, gim, F, tab = sources(1, s, 3)[0], None, rand_field(1), N.guide_table(12.0)
    gim = N.hires_downsample(src, s)
    for kind in (0, 1):
        assert np.array_equal(N.hires_render_zoom(src, F, kind, s, 4, 1, 36, 38, 1), N.hires_render(src, F, kind, s, 4, 1, 36, 38))
        assert np.array_equal(N.hires_render_guided_zoom(src, gim, F, kind, s, 4, 1, 36, 38, 1, tab),
                              N.hires_render_guided(src, gim, F, kind, s, 4, 1, 36, 38, tab))
    cv = rand_canvas(200, 136, 5)
    placed = [(37, 3, 2, rand_field(2), 0), (100, 60, 1, rand_field(3), 1)]
    placed_g = [p + (N.canvas_crop_mean(cv, p[0], p[1], p[2]),) for p in placed]
    assert np.array_equal(N.canvas_compose_zoom(cv, placed, 4, 8, 1, 64, 45, 1), N.canvas_compose(cv, placed, 4, 8, 1, 64, 45))
    assert np.array_equal(N.canvas_compose_guided_zoom(cv, placed_g, 4, 8, 1, 64, 45, 1, tab),
                          N.canvas_compose_guided(cv, placed_g, 4, 8, 1, 64, 45, tab))


def test_a_zero_field_gives_the_box_mean_of_the_source():
    s, k = 2, 4
    src, Z = sources(1, s, 4)[0], np.zeros((3, 64, 64), np.float32)
    gim, tab = N.hires_downsample(src, s), N.guide_table(8.0)
    want = N.zoom_box_mean(np.ascontiguousarray(src[:, 8:8 + 4 * 7, 4:4 + 4 * 12]), k)
    assert np.array_equal(N.hires_render_zoom(src, Z, 0, s, 4, 8, 12, 7, k), want)
    assert np.array_equal(N.hires_render_guided_zoom(src, gim, Z, 0, s, 4, 8, 12, 7, k, tab), want)
    cv = rand_canvas(200, 136, 6)
    want = N.zoom_box_mean(np.ascontiguousarray(cv[:, 1:1 + 3 * 45, 8:8 + 3 * 64]), 3)
    assert np.array_equal(N.canvas_compose_zoom(cv, [(37, 3, 2, Z, 0)], 4, 8, 1, 64, 45, 3), want)
    assert np.array_equal(N.canvas_compose_guided_zoom(cv, [(37, 3, 2, Z, 0, N.canvas_crop_mean(cv, 37, 3, 2))], 4, 8, 1, 64, 45, 3, tab), want)
    assert np.array_equal(N.canvas_compose_zoom(cv, [], 0, 8, 1, 64, 45, 3), want)      # a window that meets no square


@pytest.mark.parametrize("s", [1, 2, 3, 16])
def test_an_untouched_photo_session_at_zoom_scale_is_its_gim(s):
    src = sources(1, s, 10 + s)[0]
    gim = N.hires_downsample(src, s)
    Z = np.zeros((3, 64, 64), np.float32)
    assert np.array_equal(N.hires_render_zoom(src, Z, 0, s, 0, 0, 64, 64, s), gim)
    assert np.array_equal(N.hires_render_guided_zoom(src, gim, Z, 0, s, 0, 0, 64, 64, s, N.guide_table(5.0)), gim)


def test_a_shifted_window_is_the_crop_of_the_window():
    s, k = 3, 5
    src, F, tab = sources(1, s, 7)[0], rand_field(7), N.guide_table(12.0)
    gim = N.hires_downsample(src, s)
    a, b = 8, 3                                              # (vx + k*a, vy + k*b)
    for kind in (0, 1):
        whole = N.hires_render_zoom(src, F, kind, s, 4, 1, 36, 38, k)
        assert np.array_equal(N.hires_render_zoom(src, F, kind, s, 4 + k * a, 1 + k * b, 36 - a, 38 - b, k), whole[:, b:, a:])
        whole = N.hires_render_guided_zoom(src, gim, F, kind, s, 4, 1, 36, 38, k, tab)
        assert np.array_equal(N.hires_render_guided_zoom(src, gim, F, kind, s, 4 + k * a, 1 + k * b, 36 - a, 38 - b, k, tab), whole[:, b:, a:])
    cv = rand_canvas(200, 136, 8)
    placed = [(37, 3, 2, rand_field(2), 0), (100, 60, 1, rand_field(3), 0), (5, 70, 1, rand_field(4, 0.9), 1)]
    whole = N.canvas_compose_zoom(cv, placed, 4, 0, 0, 64, 45, 3)
    assert np.array_equal(N.canvas_compose_zoom(cv, placed, 4, 3 * 4, 3 * 5, 60, 40, 3), whole[:, 5:, 4:])
    assert not np.array_equal(whole, N.zoom_box_mean(np.ascontiguousarray(cv[:, :135, :192]), 3))      # the fields show


def test_zoom_window():
    assert N.zoom_window(2048, 1536, 4) == (512, 384)
    assert N.zoom_window(2048, 1536, 16) == (128, 96)
    assert N.zoom_window(200, 136, 3) == (64, 45)            # 66 columns fit, 64 is the multiple of 4
    assert N.zoom_window(200, 136, 16) == (12, 8)
    assert N.zoom_window(1028, 1024, 7) == (144, 146)
    assert N.zoom_window(64, 64, 1) == (64, 64)
    assert N.zoom_window(64, 64, 16) == (4, 4)
    for w, h, k in ((200, 136, 3), (1028, 1024, 7), (8192, 8192, 5)):
        vw, vh = N.zoom_window(w, h, k)
        assert vw % 4 == 0 and k * vw <= w < k * (vw + 4) and k * vh <= h < k * (vh + 1)
    for k in (0, 17, 1.5):
        with pytest.raises(ValueError):
            N.zoom_window(64, 64, k)


# ---- the packers ------------------------------------------------------------------------------------------------------------------
def test_packers_take_the_output_size_and_check_the_source_window():
    views, vw, vh = api.pack_session_views([2, 2], [(0, 0), (96, 2)], (32, 38), 3, zoom=3)
    assert (vw, vh) == (32, 38) and [(v.session, v.x, v.y) for v in views] == [(2, 0, 0), (2, 96, 2)]
    api.pack_session_views([0], (12, 2), (36, 38), 3, zoom=5)                    # ends at the picture's edge: 12 + 180, 2 + 190
    api.pack_session_views([0], (0, 0), (4, 4), 1, zoom=16)
    win, vw, vh = api.pack_canvas_windows([0, 0], [(0, 0), (8, 1)], (64, 45), [(200, 136)], zoom=3)
    assert (vw, vh) == (64, 45) and [(w.canvas, w.x, w.y) for w in win] == [(0, 0, 0), (0, 8, 1)]
    for bad, needle in (
            (lambda: api.pack_session_views([0], (0, 0), 64, 1, zoom=0), "zoom must be an integer in 1..16"),
            (lambda: api.pack_session_views([0], (0, 0), 4, 1, zoom=17), "zoom must be"),
            (lambda: api.pack_session_views([0], (0, 0), 4, 1, zoom=2.0), "zoom must be"),
            (lambda: api.pack_session_views([0], (0, 0), 4, 1, zoom=True), "zoom must be"),
            (lambda: api.pack_session_views([0], (0, 0), 64, 1, zoom=2), r"item 0: window \(0,0\) \+ 64 x 64 at zoom 2 outside the 64 x 64 picture"),
            (lambda: api.pack_session_views([0, 0], [(0, 0), (16, 2)], (36, 38), 3, zoom=5), "item 1: window .* at zoom 5 outside"),
            (lambda: api.pack_session_views([0], (2, 0), 8, 1, zoom=2), "window x 2 is not a multiple of 4"),
            (lambda: api.pack_session_views([0], (0, 0), (6, 8), 1, zoom=2), "width 6 is not a multiple of 4"),
            (lambda: api.pack_session_views([0], (0, 0), (0, 8), 1, zoom=2), "at least 1"),
            (lambda: api.pack_session_views([0], (0, 0), (8, 0), 1, zoom=2), "at least 1"),
            (lambda: api.pack_session_views([0], (0, -2), (8, 8), 1, zoom=2), "outside"),
            (lambda: api.pack_canvas_windows([0], (0, 0), 64, [(200, 136)], zoom=0), "zoom must be"),
            (lambda: api.pack_canvas_windows([0], (0, 0), 64, [(200, 136)], zoom=17), "zoom must be"),
            (lambda: api.pack_canvas_windows([0], (0, 0), (64, 46), [(200, 136)], zoom=3), r"item 0: window \(0,0\) \+ 64 x 46 at zoom 3 outside the 200 x 136 canvas"),
            (lambda: api.pack_canvas_windows([0], (12, 0), (64, 45), [(200, 136)], zoom=3), "at zoom 3 outside"),
            (lambda: api.pack_canvas_windows([0], (2, 0), (64, 45), [(200, 136)], zoom=3), "not a multiple of 4"),
    ):
        with pytest.raises(ValueError, match=needle):
            bad()
    # zoom = 1 keeps the words it always had
    with pytest.raises(ValueError, match=r"item 0: window \(4,0\) \+ 64 x 64 outside the 64 x 64 picture"):
        api.pack_session_views([0], (4, 0), 64, 1)
    with pytest.raises(ValueError, match=r"item 0: window \(0,80\) \+ 64 x 64 outside the 200 x 136 canvas"):
        api.pack_canvas_windows([0], (0, 80), 64, [(200, 136)])


# ---- which entry the class calls --------------------------------------------------------------------------------------------------
BOX, COL = (0, 0, 4, 4), (1, 2, 3)


def hires_stub(tips=False):
    s, h = stub_sessions(sourced=(0, 1, 2, 3), scale=3, args=True)
    if tips:
        s.reserve_tips(2)
        s.set_tip(0, np.ones((4, 4)))
        h.calls.clear()
    return s, h


def test_zoom_one_calls_the_old_entries_and_a_zoom_the_new_ones():
    s, h = hires_stub()
    out = s.render([0, 1], (4, 1), (36, 38))
    assert out.shape == (2, 3, 38, 36)
    (name, a), = h.calls
    assert name == "session_render" and len(a) == 4 and a[1:3] == (36, 38) and a[3] is out
    h.calls.clear()
    out = s.render([0, 1], (4, 1), (36, 38), zoom=5)
    (name, a), = h.calls
    assert name == "session_zoom" and a[1:4] == (36, 38, 5) and a[4] is out and out.shape == (2, 3, 38, 36)
    assert [(v.session, v.x, v.y) for v in a[0]] == [(0, 4, 1), (1, 4, 1)]                 # origins stay in full-resolution pixels
    h.calls.clear()
    s.brush_view([2], BOX, COL, origins=(0, 0), size=64)
    s.brush_view([2], BOX, COL, origins=(0, 0), size=64, zoom=3)
    s.paint([2], BOX, COL, view=((0, 0), 64))
    s.paint([2], BOX, COL, view=((0, 0), 64, 3))
    s.scroll([2], BOX, 1.0, view=((12, 2), (36, 38), 5))
    s.scroll([2], BOX, 1.0, view=((12, 2), (36, 38)))
    names = [c[0] for c in h.calls]
    assert names == ["session_brush_view", "session_brush_zoom", "session_brush_view", "session_brush_zoom", "session_brush_zoom",
                     "session_brush_view"]
    ev, tips, shown, views, vw, vh, zoom, out = h.calls[1][1]
    assert tips is None and (vw, vh, zoom) == (64, 64, 3) and shown.shape == (1, 3, 64, 64) and out.shape == (1, 3, 64, 64)
    assert ev[0].session == views[0].session == 2
    assert h.calls[4][1][4:7] == (36, 38, 5) and (h.calls[4][1][3][0].x, h.calls[4][1][3][0].y) == (12, 2)
    for bad in (lambda: s.render([0], (0, 0), 64, zoom=4), lambda: s.brush_view([2], BOX, COL, origins=(0, 0), size=64, zoom=0),
                lambda: s.paint([2], BOX, COL, view=((0, 0), 64, 17)), lambda: s.paint([2], BOX, COL, view=((0, 0),)),
                lambda: s.paint([2], BOX, COL, view=((2, 0), 8, 2))):
        n = len(h.calls)
        with pytest.raises(ValueError):
            bad()
        assert len(h.calls) == n


def test_a_tip_goes_with_the_zoomed_brush_view():
    s, h = hires_stub(tips=True)
    s.brush_view([1], BOX, COL, origins=(0, 0), size=64, tips=0)
    s.brush_view([1], BOX, COL, origins=(0, 0), size=64, tips=0, zoom=3)
    assert [c[0] for c in h.calls] == ["session_brush_tip", "session_brush_zoom"]
    sel = h.calls[1][1][1]
    assert sel.dtype == np.int32 and list(sel) == [0] and h.calls[1][1][6] == 3


def test_compose_and_brush_compose_choose_the_entry_by_the_zoom():
    h = StubHandle(True)
    s = api.EditSessions(h, 8, 100)
    s.reserve_hires(2)
    s._opened = {0, 1, 2, 3}
    s.reserve_canvases(1, 256, 160, 4)
    s.canvas_put(0, np.zeros((3, 136, 200), np.uint8))
    h.calls.clear()
    out = s.compose([0, 0], [(0, 0), (8, 1)], (64, 45), zoom=3)
    s.compose([0], (0, 0), (200, 136))
    s.brush_compose([1], BOX, COL, windows=([0], (8, 0), (12, 8), 16))
    s.brush_compose([1], BOX, COL, windows=([0], (8, 0), (12, 8)))
    s.brush_compose([1], BOX, COL, windows=([0], (8, 0), (12, 8), 1))
    assert [c[0] for c in h.calls] == ["compose_zoom", "canvas_compose", "compose_brush_zoom", "canvas_brush", "canvas_brush"]
    win, vw, vh, zoom, o = h.calls[0][1]
    assert (vw, vh, zoom) == (64, 45, 3) and o is out and out.shape == (2, 3, 45, 64) and [(w.x, w.y) for w in win] == [(0, 0), (8, 1)]
    ev, win, vw, vh, zoom, o, shown = h.calls[2][1]
    assert (vw, vh, zoom) == (12, 8, 16) and o.shape == (1, 3, 8, 12) and shown.shape == (1, 3, 64, 64) and ev[0].session == 1
    assert len(h.calls[3][1]) == 6                                               # the words canvas_brush always got
    for bad in (lambda: s.compose([0], (0, 0), (104, 68), zoom=2), lambda: s.compose([0], (0, 0), 8, zoom=17),
                lambda: s.brush_compose([1], BOX, COL, windows=([0], (8, 0), (12, 9), 16)),
                lambda: s.brush_compose([1], BOX, COL, windows=([0], (8, 0))),
                lambda: s.brush_compose([1], BOX, COL, windows=([0], (8, 0), 8, 2, 2))):
        n = len(h.calls)
        with pytest.raises(ValueError):
            bad()
        assert len(h.calls) == n


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_the_four_entries_are_declared_exported_and_prototyped_alike():
    declared = set(re.findall(r"\b(ian_[a-z_0-9]+)\s*\(", header_code()))
    assert {n for n in declared if n.endswith("_zoom")} == set(NEW_EXPORTS) == {n for n in L.EXPORTS if n.endswith("_zoom")}
    for n in NEW_EXPORTS:       # the patterns the other session tests hold their own names to
        assert not any(w in n for w in ("hires", "render", "view", "stroke", "clone", "tip", "guide", "canvas", "edges")), n
        assert not n.endswith(("_local", "_fit")), n
    lib = L.load_library()
    protos = {name: argt for _, name, argt in L.parse_header_prototypes(HEADER)}
    want = {"ian_session_zoom": 8, "ian_session_brush_zoom": 11, "ian_compose_zoom": 8, "ian_compose_brush_zoom": 11}
    for name in NEW_EXPORTS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == len(protos[name]) == want[name], name

"""Brush tips on the host (ian_sessions_reserve_tips / _set_tip / _tip, ian_session_brush_tip, ian_session_path_tip): the declarations
and the loader, npe_ops.tip_weights / round_tip / tip_rect / tip_seed against what they promise, api.pack_session_tips (every refusal
before the library is reached), EditSessions over a stub (without tips the calls of before, with tips the tips in the library's order)
and csrc/ian_tip_check.h, compiled into a stand-alone program under AddressSanitizer and UBSan (tests/tip_check_main.cpp)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from neural_photo_editor_amd import api, npe_ops as N
from neural_photo_editor_amd import lib as L
from session_helpers import HEADER, ROOT, header_code, stub_sessions

NEW_EXPORTS = ("ian_sessions_reserve_tips", "ian_sessions_set_tip", "ian_sessions_tip", "ian_session_brush_tip", "ian_session_path_tip")
CSRC = os.path.join(ROOT, "neural_photo_editor_amd", "csrc")


# ---- 1. header and loader ----------------------------------------------------------------------------------------------------------
def test_header_and_export_list_agree_on_the_new_names():
    declared = set(re.findall(r"\b(ian_[a-z_0-9]+)\s*\(", header_code()))
    for n in NEW_EXPORTS:
        assert n in declared and n in L.EXPORTS, n
        # the patterns the other session tests hold their own names to
        assert not any(w in n for w in ("stroke", "clone", "guide", "canvas", "hires", "render", "view")) and not n.endswith(("_local", "_fit")), n
    assert {n for n in declared if "tip" in n} == set(NEW_EXPORTS) == {n for n in L.EXPORTS if "tip" in n}
    protos = {name: argt for _, name, argt in L.parse_header_prototypes(HEADER)}
    i32, ptr = "int32_t", "ptr"
    assert protos["ian_sessions_reserve_tips"] == [ptr, i32]
    assert protos["ian_sessions_set_tip"] == [ptr, i32, i32, i32, ptr]
    assert protos["ian_sessions_tip"] == [ptr, i32, ptr, ptr]
    assert protos["ian_session_brush_tip"] == [ptr, i32, ptr, ptr, ptr, ptr, i32, i32, ptr, ptr]
    assert protos["ian_session_path_tip"] == [ptr, i32, ptr, ptr, i32, ptr, i32, ptr, ptr]
    lib = L.load_library()
    for n in NEW_EXPORTS:
        fn = getattr(lib, n)                               # exported by the built library
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == len(protos[n]), n
        assert [a is ctypes.c_int32 for a in fn.argtypes] == [t == i32 for t in protos[n]], n
    # a null handle is an error, not a crash
    ev, st, bx = (L.SessionEvent * 1)(), (L.SessionStroke * 1)(), (L.StrokeBox * 1)()
    one = np.zeros(1, np.int32)
    w = np.ones((2, 2), np.float32)
    assert lib.ian_sessions_reserve_tips(None, 4) != 0
    assert lib.ian_sessions_set_tip(None, 0, 2, 2, L._ptr(w)) != 0
    assert lib.ian_sessions_tip(None, 0, L._ptr(np.zeros(2, np.int32)), None) != 0
    assert lib.ian_session_brush_tip(None, 1, ev, L._ptr(one), None, None, 0, 0, None, None) != 0
    assert lib.ian_session_path_tip(None, 1, st, L._ptr(one), 1, bx, 0, None, None) != 0


# ---- 2. the host's policy: shapes into weights ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("th,tw", [(1, 1), (3, 5), (13, 13), (64, 64)])
def test_tip_weights_of_ones_is_the_rectangles_own_factor(th, tw):
    wn = N.tip_weights(np.ones((th, tw)))
    assert wn.dtype == np.float32 and wn.shape == (th, tw)
    assert np.all(wn == np.float32(1) / np.float32(3 * th * tw))          # seed_inv: 1.f / (float)(3 * th * tw)


def test_tip_weights_sum_to_a_third():
    w = np.random.RandomState(3).uniform(0, 1, (17, 23))
    assert abs(3 * N.tip_weights(w).astype(np.float64).sum() - 1) < 1e-6
    for bad in (np.zeros((2, 2)), -np.ones((2, 2)), np.full((2, 2), np.nan), np.ones(3), np.ones((65, 2)), np.ones((0, 2))):
        with pytest.raises(ValueError):
            N.tip_weights(bad)


@pytest.mark.parametrize("D,hardness", [(1, 0.5), (3, 0.0), (4, 0.5), (7, 0.5), (12, 0.5), (13, 0.25), (33, 0.9), (64, 0.5), (9, 1.0)])
def test_round_tip_is_round(D, hardness):
    w = N.round_tip(D, hardness)
    assert w.dtype == np.float32 and w.shape == (D, D) and w.min() >= 0 and w.max() == 1
    for s in (w.T, w[::-1], w[:, ::-1], w[::-1, ::-1], w.T[::-1], w.T[:, ::-1], w.T[::-1, ::-1]):   # with w itself: the eight symmetries
        assert np.array_equal(s, w)
    R = D / 2.0
    if D % 2 == 1 or hardness * R >= np.sqrt(0.5):      # a pixel whose centre lies inside the flat part: weight 1 at the centre
        assert w[D // 2, D // 2] == 1
    if D >= 4:
        assert w[0, 0] == w[0, -1] == w[-1, 0] == w[-1, -1] == 0
    o = np.arange(D) + 0.5 - R
    r2 = (o[:, None] ** 2 + o[None, :] ** 2).ravel()
    order = np.argsort(r2, kind="stable")
    assert np.all(np.diff(w.ravel()[order]) <= 0)       # non-increasing in the radius
    assert np.all(w.ravel()[r2 >= R * R] == 0) and np.all(w.ravel()[np.sqrt(r2) <= hardness * R] == 1)


def test_round_tip_refusals():
    for D, hd in ((0, 0.5), (65, 0.5), (8, -0.1), (8, 1.5)):
        with pytest.raises(ValueError):
            N.round_tip(D, hd)


@pytest.mark.parametrize("d", [0, 12, 13, 48, 252])
def test_tip_rect_places_a_square_tip_as_brush_rect_places_the_square(d):
    bw = d // 4 + 1
    for x, y in ((0, 0), (63, 0), (0, 63), (63, 63), (31, 29)):
        assert N.tip_rect(x, y, bw, bw) == N.brush_rect(x, y, d), (x, y)
    c1, r1, c2, r2 = N.tip_rect(63, 1, 5, 3)            # not square: pushed back inside on each axis by its own side
    assert (c1, r1, c2, r2) == (59, 0, 64, 3)
    with pytest.raises(ValueError):
        N.tip_rect(3, 3, 0, 4)


@pytest.mark.parametrize("box", [(61, 0, 64, 3), (0, 59, 5, 64), (10, 20, 17, 24)])
def test_tip_seed_against_float64(box):
    rs = np.random.RandomState(5)
    c1, r1, c2, r2 = box
    xhat = rs.uniform(-1, 1, (3, 64, 64)).astype(np.float32)
    wn = N.tip_weights(rs.uniform(0, 1, (r2 - r1, c2 - c1)))
    rgb = np.float32([0.5, -0.25, 0.9])
    want = np.zeros((3, 64, 64))
    want[:, r1:r2, c1:c2] = 2.0 * (xhat[:, r1:r2, c1:c2].astype(np.float64) - rgb.astype(np.float64)[:, None, None]) * wn.astype(np.float64)
    got = N.tip_seed(xhat, box, wn, rgb, 1)
    assert got.dtype == np.float32 and got.shape == (3, 64, 64)
    # two float32 roundings (the difference, the product with wn; the factor 2 is exact) on values below 2 * 2 * max(wn)
    assert np.abs(got - want).max() <= 2 * 2.0 ** -24 * 4 * float(wn.max())
    inside = np.zeros((64, 64), bool)
    inside[r1:r2, c1:c2] = True
    assert np.all(got[:, ~inside] == 0)
    g0 = N.tip_seed(xhat, box, wn, None, 0)
    assert np.all(g0[:, ~inside] == 0) and all(np.array_equal(g0[c, r1:r2, c1:c2], wn) for c in range(3))
    # ones: the rectangle brush's seed, operation by operation 2.f * (xh - t) * inv
    ones = N.tip_weights(np.ones((r2 - r1, c2 - c1)))
    inv = np.float32(1) / np.float32(3 * (r2 - r1) * (c2 - c1))
    rect = np.float32(2) * (xhat[:, r1:r2, c1:c2] - rgb[:, None, None]) * inv
    assert np.array_equal(N.tip_seed(xhat, box, ones, rgb, 1)[:, r1:r2, c1:c2], rect)
    with pytest.raises(ValueError):
        N.tip_seed(xhat, (c1, r1, c2 - 1, r2), wn, rgb, 1)


# ---- 3. pack_session_tips ----------------------------------------------------------------------------------------------------------------
def test_pack_session_tips_broadcasts_and_refuses():
    sizes = {0: (5, 3), 2: (4, 4)}                      # tip -> (tw, th)
    boxes = [[(59, 61, 64, 64)], [(0, 0, 4, 4)], [(1, 1, 9, 2)]]
    got = api.pack_session_tips([0, 2, -1], boxes, sizes, 4)
    assert got.dtype == np.int32 and got.tolist() == [0, 2, -1] and got.flags.c_contiguous
    assert api.pack_session_tips(2, [[(0, 0, 4, 4)], [(8, 8, 12, 12), (9, 9, 13, 13)]], sizes, 4).tolist() == [2, 2]
    assert api.pack_session_tips(-1, boxes, {}, 0).tolist() == [-1, -1, -1]
    bad = [
        (([0, 4, -1], boxes, sizes, 4), r"item 1: tip 4 outside -1\.\.3"),
        (([0, -2, -1], boxes, sizes, 4), "item 1: tip -2 outside"),
        (([0, 1, -1], boxes, sizes, 4), "item 1: tip 1 has never been set"),
        (([2, 2, -1], boxes, sizes, 4), r"item 0: point 0: patch \(59,61,64,64\) is not the 4 x 4 of tip 2"),
        ((2, [[(0, 0, 4, 4), (0, 0, 4, 5)]], sizes, 4), r"item 0: point 1: patch \(0,0,4,5\)"),
        (([0, 2], boxes, sizes, 4), "one integer or 3 integers"),
        (([0.0, 2.0, -1.0], boxes, sizes, 4), "one integer or 3 integers"),
    ]
    for args, needle in bad:
        with pytest.raises(ValueError, match=needle):
            api.pack_session_tips(*args)


# ---- 4. EditSessions over a stub ---------------------------------------------------------------------------------------------------------
def recorded(fn, **kw):
    s, h = stub_sessions(args=True, scale=2, sourced=(0, 1, 2, 3), **kw)
    fn(s)
    return h.calls


def same_call(a, b):
    """Two recorded (name, args): the same name, and argument by argument the same bytes (ctypes arrays, numpy arrays) or value."""
    if a[0] != b[0] or len(a[1]) != len(b[1]):
        return False
    for x, y in zip(a[1], b[1]):
        if isinstance(x, ctypes.Array):
            if bytes(x) != bytes(y):
                return False
        elif isinstance(x, np.ndarray):
            if x.shape != y.shape or x.dtype != y.dtype:           # np.empty results: the bytes are whatever was there
                return False
        elif x != y:
            return False
    return True


BOX = [(10, 10, 14, 14), (20, 20, 24, 24)]
PATHS = [np.array([(1, 1, 5, 5)]), np.array([(2, 2, 6, 6), (3, 3, 7, 7), (4, 4, 8, 8)])]
PTS = [np.array([(5, 5)]), np.array([(6, 6), (63, 7)])]
CALLS = {
    "brush": lambda s, **k: s.brush([0, 1], BOX, (200, 10, 10), **k),
    "brush_view": lambda s, **k: s.brush_view([0, 1], BOX, (200, 10, 10), origins=(4, 8), size=(32, 16), **k),
    "paint": lambda s, **k: s.paint([0, 1], BOX, (200, 10, 10), **k),
    "paint_view": lambda s, **k: s.paint([0, 1], BOX, (200, 10, 10), view=((4, 8), (32, 16)), **k),
    "scroll": lambda s, **k: s.scroll([0, 1], BOX, [1.0, -1.0], **k),
    "scroll_view": lambda s, **k: s.scroll([0, 1], BOX, [1.0, -1.0], view=((4, 8), (32, 16)), **k),
    "stroke": lambda s, **k: s.stroke([0, 1], PATHS, (200, 10, 10), **k),
}
BEFORE = {"brush": "session_brush", "brush_view": "session_brush_view", "paint": "session_brush", "paint_view": "session_brush_view",
          "scroll": "session_brush", "scroll_view": "session_brush_view", "stroke": "session_stroke"}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_without_tips_every_method_makes_the_call_it_made_before(name):
    plain = recorded(lambda s: CALLS[name](s))
    none = recorded(lambda s: CALLS[name](s, tips=None))
    assert [c[0] for c in plain] == [BEFORE[name]] and len(none) == 1 and same_call(plain[0], none[0])
    # the arguments of before, by position: (events, shown) / (events, views, vw, vh, out, shown) / (strokes, boxes, flags, shown)
    assert len(plain[0][1]) == {"session_brush": 2, "session_brush_view": 6, "session_stroke": 4}[BEFORE[name]]
    with_reservation = recorded(lambda s: (s.reserve_tips(4), s.set_tip(1, np.ones((4, 4))), CALLS[name](s)))
    assert [c[0] for c in with_reservation] == ["sessions_reserve_tips", "sessions_set_tip", BEFORE[name]]
    assert same_call(plain[0], with_reservation[2])


def test_paint_stroke_without_a_tip_is_the_call_of_before():
    plain = recorded(lambda s: (s.reserve_history(4), s.paint_stroke([0, 1], PTS, (9, 9, 9), d=12)))
    none = recorded(lambda s: (s.reserve_history(4), s.paint_stroke([0, 1], PTS, (9, 9, 9), d=12, tip=None)))
    assert [c[0] for c in plain] == ["sessions_reserve_history", "session_stroke"] and same_call(plain[1], none[1])


def with_tips(fn):
    def run(s):
        s.reserve_tips(4)
        s.set_tip(1, np.ones((4, 4)))
        s.set_tip(3, N.round_tip(4, 0.5))
        fn(s)
    return recorded(run)[3:]


@pytest.mark.parametrize("name", ["brush", "paint", "scroll"])
def test_with_tips_the_events_and_the_tips_reach_the_library(name):
    (plain,) = recorded(lambda s: CALLS[name](s))
    (call,) = with_tips(lambda s: CALLS[name](s, tips=[3, -1]))
    assert call[0] == "session_brush_tip" and len(call[1]) == 3
    ev, tips, shown = call[1]
    assert bytes(ev) == bytes(plain[1][0]) and tips.dtype == np.int32 and tips.tolist() == [3, -1] and shown.shape == (2, 3, 64, 64)
    (call,) = with_tips(lambda s: CALLS[name](s, tips=1))                # one tip for all
    assert call[1][1].tolist() == [1, 1]


@pytest.mark.parametrize("name", ["brush_view", "paint_view", "scroll_view"])
def test_with_tips_the_windows_travel_with_the_events(name):
    (plain,) = recorded(lambda s: CALLS[name](s))
    (call,) = with_tips(lambda s: CALLS[name](s, tips=[-1, 1]))
    ev0, views0, vw0, vh0, out0, shown0 = plain[1]
    assert call[0] == "session_brush_tip"
    ev, tips, shown, views, vw, vh, out = call[1]
    assert bytes(ev) == bytes(ev0) and bytes(views) == bytes(views0) and (vw, vh) == (vw0, vh0) == (32, 16)
    assert tips.tolist() == [-1, 1] and out.shape == out0.shape == (2, 3, 16, 32) and shown.shape == shown0.shape


def test_stroke_sorts_and_the_tips_follow_the_permutation():
    (plain,) = recorded(lambda s: CALLS["stroke"](s))
    (call,) = with_tips(lambda s: CALLS["stroke"](s, tips=[1, 3], mark=False))
    assert call[0] == "session_path_tip"
    strokes, tips, boxes, flags, got = call[1]
    assert bytes(strokes) == bytes(plain[1][0]) and bytes(boxes) == bytes(plain[1][1]) and flags == 0
    assert [s.session for s in strokes] == [1, 0]                        # the 3-point stroke first
    assert tips.dtype == np.int32 and tips.tolist() == [3, 1] and tips.flags.c_contiguous
    (call,) = with_tips(lambda s: (s.reserve_history(2), CALLS["stroke"](s, tips=[1, -1], mark=True)))[1:]
    assert call[1][1].tolist() == [-1, 1] and call[1][3] == 1


def test_paint_stroke_with_a_tip_takes_tip_rect_rectangles():
    def run(s):
        s.set_tip(2, np.ones((3, 5)), normalise=False)                   # th = 3, tw = 5
        s.paint_stroke([0, 1], PTS, (9, 9, 9), d=200, mark=False, tip=2)
    (_, call) = with_tips(run)
    assert call[0] == "session_path_tip"
    strokes, tips, boxes, flags, _ = call[1]
    assert tips.tolist() == [2, 2] and flags == 0 and [s.session for s in strokes] == [1, 0]
    want = [N.tip_rect(6, 6, 5, 3), N.tip_rect(63, 7, 5, 3), N.tip_rect(5, 5, 5, 3)]
    assert [(b.c1, b.r1, b.c2, b.r2) for b in boxes] == want and want[1] == (59, 6, 64, 9)
    assert [b.gscale for b in boxes] == [6.0, 6.0, 6.0]


def test_the_host_refuses_before_the_library_is_reached():
    def none_reach(fn, needle, setup=True):
        def run(s):
            if setup:
                s.reserve_tips(4)
                s.set_tip(1, np.ones((4, 4)))
            with pytest.raises(ValueError, match=needle):
                fn(s)
        calls = recorded(run)
        assert [c[0] for c in calls] == (["sessions_reserve_tips", "sessions_set_tip"] if setup else []), needle

    none_reach(lambda s: s.brush([0, 1], BOX, (1, 2, 3), tips=1), "no tip reservation", setup=False)
    none_reach(lambda s: s.set_tip(0, np.ones((2, 2))), "no tip reservation", setup=False)
    none_reach(lambda s: s.reserve_tips(65), r"0\.\.64", setup=False)
    none_reach(lambda s: s.brush([0, 1], BOX, (1, 2, 3), tips=[1, 2]), "item 1: tip 2 has never been set")
    none_reach(lambda s: s.brush([0, 1], BOX, (1, 2, 3), tips=[1, 4]), "item 1: tip 4 outside")
    none_reach(lambda s: s.brush([0, 1], [(10, 10, 14, 14), (20, 20, 25, 24)], (1, 2, 3), tips=1), "item 1: point 0: patch")
    none_reach(lambda s: s.stroke([0, 1], PATHS, (1, 2, 3), tips=[1, 2]), "item 1: tip 2 has never been set")
    none_reach(lambda s: s.paint_stroke([0, 1], PTS, (1, 2, 3), mark=False, tip=2), "tip 2 has never been set")
    none_reach(lambda s: s.set_tip(4, np.ones((2, 2))), "tip 4 outside the reservation")
    none_reach(lambda s: s.set_tip(0, -np.ones((2, 2)), normalise=False), "finite and >= 0")
    none_reach(lambda s: s.set_tip(0, np.full((2, 2), np.nan), normalise=False), "finite and >= 0")
    none_reach(lambda s: s.set_tip(0, np.ones((65, 2)), normalise=False), r"both sides 1\.\.64")
    none_reach(lambda s: s.tip(2), "tip 2 has never been set")


def test_a_new_count_forgets_the_tips():
    s, h = stub_sessions(args=True)
    s.reserve_tips(4)
    s.set_tip(1, np.zeros((2, 3)), normalise=False)                      # all zero is allowed as given
    assert s._tips == {1: (3, 2)} and h.calls[-1][0] == "sessions_set_tip" and h.calls[-1][1][0] == 1
    assert h.calls[-1][1][1].dtype == np.float32 and h.calls[-1][1][1].shape == (2, 3)
    s.reserve_tips(4)
    assert s._tips == {1: (3, 2)}
    s.reserve_tips(8)
    assert s._tips == {} and s.tips == 8
    s.close()
    assert s.tips == 0


# ---- 5. csrc/ian_tip_check.h under the sanitizers -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tip_check") / "tip_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "tip_check_main.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (args, r.stderr[-2000:])
    return r.stdout.split()


OK, BAD_SIZE, BAD_WEIGHT, OUTSIDE, NEVER_SET, RECT_SIZE = range(6)


def test_tip_check_sizes(program):
    for tw in (0, 1, 64, 65):
        for th in (0, 1, 64, 65):
            want = OK if tw in (1, 64) and th in (1, 64) else BAD_SIZE
            assert run(program, "size", tw, th) == [str(want)], (tw, th)
    assert run(program, "size", -1, 4) == [str(BAD_SIZE)] and run(program, "size", 2 ** 31 - 1, 1) == [str(BAD_SIZE)]


def test_tip_check_weights(program):
    for tw, th in ((1, 1), (64, 1), (1, 64), (64, 64), (5, 3)):
        last = tw * th - 1
        assert run(program, "weights", tw, th, "none", 0) == [str(OK), "-1"]
        assert run(program, "weights", tw, th, "zero", last) == [str(OK), "-1"]
        for what in ("neg", "nan", "inf", "ninf"):
            for at in sorted({0, last // 2, last}):                       # the last weight: the loop reads all of th * tw and no more
                assert run(program, "weights", tw, th, what, at) == [str(BAD_WEIGHT), str(at)], (tw, th, what, at)


def test_tip_check_events(program):
    tips = (5, 3, 0, 0, 64, 64, 1, 1)                                      # tip 0: 5 x 3, tip 1: never set, tip 2: 64 x 64, tip 3: 1 x 1
    ev = lambda tip, *rect: run(program, "event", tip, *(rect + tips))
    assert ev(0, 59, 61, 64, 64) == [str(OK)]
    assert ev(2, 0, 0, 64, 64) == [str(OK)] and ev(3, 63, 63, 64, 64) == [str(OK)]
    assert ev(-1, 0, 0, 7, 9) == [str(OK)]                                 # no tip: any rectangle
    assert ev(4, 0, 0, 1, 1) == [str(OUTSIDE)] and ev(-2, 0, 0, 1, 1) == [str(OUTSIDE)] and ev(2 ** 31 - 1, 0, 0, 1, 1) == [str(OUTSIDE)]
    assert ev(1, 0, 0, 1, 1) == [str(NEVER_SET)]
    for rect in ((59, 61, 63, 64), (59, 61, 64, 63), (0, 0, 3, 5), (0, 0, 0, 0), (64, 64, 59, 61), (0, 0, 6, 3)):
        assert ev(0, *rect) == [str(RECT_SIZE)], rect
    assert ev(2, 0, 0, 65, 64) == [str(RECT_SIZE)] and ev(3, 5, 5, 5, 6) == [str(RECT_SIZE)]
    assert ev(0, -2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1) == [str(RECT_SIZE)]   # the differences are taken in 64 bits
    assert run(program, "event", -1, 0, 0, 1, 1) == [str(OK)] and run(program, "event", 0, 0, 0, 1, 1) == [str(OUTSIDE)]   # no tips at all


def test_tip_slots(program):
    for tw, th in ((1, 1), (64, 64), (5, 3), (64, 1), (1, 64)):
        assert run(program, "slot", tw, th) == ["ok"], (tw, th)

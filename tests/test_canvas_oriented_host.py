"""CPU tests of oriented placements (ian_place_oriented, ian_placements_oriented): the properties of the numpy
functions that specify the arithmetic (npe_ops.oriented_* / canvas_crop_mean_oriented / canvas_compose_oriented), csrc/ian_oriented.h
against them, compiled into a stand-alone program under AddressSanitizer and UBSan (tests/oriented_main.cpp), the packer's refusals,
the header / export list agreement and the struct's layout."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from neural_photo_editor_amd import api
from neural_photo_editor_amd import lib as L
from neural_photo_editor_amd import npe_ops as N
from session_helpers import HEADER, StubHandle, header_code, run_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural_photo_editor_amd", "csrc")
NEW_EXPORTS = ("ian_place_oriented", "ian_placements_oriented")
W, H = 344, 300


def canvas(seed=0, w=W, h=H):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127.5 + 100.0 * np.sin(xx / 9.0 + rs.uniform(0, 6, (3, 1, 1))) * np.cos(yy / 11.0 + rs.uniform(0, 6, (3, 1, 1)))
    return np.uint8(np.clip(base + rs.randint(-40, 41, (3, h, w)), 0, 255))


def field(seed, kind):
    rs = np.random.RandomState(seed)
    return np.float32(rs.uniform(-1, 1, (3, 64, 64)) * (1.0 if kind else 0.6))


def aligned(ox, oy, s):
    """The oriented form of the upright square (ox, oy) + 64s."""
    return (2 * ox + 64 * s, 2 * oy + 64 * s, s * 65536, 0)


def inside_mask(w, h, p):
    """True where a pixel's centre lies in the square, by the compose's own integers."""
    _, bx, by = N.oriented_derive(p[2], p[3])
    dx = (2 * np.arange(w, dtype=np.int64) + 1 - p[0])[None, :]
    dy = (2 * np.arange(h, dtype=np.int64) + 1 - p[1])[:, None]
    U, V = dx * bx + dy * by, dy * bx - dx * by
    return (U >= -2 ** 26) & (U < 2 ** 26) & (V >= -2 ** 26) & (V < 2 ** 26)


# two squares that overlap at different angles, a sample (kind 1) over both, a small upright one
PLACED = [N.oriented_placement(110, 120, 150, 23) + (field(1, 0), 0), N.oriented_placement(180.5, 150, 129, -157) + (field(2, 0), 0),
          N.oriented_placement(150, 140, 200, 45) + (field(3, 1), 1), N.oriented_placement(300, 250, 70, 90) + (field(4, 0), 0)]


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------
def test_helpers_by_hand():
    assert N.oriented_placement(10.5, 20, 128, 0) == (21, 40, 131072, 0)
    assert N.oriented_placement(10, 20, 64, 90) == (20, 40, 0, 65536)
    assert N.oriented_placement(0, 0, 64, 180)[2:] == (-65536, 0)
    assert N.oriented_derive(65536, 0) == (0, 1 << 20, 0)
    assert N.oriented_derive(0, -65536) == (0, 0, -(1 << 20))
    assert N.oriented_derive(1 << 20, 0) == (4, 1 << 16, 0)
    assert N.oriented_derive(65536, 1)[0] == 1                                 # L2 one above a power of four
    assert N.oriented_derive(131072, 0)[0] == 1 and N.oriented_derive(131072, 1)[0] == 2
    for m, (ax, ay) in enumerate([(65536, 0), (100000, 0), (200000, 10), (0, 400000), (-600000, 600000)]):
        L2 = ax * ax + ay * ay
        got = N.oriented_derive(ax, ay)
        assert got[0] == m and 2 ** (32 + 2 * m) >= L2 and (m == 0 or 2 ** (30 + 2 * m) < L2)
        for a, b in ((ax, got[1]), (ay, got[2])):                             # round to nearest, halves up, negative numerators too
            assert abs(b * L2 - (a << 36)) * 2 <= L2
    for bad in ((65535, 0), (0, 65535), (46340, 46340), ((1 << 20) + 1, 0), (1 << 20, 1), (0, 0), (2 ** 31, 0), (65536.5, 0)):
        with pytest.raises(ValueError):
            N.oriented_derive(*bad)


def test_inside_is_the_brute_force_over_every_sample():
    rs = np.random.RandomState(3)
    seen = set()
    for _ in range(300):
        side, ang = rs.uniform(65, 200), rs.uniform(-180, 180)
        p = N.oriented_placement(rs.uniform(0, W), rs.uniform(0, H), side, ang)
        m = N.oriented_derive(p[2], p[3])[0]
        n = 1 << m
        U = (2 * np.arange(64 * n, dtype=np.int64) + 1 - 64 * n)[None, :]
        V = U.T
        X = ((p[0] << (16 + m)) + U * p[2] - V * p[3]) >> (17 + m)
        Y = ((p[1] << (16 + m)) + U * p[3] + V * p[2]) >> (17 + m)
        want = bool(X.min() >= 0 and X.max() < W and Y.min() >= 0 and Y.max() < H)
        assert N.oriented_inside(W, H, *p) == want, p
        seen.add(want)
    assert seen == {True, False}


@pytest.mark.parametrize("s", [1, 2, 4, 8, 16])
def test_angle_0_is_the_aligned_crop_mean_and_90_degrees_its_rotation(s):
    w, h = (1100, 1040) if s > 4 else (W, H)
    c = canvas(s, w, h)
    for (ox, oy) in ((0, 0), (w - 64 * s, h - 64 * s), (min(37, w - 64 * s), min(11, h - 64 * s))):
        p = aligned(ox, oy, s)
        assert N.oriented_derive(p[2], p[3])[0] == {1: 0, 2: 1, 4: 2, 8: 3, 16: 4}[s]
        want = N.canvas_crop_mean(c, ox, oy, s)
        got = N.canvas_crop_mean_oriented(c, *p)
        assert got.dtype == np.uint8 and got.shape == (3, 64, 64) and np.array_equal(got, want), (s, ox, oy)
        assert np.array_equal(N.canvas_crop_mean_oriented(c, p[0], p[1], 0, s * 65536), np.rot90(want, 1, axes=(1, 2))), (s, ox, oy)


@pytest.mark.parametrize("s", [1, 2, 4, 8, 16])
def test_angle_0_is_the_aligned_compose(s):
    w, h = (1100, 1040) if s > 4 else (W, H)
    c = canvas(10 + s, w, h)
    ox, oy = min(37, w - 64 * s), min(11, h - 64 * s)
    for kind in (0, 1):
        F = field(20 + s + kind, kind)
        for f in (0, 4, 16):
            got = N.canvas_compose_oriented(c, [aligned(ox, oy, s) + (F, kind)], f, 0, 0, w, h)
            assert got.dtype == np.uint8 and np.array_equal(got, N.canvas_compose(c, [(ox, oy, s, F, kind)], f, 0, 0, w, h)), (s, kind, f)


@pytest.mark.parametrize("f", [0, 4])
def test_zero_fields_return_the_canvas_and_nothing_outside_the_squares_changes(f):
    c = canvas()
    zero = [p[:4] + (np.zeros((3, 64, 64), np.float32), 0) for p in PLACED]
    assert np.array_equal(N.canvas_compose_oriented(c, zero, f, 0, 0, W, H), c)
    assert np.array_equal(N.canvas_compose_oriented(c, [p[:4] + (-p[4], 0) for p in zero], f, 0, 0, W, H), c)   # fields of -0.0
    assert np.array_equal(N.canvas_compose_oriented(c, [], f, 0, 0, W, H), c)
    out = N.canvas_compose_oriented(c, PLACED, f, 0, 0, W, H)
    inside = np.zeros((H, W), bool)
    for p in PLACED:
        m = inside_mask(W, H, p)
        x0, y0, x1, y1 = N.oriented_bbox(*p[:4])                               # the bounding box holds the whole square
        ys, xs = np.nonzero(m)
        assert x0 <= xs.min() and xs.max() <= x1 and y0 <= ys.min() and ys.max() <= y1, p[:4]
        assert xs.min() - x0 <= 3 and x1 - xs.max() <= 3 and ys.min() - y0 <= 3 and y1 - ys.max() <= 3     # ... and is tight
        inside |= m
    assert np.array_equal(out[:, ~inside], c[:, ~inside]) and (out[:, inside] != c[:, inside]).any() and not inside.all()


@pytest.mark.parametrize("f", [0, 4, 16])
def test_a_window_is_the_crop_of_the_whole_compose(f):
    c = canvas(7)
    whole = N.canvas_compose_oriented(c, PLACED, f, 0, 0, W, H)
    rs = np.random.RandomState(f)
    wins = [(0, 0, 4, 1), (W - 4, H - 1, 4, 1), (40, 3, 64, 13), (0, 100, W, 8), (132, 0, 136, H), (W - 4, 0, 4, H)]
    for _ in range(8):
        vw, vh = 4 * rs.randint(1, W // 4 + 1), rs.randint(1, H + 1)
        wins.append((4 * rs.randint(0, (W - vw) // 4 + 1), rs.randint(0, H - vh + 1), vw, vh))
    for (vx, vy, vw, vh) in wins:
        assert np.array_equal(N.canvas_compose_oriented(c, PLACED, f, vx, vy, vw, vh), whole[:, vy:vy + vh, vx:vx + vw]), (vx, vy, vw, vh)
    assert np.array_equal(N.canvas_compose_oriented_zoom(c, PLACED, f, 8, 6, 40, 30, 3), N.zoom_box_mean(whole[:, 6:96, 8:128], 3))


def test_compose_refuses_what_is_no_window_or_placement():
    c = canvas()
    F = field(0, 0)
    p = PLACED[0]
    for bad in (lambda: N.canvas_compose_oriented(c, PLACED, 4, 0, 0, W + 4, 8), lambda: N.canvas_compose_oriented(c, PLACED, 4, -4, 0, 8, 8),
                lambda: N.canvas_compose_oriented(c, PLACED, 17, 0, 0, 8, 8), lambda: N.canvas_compose_oriented(c, [p[:5] + (2,)], 4, 0, 0, 8, 8),
                lambda: N.canvas_compose_oriented(c, [(100, 100, 65535, 0, F, 0)], 4, 0, 0, 8, 8),
                lambda: N.canvas_compose_oriented(c, [p] * 9, 4, 0, 0, 8, 8),
                lambda: N.canvas_crop_mean_oriented(c, 60, 200, 65536, 0),       # a sample off the canvas
                lambda: N.canvas_crop_mean_oriented(c, 100, 100, 65535, 0), lambda: N.canvas_crop_mean_oriented(c.astype(np.float32), *p[:4])):
        with pytest.raises(ValueError):
            bad()


# ---- csrc/ian_oriented.h under the sanitizers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("oriented") / "oriented"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "oriented_main.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_the_header_matches_the_python_functions(program):
    Q = 65536
    cases = [(W, H, 200, 180, Q, 0), (W, H, 200, 180, -Q, 0), (W, H, 200, 180, 0, -Q), (W, H, 64, 64, Q, 0), (W, H, 63, 64, Q, 0),
             (W, H, 2 * W - 64, 2 * H - 64, Q, 0), (W, H, 2 * W - 63, 2 * H - 64, Q, 0),
             (2048, 2048, 2048, 2048, 1 << 20, 0), (2048, 2048, 2048, 2048, 0, -(1 << 20)), (2048, 2048, 2049, 2048, 1 << 20, 0),   # L2 = 2^40
             (W, H, 200, 180, Q, 1), (W, H, 200, 180, Q, -1), (W, H, 200, 180, 2 * Q, 1), (W, H, 300, 300, -4 * Q, -1),   # one above a power of four
             (8192, 8192, 8000, 8000, 1 << 19, -(1 << 19)), (W, H, -5, -7, -46341, -46341), (W, H, 2 ** 31 - 1, -2 ** 31, -741455, 741455),
             (W, H, 0, 0, Q - 1, 0), (W, H, 0, 0, 46340, 46340), (W, H, 0, 0, (1 << 20) + 1, 0), (W, H, 0, 0, 1 << 20, 1), (W, H, 0, 0, 0, 0),
             (W, H, 0, 0, 2 ** 31 - 1, -2 ** 31), (W, H, 0, 0, -2 ** 31, -2 ** 31)]
    rs = np.random.RandomState(11)
    for _ in range(60):
        w, h = 4 * rs.randint(16, 600), rs.randint(64, 2400)
        cases.append((w, h) + N.oriented_placement(rs.uniform(-20, w + 20), rs.uniform(-20, h + 20), rs.uniform(60, 1030), rs.uniform(-360, 360)))
    r = subprocess.run([program] + [str(v) for c in cases for v in c], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    seen = set()
    for (w, h, cx2, cy2, ax, ay), line in zip(cases, lines):
        try:
            m, bx, by = N.oriented_derive(ax, ay)
        except ValueError:
            assert line == "bad", (ax, ay, line)
            seen.add("bad")
            continue
        ins = N.oriented_inside(w, h, cx2, cy2, ax, ay)
        seen.add(ins)
        assert line.split() == ["ok"] + [str(v) for v in (m, bx, by, int(ins)) + N.oriented_bbox(cx2, cy2, ax, ay)], (cx2, cy2, ax, ay, line)
    assert seen == {"bad", True, False}


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_the_struct_is_6_words(tmp_path):
    assert ctypes.sizeof(L.CanvasOriented) == 24
    assert [(f, getattr(L.CanvasOriented, f).offset) for f, _ in L.CanvasOriented._fields_] == \
        [("session", 0), ("canvas", 4), ("cx2", 8), ("cy2", 12), ("ax", 16), ("ay", 20)]
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    P = "ian_canvas_oriented"
    out = run_c(tmp_path, ['#include <stdio.h>', '#include <stddef.h>', '#include "ian.h"', 'int main(void) {',
                           '  printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(%s), offsetof(%s, session), offsetof(%s, canvas), '
                           'offsetof(%s, cx2), offsetof(%s, cy2), offsetof(%s, ax), offsetof(%s, ay));' % ((P,) * 7), '  return 0;', '}'])
    assert out[0].split() == ["24", "0", "4", "8", "12", "16", "20"]


def test_header_and_export_list_declare_exactly_the_two_oriented_names():
    declared = set(re.findall(r"\b(ian_[a-z_0-9]+)\s*\(", header_code()))
    assert {n for n in declared if "oriented" in n} == set(NEW_EXPORTS) == {n for n in L.EXPORTS if "oriented" in n}
    for n in NEW_EXPORTS:       # the patterns the other session tests hold their own names to
        assert not ("hires" in n or "render" in n or "view" in n or "canvas" in n or "tip" in n or "edges" in n or "guide" in n), n
        assert not (n.endswith("_local") or n.endswith("_zoom") or n.endswith("_fit")), n
    lib = L.load_library()
    protos = {name: argt for _, name, argt in L.parse_header_prototypes(HEADER)}
    for name in NEW_EXPORTS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == len(protos[name]), name


# ---- the packer and the class ----------------------------------------------------------------------------------------------------
def stub(args=False):
    """EditSessions over a StubHandle with canvases 0 (344 x 300) and 1 (1104 x 1040) put, canvas 2 never; sessions 0..3 opened."""
    h = StubHandle(args)
    s = api.EditSessions(h, 16, 100)
    s.reserve_hires(2)
    s._opened = {0, 1, 2, 3}
    s.reserve_canvases(3, 1104, 1040, 4)
    s.canvas_put(0, np.zeros((3, H, W), np.uint8))
    s.canvas_put(1, np.zeros((3, 1040, 1104), np.uint8))
    h.calls.clear()
    return s, h


def test_packer_broadcasts_and_fills_the_struct():
    sizes = [(W, H), None, (1104, 1040)]
    a, b = N.oriented_placement(150, 140, 150, 23), N.oriented_placement(552.5, 520, 800, -10)
    items = api.pack_canvas_oriented([3, 1], [0, 2], [a, b], sizes)
    assert [(p.session, p.canvas, p.cx2, p.cy2, p.ax, p.ay) for p in items] == [(3, 0) + a, (1, 2) + b]
    items = api.pack_canvas_oriented([2, 5], 0, a, sizes)
    assert [(p.session, p.canvas, p.cx2, p.cy2, p.ax, p.ay) for p in items] == [(2, 0) + a, (5, 0) + a]
    on0 = {i: 0 for i in range(8)}
    api.pack_canvas_oriented([3], 0, a, sizes, placed=on0)                      # a move does not count twice
    with pytest.raises(ValueError, match="item 0: canvas 0 already holds 8"):
        api.pack_canvas_oriented([9], 0, a, sizes, placed=on0)
    with pytest.raises(ValueError, match="item 1: canvas 1 holds no picture"):
        api.pack_canvas_oriented([0, 1], [0, 1], a, sizes)


GOOD = N.oriented_placement(150, 140, 150, 23)


@pytest.mark.parametrize("call", [
    lambda s: s.place_oriented_raw([0, 16], 0, GOOD),                         # an id outside the pool
    lambda s: s.place_oriented_raw([], 0, np.zeros((0, 4), int)),             # n outside 1..256
    lambda s: s.place_oriented_raw([0, 1, 0], 0, GOOD),                       # an id given twice
    lambda s: s.place_oriented_raw([0], 3, GOOD),                             # a canvas outside its range
    lambda s: s.place_oriented_raw([0], 2, GOOD),                             # ... never put
    lambda s: s.place_oriented_raw([0], 0, (300, 280, 65535, 0)),             # L2 below 2^32
    lambda s: s.place_oriented_raw([0], 0, (300, 280, 1 << 20, 1)),           # L2 above 2^40
    lambda s: s.place_oriented_raw([0], 0, (62, 280, 65536, 0)),              # a sample off the canvas: left
    lambda s: s.place_oriented_raw([0], 0, (300, 2 * H - 62, 65536, 0)),      # ... bottom
    lambda s: s.place_oriented_raw([0], 0, N.oriented_placement(40, 140, 100, 45)),   # ... a corner of a tilted square
    lambda s: s.place_oriented_raw([0], 0, (300.0, 280.0, 65536.0, 0.0)),     # the integers are integers
    lambda s: s.place_oriented_raw([0], 0, (2 ** 31, 280, 65536, 0)),
    lambda s: s.place_oriented_raw([0, 1], 0, [GOOD]),                        # one item per id
    lambda s: s.place_oriented([0], 0, (150, 140), 63, 0),                    # a side outside 64..1024
    lambda s: s.place_oriented([0], 0, (150, 140), 1025, 0),
    lambda s: s.place_oriented([0], 0, (150, 140), 150, float("nan")),
    lambda s: s.place_oriented([0, 1], 0, [(150, 140)], 150, 0),
    lambda s: s.placements_oriented(3),
])
def test_invalid_input_raises_before_any_library_call(call):
    s, h = stub()
    with pytest.raises(ValueError):
        call(s)
    assert h.calls == []


def test_valid_calls_reach_the_library_and_track_placements():
    s, h = stub(args=True)
    shown = s.place_oriented([2, 0], 0, [(110, 120), (180.5, 150)], [150, 129], [23, -157])
    assert shown.shape == (2, 3, 64, 64) and [c[0] for c in h.calls] == ["place_oriented"]
    a, b = N.oriented_placement(110, 120, 150, 23), N.oriented_placement(180.5, 150, 129, -157)
    assert [(p.session, p.canvas, p.cx2, p.cy2, p.ax, p.ay) for p in h.calls[0][1][0]] == [(2, 0) + a, (0, 0) + b]
    assert s.placements_oriented(0) == [(0,) + b, (2,) + a] and s.placements(0) == [] and s.placements_oriented(1) == []
    assert 2 in s._opened and 2 not in s._sourced
    # a canvas holds one form; a session that moves away does not count
    h.calls.clear()
    with pytest.raises(ValueError, match="item 0: canvas 0 holds 2 oriented placements"):
        s.place([1], 0, (0, 0), 1)
    s.place([1], 1, (0, 0), 1)
    with pytest.raises(ValueError, match="item 0: canvas 1 holds 1 upright placements"):
        s.place_oriented_raw([3], 1, GOOD)
    with pytest.raises(ValueError, match="placed on canvas 0.*canvas_commit"):
        s.commit([2])
    assert [c[0] for c in h.calls] == ["canvas_place"]
    s.place_oriented_raw([1], 1, GOOD)                                        # the one upright session of canvas 1 becomes oriented
    assert s.placements(1) == [] and s.placements_oriented(1) == [(1,) + GOOD]
    s.place([1], 1, (4, 4), 2)                                                # ... and upright again
    assert s.placements(1) == [(1, 4, 4, 2)] and s.placements_oriented(1) == []
    # the edge-aware compose has no oriented form
    with pytest.raises(ValueError, match="oriented placements exist"):
        s.reserve_canvas_guide(sigma=10.0)
    # commit counts both forms; open, load, put and a smaller pool un-place
    assert s.canvas_commit(0).shape == (2, 3, 64, 64)
    s.open([2], np.zeros((1, 3, 64, 64), np.uint8))
    assert s.placements_oriented(0) == [(0,) + b]
    s.place_oriented_raw([12], 0, GOOD)
    s.reserve(8)
    assert s.placements_oriented(0) == [(0,) + b]
    s.canvas_put(0, np.zeros((3, H, W), np.uint8))
    assert s.placements_oriented(0) == [] and s.placements(1) == [(1, 4, 4, 2)]
    s.reserve_canvas_guide(sigma=10.0)
    h.calls.clear()
    with pytest.raises(ValueError, match="edge-aware compose is on"):
        s.place_oriented_raw([0], 0, GOOD)
    assert h.calls == []

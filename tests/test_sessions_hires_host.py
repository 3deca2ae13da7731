"""CPU tests of the full-resolution edit sessions' host side (ian_sessions_reserve_hires, ian_session_open_hires, ian_session_render,
ian_session_brush_view): the numpy functions that specify the arithmetic (npe_ops.hires_*, edit_field), the view struct's layout
against the header, the view packer (every validation before any library call) and the header / export list agreement."""
import ctypes
import functools
import re
import shutil
import time

import numpy as np
import pytest

from neural_photo_editor_amd import api, npe_ops as N
from neural_photo_editor_amd import lib as L
from session_helpers import HEADER, StubHandle, header_code, run_c, stub_sessions

stub_sessions = functools.partial(stub_sessions, sourced=(0, 1, 2), scale=3)
SCALES = [1, 2, 3, 5, 16]
NEW_EXPORTS = ("ian_sessions_reserve_hires", "ian_session_open_hires", "ian_session_render", "ian_session_brush_view")


def picture(s, seed=0):
    rs = np.random.RandomState(100 * s + seed)
    src = rs.randint(0, 256, (3, 64 * s, 64 * s)).astype(np.uint8)
    field = rs.uniform(-1.5, 1.5, (3, 64, 64)).astype(np.float32)      # beyond +-1: the clip to 0..255 is exercised
    return src, field


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SCALES)
def test_zero_field_returns_the_source_bytes(s):
    src, _ = picture(s)
    S = 64 * s
    assert np.array_equal(N.hires_render(src, np.zeros((3, 64, 64), np.float32), 0, s, 0, 0, S, S), src)
    assert np.array_equal(N.hires_render(src, -np.zeros((3, 64, 64), np.float32), 0, s, 0, 0, S, S), src)     # a field of -0.0 too


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("kind", [0, 1])
def test_a_window_is_the_crop_of_the_whole_render(s, kind):
    src, field = picture(s, 1)
    S = 64 * s
    whole = N.hires_render(src, field, kind, s, 0, 0, S, S)
    assert whole.dtype == np.uint8 and whole.shape == (3, S, S)
    rs = np.random.RandomState(s)
    windows = [(0, 0, 4, 1), (S - 4, S - 1, 4, 1), (0, S // 2, S, 1)]
    for _ in range(6):
        vw, vh = 4 * rs.randint(1, S // 4 + 1), rs.randint(1, S + 1)
        windows.append((4 * rs.randint(0, (S - vw) // 4 + 1), rs.randint(0, S - vh + 1), vw, vh))
    for vx, vy, vw, vh in windows:
        assert np.array_equal(N.hires_render(src, field, kind, s, vx, vy, vw, vh), whole[:, vy:vy + vh, vx:vx + vw]), (vx, vy, vw, vh)


def test_scale_one_is_the_plain_sum():
    src, field = picture(1, 2)
    want = np.uint8(np.clip(np.rint(np.float32(src) + np.float32(127.5) * field), 0, 255))
    assert np.array_equal(N.hires_render(src, field, 0, 1, 0, 0, 64, 64), want)
    assert np.array_equal(N.hires_render(src, field, 1, 1, 0, 0, 64, 64),
                          np.uint8(np.clip(np.rint(np.float32(127.5) * (field + np.float32(1.0))), 0, 255)))
    assert np.array_equal(N.hires_downsample(src, 1), src)
    # rint rounds ties to even, where the reference's bare cast would truncate
    half = np.full((3, 64, 64), np.float32(1.0 / 255.0))               # 127.5 * (1 / 255) = 0.5 exactly
    base = np.zeros((3, 64, 64), np.uint8)
    base[1] = 1
    out = N.hires_render(base, half, 0, 1, 0, 0, 64, 64)
    assert np.all(out[0] == 0) and np.all(out[1] == 2)                  # 0.5 -> 0, 1.5 -> 2


@pytest.mark.parametrize("s", SCALES)
def test_integer_taps_agree_with_the_half_pixel_formula(s):
    S = 64 * s
    i0, i1, t = N.hires_axis_taps(s, 0, S)
    Y = np.arange(S)
    pos = (Y + 0.5) / s - 0.5                                            # exact in float64 for these sizes
    fl = np.floor(pos).astype(np.int64)
    assert np.array_equal(i0, np.clip(fl, 0, 63)) and np.array_equal(i1, np.clip(fl + 1, 0, 63))
    assert t.dtype == np.float32 and np.all(t >= 0) and np.all(t < 1)
    assert np.allclose(t, pos - fl, rtol=0, atol=1e-7)
    # a sub-range is the slice of the whole axis
    lo, cnt = S // 3, S // 2
    for a, b in zip(N.hires_axis_taps(s, lo, cnt), (i0, i1, t)):
        assert np.array_equal(a, b[lo:lo + cnt])


@pytest.mark.parametrize("s", SCALES)
def test_downsample_is_the_exact_rounded_box_mean(s):
    src, _ = picture(s, 3)
    got = N.hires_downsample(src, s)
    assert got.dtype == np.uint8 and got.shape == (3, 64, 64)
    rs = np.random.RandomState(s)
    for _ in range(50):
        c, y, x = rs.randint(3), rs.randint(64), rs.randint(64)
        block = src[c, y * s:(y + 1) * s, x * s:(x + 1) * s].astype(int)
        assert got[c, y, x] == (int(block.sum()) + (s * s) // 2) // (s * s)
    const = np.full((3, 64 * s, 64 * s), 255, np.uint8)
    assert np.all(N.hires_downsample(const, s) == 255)
    with pytest.raises(ValueError):
        N.hires_downsample(src[:, :-1], s)
    with pytest.raises(ValueError):
        N.hires_downsample(src, 17)


def test_edit_field_is_what_the_blend_adds_to_the_photo():
    """IM = from_tanh(to_tanh(RECON) + MASK*DELTA + (1-MASK)*ERROR) with ERROR = to_tanh(GIM) - to_tanh(RECON) is GIM + 127.5 * F up to
    the blend's float64 rounding: at scale 1 the render of (GIM, F) is within one level of the blend's IM, and F is float32."""
    rs = np.random.RandomState(5)
    gim = rs.randint(20, 236, (3, 64, 64)).astype(np.uint8)
    recon = np.uint8(np.clip(gim.astype(int) + rs.randint(-9, 10, gim.shape), 0, 255))
    error = N.to_tanh(np.float32(gim)) - N.to_tanh(np.float32(recon))
    x = np.float32(N.to_tanh(np.float32(recon))) + rs.uniform(-0.05, 0.05, gim.shape).astype(np.float32)
    im, mask = N.photo_blend_host(x, recon, error)
    F = N.edit_field(x, recon, error, mask)
    assert F.dtype == np.float32 and F.shape == (3, 64, 64)
    delta = x - N.to_tanh(np.float32(recon))
    assert np.array_equal(F, np.float32(mask * (np.float64(delta) - np.float64(error))))
    out = N.hires_render(gim, F, 0, 1, 0, 0, 64, 64)
    assert np.abs(out.astype(int) - im.astype(int)).max() <= 1          # truncation (the blend) against rounding (the render)
    # nothing painted: x is the reconstruction, the mask is ~0 and so is the field
    _, m0 = N.photo_blend_host(np.float32(N.to_tanh(np.float32(recon))), recon, error)
    assert np.array_equal(N.hires_render(gim, N.edit_field(np.float32(N.to_tanh(np.float32(recon))), recon, error, m0), 0, 1, 0, 0, 64, 64), gim)


def test_a_whole_1024_render_is_quick_in_numpy():
    src, field = picture(16, 4)
    N.hires_render(src, field, 0, 16, 0, 0, 1024, 1024)
    t0 = time.perf_counter()
    N.hires_render(src, field, 0, 16, 0, 0, 1024, 1024)
    assert time.perf_counter() - t0 < 2.0                               # ~0.1 s: vectorised, not a Python loop per pixel


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_session_view_layout_matches_header(tmp_path):
    cls = L.SessionView
    assert ctypes.sizeof(cls) == 12
    assert [(f, getattr(cls, f).offset) for f, _ in cls._fields_] == [("session", 0), ("x", 4), ("y", 8)]
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ian.h"', 'int main(void) {',
             '  printf("%zu %zu %zu %zu\\n", sizeof(ian_session_view), offsetof(ian_session_view, session), offsetof(ian_session_view, x), '
             'offsetof(ian_session_view, y));',
             '  printf("%d %d %d\\n", IAN_SESSION_FIELD, IAN_SESSION_FIELD_KIND, IAN_SESSION_SOURCE);', '  return 0;', '}']
    out = run_c(tmp_path, lines)
    assert out[0].split() == ["12", "0", "4", "8"]
    assert out[1].split() == [str(L.SESSION_FIELDS[k][0]) for k in ("FIELD", "FIELD_KIND", "SOURCE")] == ["6", "7", "8"]


def test_header_declares_exactly_what_the_library_exports_for_the_new_names():
    declared = set(re.findall(r"\b(ian_[a-z_0-9]+)\s*\(", header_code()))
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS, name
    assert {n for n in declared if "hires" in n or "render" in n or "view" in n} == set(NEW_EXPORTS)
    assert {n for n in L.EXPORTS if "hires" in n or "render" in n or "view" in n} == set(NEW_EXPORTS)
    lib = L.load_library()
    for name in NEW_EXPORTS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32
    protos = {name: argt for _, name, argt in L.parse_header_prototypes(HEADER)}
    for name in NEW_EXPORTS:
        assert len(getattr(lib, name).argtypes) == len(protos[name]), name


# ---- the packer ---------------------------------------------------------------------------------------------------------------
def test_packer_broadcasts_and_fills_the_views():
    views, vw, vh = api.pack_session_views([2, 2, 0], [(0, 0), (96, 0), (4, 191)], (96, 1), 3)
    assert (vw, vh) == (96, 1) and len(views) == 3
    assert [(v.session, v.x, v.y) for v in views] == [(2, 0, 0), (2, 96, 0), (0, 4, 191)]     # the same session twice: tiles
    views, vw, vh = api.pack_session_views([1, 0], (8, 5), 64, 2, capacity=4, opened={0, 1}, sourced={0, 1})
    assert (vw, vh) == (64, 64) and [(v.session, v.x, v.y) for v in views] == [(1, 8, 5), (0, 8, 5)]
    ev = api.pack_session_events([1, 0], (0, 0, 4, 4), (1, 2, 3))
    api.pack_session_views([1, 0], (0, 0), 128, 2, events=ev)
    with pytest.raises(ValueError, match="item 1"):
        api.pack_session_views([1, 2], (0, 0), 128, 2, events=ev)


BOX, COL = (0, 0, 4, 4), (1, 2, 3)


@pytest.mark.parametrize("call", [
    lambda s: s.render([0, 8], (0, 0), 64),                                   # an id outside the pool
    lambda s: s.render([-1], (0, 0), 64),
    lambda s: s.render([4], (0, 0), 64),                                      # a session not opened
    lambda s: s.render([3], (0, 0), 64),                                      # an opened session without a source
    lambda s: s.render([], np.zeros((0, 2), int), 64),                        # n outside 1..256
    lambda s: s.render([0] * 257, (0, 0), 64),
    lambda s: s.render([0], (0, 0), (0, 8)),                                  # vw < 1
    lambda s: s.render([0], (0, 0), (8, 0)),                                  # vh < 1
    lambda s: s.render([0], (0, 0), (-4, 8)),
    lambda s: s.render([0], (0, 0), (196, 8)),                                # a window not inside S x S (S = 192)
    lambda s: s.render([0], (132, 0), (64, 8)),
    lambda s: s.render([0], (0, 129), (64, 64)),
    lambda s: s.render([0], (-4, 0), (64, 64)),
    lambda s: s.render([0], (0, -1), (64, 64)),
    lambda s: s.render([0], (2, 0), (64, 64)),                                # x not a multiple of 4
    lambda s: s.render([0], (0, 0), (66, 64)),                                # vw not a multiple of 4
    lambda s: s.render([0], (0.0, 0.0), (64, 64)),                            # coordinates are integers
    lambda s: s.render([0, 1], [(0, 0)], 64),                                 # one origin per view
    lambda s: s.brush_view([0, 3], BOX, COL, origins=(0, 0), size=64),        # brush_view: a session without a source
    lambda s: s.brush_view([0, 1, 0], BOX, COL, origins=(0, 0), size=64),     # ... the same session twice is still refused for events
    lambda s: s.brush_view([0], (0, 0, 65, 4), COL, origins=(0, 0), size=64),  # ... the event's own checks
    lambda s: s.brush_view([0], BOX, COL, origins=(0, 0), size=(64, 193)),
    lambda s: s.paint([0], BOX, COL, view=((2, 0), 64)),                      # paint / scroll with view=
    lambda s: s.scroll([3], BOX, 1.0, view=((0, 0), 64)),
    lambda s: s.open_hires([4], np.zeros((1, 3, 64, 64), np.uint8)),          # photos of the wrong size for the scale
    lambda s: s.open_hires([4], np.zeros((1, 3, 192, 192), np.float32)),      # photos are uint8
    lambda s: s.open_hires([4, 4], np.zeros((2, 3, 192, 192), np.uint8)),
    lambda s: s.open_hires([8], np.zeros((1, 3, 192, 192), np.uint8)),
    lambda s: s.reserve_hires(17),
    lambda s: s.reserve_hires(-1),
])
def test_invalid_input_raises_before_any_library_call(call):
    s, h = stub_sessions()
    with pytest.raises(ValueError):
        call(s)
    assert h.calls == []


def test_views_differing_from_the_events_are_refused_before_any_library_call():
    ev = api.pack_session_events([0, 1], BOX, COL)
    with pytest.raises(ValueError, match="item 1: the view names session 2, the event session 1"):
        api.pack_session_views([0, 2], (0, 0), 64, 3, events=ev)
    with pytest.raises(ValueError):
        api.pack_session_views([0], (0, 0), 64, 3, events=ev)


def test_without_a_reservation_every_full_resolution_call_is_refused():
    h = StubHandle()
    s = api.EditSessions(h, 8, 100)
    s._opened = {0}
    h.calls.clear()
    for call in (lambda: s.render([0], (0, 0), 64), lambda: s.open_hires([0], np.zeros((1, 3, 64, 64), np.uint8)),
                 lambda: s.brush_view([0], BOX, COL, origins=(0, 0), size=64)):
        with pytest.raises(ValueError, match="no full-resolution reservation"):
            call()
    assert h.calls == []
    with pytest.raises(ValueError):
        api.pack_session_views([0], (0, 0), 64, None)


def test_valid_calls_reach_the_library_and_track_sources():
    s, h = stub_sessions()
    s.open_hires([4, 5], np.zeros((2, 3, 192, 192), np.uint8))
    s.render([4, 4, 5], [(0, 0), (96, 0), (0, 0)], (96, 192))
    s.brush_view([5, 0], BOX, COL, origins=(64, 64), size=(128, 8))
    s.paint([4], BOX, COL, view=((0, 0), 192))
    s.scroll([4], BOX, 1.0, view=((0, 0), 4))
    assert h.calls == ["session_open_hires", "session_render", "session_brush_view", "session_brush_view", "session_brush_view"]
    s.open([4], np.zeros((1, 3, 64, 64), np.uint8))                           # a plain open clears the source
    with pytest.raises(ValueError, match="session 4 has no full-resolution source"):
        s.render([4], (0, 0), 64)
    s.reserve(5)                                                              # shrinking drops the ids that left the pool
    with pytest.raises(ValueError, match="session 5"):
        s.render([5], (0, 0), 64)
    s.reserve_hires(2)                                                        # another scale: every source is gone
    with pytest.raises(ValueError, match="session 0 has no full-resolution source"):
        s.render([0], (0, 0), 64)
    s.reserve_hires(0)
    with pytest.raises(ValueError, match="no full-resolution reservation"):
        s.render([0], (0, 0), 64)

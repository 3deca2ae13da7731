"""The edge-aware render on the host (ian_sessions_reserve_guide, ian_sessions_guide): the declarations and the loader, the numpy
functions that specify the arithmetic (npe_ops.guide_table, hires_render_guided) and EditSessions.reserve_guide / guide over a stub
(every refusal before the library is reached)."""
import ctypes
import re

import numpy as np
import pytest

from neural_photo_editor_amd import npe_ops as N
from neural_photo_editor_amd import lib as L
from session_helpers import HEADER, header_code, stub_sessions

NEW_EXPORTS = ("ian_sessions_reserve_guide", "ian_sessions_guide")


# ---- 1. header and loader ----------------------------------------------------------------------------------------------------------
def test_header_and_export_list_agree_on_the_new_names():
    declared = set(re.findall(r"\b(ian_[a-z_0-9]+)\s*\(", header_code()))
    assert {n for n in declared if "guide" in n} == set(NEW_EXPORTS)
    assert {n for n in L.EXPORTS if "guide" in n} == set(NEW_EXPORTS)
    for n in NEW_EXPORTS:                                  # the patterns the other session tests hold their own names to
        assert not any(w in n for w in ("hires", "render", "view", "canvas", "stroke", "clone")) and not n.endswith(("_local", "_fit")), n
    lib = L.load_library()
    protos = {name: argt for _, name, argt in L.parse_header_prototypes(HEADER)}
    assert protos["ian_sessions_reserve_guide"] == ["ptr", "ptr", "int32_t"]
    assert protos["ian_sessions_guide"] == ["ptr", "ptr"]
    for name in NEW_EXPORTS:                               # exported by the built library, prototypes as declared
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == len(protos[name]), name
    assert lib.ian_sessions_reserve_guide.argtypes[2] is ctypes.c_int32


def test_a_null_handle_is_an_error_not_a_crash():
    lib = L.load_library()
    table = N.guide_table(4.0)
    assert lib.ian_sessions_reserve_guide(None, table.ctypes.data, 766) == -1
    assert lib.ian_sessions_reserve_guide(None, None, 0) == -1
    assert lib.ian_sessions_guide(None, None) == -1
    assert lib.ian_sessions_guide(None, table.ctypes.data) == -1


# ---- 2. the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 4.0, 16.0, 300.0])
def test_guide_table(sigma):
    t = N.guide_table(sigma)
    assert t.dtype == np.float32 and t.shape == (766,) == (N.GUIDE_TABLE_LEN,)
    assert t[0] == np.float32(1.0)
    assert np.all(np.diff(t) <= 0)
    assert np.all(t >= np.float32(2.0 ** -24)) and np.all(np.isfinite(t))
    d = np.arange(766, dtype=np.float64)
    assert np.array_equal(t, np.maximum(np.float32(np.exp(-d * d / (2.0 * (3.0 * sigma) ** 2))), np.float32(2.0 ** -24)))
    if sigma == 0.5:
        assert t[1] < 1 and np.all(t[9:] == np.float32(2.0 ** -24))       # exp(-81 / 4.5) = 1.5e-8 < 2^-24 = 6.0e-8
    if sigma == 300.0:
        assert t[-1] > 0.5                                                   # a wide sigma: nearly the plain bilinear weights


@pytest.mark.parametrize("bad", [0, -1.0, float("nan"), float("inf")])
def test_guide_table_refuses_a_sigma_that_is_no_positive_number(bad):
    with pytest.raises(ValueError):
        N.guide_table(bad)


# ---- 3. the render --------------------------------------------------------------------------------------------------------------------
def picture(s, seed=0):
    rs = np.random.RandomState(1000 * s + seed)
    src = rs.randint(0, 256, (3, 64 * s, 64 * s)).astype(np.uint8)
    field = rs.uniform(-1.5, 1.5, (3, 64, 64)).astype(np.float32)          # beyond +-1: the clip to 0..255 is exercised
    return src, N.hires_downsample(src, s), field


@pytest.mark.parametrize("s", [1, 2, 3, 16])
@pytest.mark.parametrize("sigma", [0.5, 16.0])
def test_zero_field_returns_the_source_bytes(s, sigma):
    src, gim, _ = picture(s)
    S, table = 64 * s, N.guide_table(sigma)
    for zero in (np.zeros((3, 64, 64), np.float32), -np.zeros((3, 64, 64), np.float32)):
        assert np.array_equal(N.hires_render_guided(src, gim, zero, 0, s, 0, 0, S, S, table), src)


@pytest.mark.parametrize("s", [1, 3])
def test_kind_one_is_the_plain_render(s):
    src, gim, field = picture(s, 1)
    S = 64 * s
    got = N.hires_render_guided(src, gim, field, 1, s, 4, 1, S - 4, S - 2, N.guide_table(4.0))
    assert np.array_equal(got, N.hires_render(src, field, 1, s, 4, 1, S - 4, S - 2))


@pytest.mark.parametrize("s", [2, 3])
def test_a_window_is_the_crop_of_the_whole_render(s):
    src, gim, field = picture(s, 2)
    S, table = 64 * s, N.guide_table(8.0)
    whole = N.hires_render_guided(src, gim, field, 0, s, 0, 0, S, S, table)
    assert whole.dtype == np.uint8 and whole.shape == (3, S, S)
    for vx, vy, vw, vh in ((0, 0, 4, 1), (S - 4, S - 1, 4, 1), (8, 7, 40, 9), (0, S // 2, S, 1)):
        assert np.array_equal(N.hires_render_guided(src, gim, field, 0, s, vx, vy, vw, vh, table), whole[:, vy:vy + vh, vx:vx + vw])


@pytest.mark.parametrize("s", [1, 2, 3, 16])
def test_a_table_of_ones_is_the_bilinear_render_within_one_level(s):
    """With every range weight 1 the guided sample is the bilinear one in another order of operations ((1-ty)(1-tx) f00 + ... over a
    denominator of 1 +- a few ulp against two nested lerps): both are within a few ulp of the exact bilinear value, so the rounded
    bytes differ by at most one level, and only where q lies next to a tie."""
    src, gim, field = picture(s, 3)
    S = 64 * s
    a = N.hires_render_guided(src, gim, field, 0, s, 0, 0, S, S, np.ones(766, np.float32))
    b = N.hires_render(src, field, 0, s, 0, 0, S, S)
    diff = np.abs(a.astype(int) - b.astype(int))
    print("scale %d: largest difference %d level(s), %d of %d bytes differ" % (s, diff.max(), np.count_nonzero(diff), diff.size))
    assert diff.max() <= 1
    assert np.count_nonzero(diff) < diff.size // 1000


def test_the_edit_stops_at_an_edge_of_the_photo():
    """Scale 8, a photo of 30 | 220 with the edge 3 pixels inside a field block; the field is 0.5 left of the block's boundary, 0 right."""
    s, S = 8, 512
    E = 8 * 20 + 3
    src = np.full((3, S, S), 30, np.uint8)
    src[:, :, E:] = 220
    gim = N.hires_downsample(src, s)
    field = np.zeros((3, 64, 64), np.float32)
    field[:, :, :20] = 0.5
    win = (E - 12, 256, 24, 1)
    v = N.hires_guide_field(src, gim, field, s, *win, N.guide_table(16.0))[0, 0]
    c0, c1, tx = N.hires_axis_taps(s, E - 12, 24)
    b = field[0, 32, c0] + tx * (field[0, 32, c1] - field[0, 32, c0])       # the bilinear sample of the same row (constant down a column)
    assert v.dtype == np.float32 and v.shape == (24,)
    dark_g, dark_b = np.abs(v[:12] - np.float32(0.5)), np.abs(b[:12] - np.float32(0.5))
    assert np.all(dark_g <= dark_b) and np.any(dark_g < dark_b)
    assert np.all(np.abs(v[12:]) <= np.abs(b[12:]))
    # bilinear ramps across the edge; the guided field holds 0.5 up to it and drops to 0 behind it, up to the floored weight
    # (2^-24 against a neighbour's weight of at least 1/16 * table[3 * 71] = 3e-6) of the tap on the other side
    assert b[:12].min() < 0.1 and b[12:].max() > 0.03
    assert np.all(dark_g < 1e-5) and np.all(np.abs(v[12:]) < 1e-2)


def test_the_denominator_stays_normal():
    """Every spatial weight is a product of two multiples of 1/32 that sum to 1 per axis, so the largest of the four is at least 1/4
    and den >= 2^-2 * 2^-24, far above the smallest normal float32."""
    s = 16
    rs = np.random.RandomState(7)
    src = rs.randint(0, 256, (3, 64 * s, 64 * s)).astype(np.uint8)
    gim = np.uint8(255 - N.hires_downsample(src, s))                        # a guide as far from the photo as it gets
    field = np.ones((3, 64, 64), np.float32)
    v = N.hires_guide_field(src, gim, field, s, 0, 0, 256, 64, N.guide_table(0.5))
    assert np.all(np.isfinite(v)) and np.abs(v - 1).max() < 1e-6            # a constant field comes back whatever the weights


@pytest.mark.parametrize("call", [
    lambda: N.hires_render_guided(*picture(2)[:3], 2, 2, 0, 0, 8, 8, N.guide_table(4.0)),              # kind
    lambda: N.hires_render_guided(*picture(2)[:3], 0, 2, 0, 0, 132, 8, N.guide_table(4.0)),            # a window outside the picture
    lambda: N.hires_render_guided(*picture(2)[:3], 0, 2, 0, 0, 8, 8, np.ones(765, np.float32)),        # the table's length
    lambda: N.hires_render_guided(*picture(2)[:3], 0, 2, 0, 0, 8, 8, np.ones(766, np.float64)),        # ... and type
])
def test_the_render_refuses_bad_arguments(call):
    with pytest.raises(ValueError):
        call()


# ---- 4. EditSessions over a stub ---------------------------------------------------------------------------------------------------------
ONES = np.ones(766, np.float32)


def bad_table(at, value):
    t = ONES.copy()
    t[at] = value
    return t


@pytest.mark.parametrize("call", [
    lambda s: s.reserve_guide(4.0, ONES),                                     # both
    lambda s: s.reserve_guide(sigma=0.0),                                     # junk
    lambda s: s.reserve_guide(sigma=-2.0),
    lambda s: s.reserve_guide(sigma=float("nan")),
    lambda s: s.reserve_guide(table=np.ones(5, np.float32)),
    lambda s: s.reserve_guide(table=np.ones((766, 1), np.float32)),
    lambda s: s.reserve_guide(table=bad_table(3, 0.0)),
    lambda s: s.reserve_guide(table=bad_table(765, -1.0)),
    lambda s: s.reserve_guide(table=bad_table(0, np.nan)),
    lambda s: s.reserve_guide(table=bad_table(9, np.inf)),
])
def test_invalid_input_raises_before_any_library_call(call):
    s, h = stub_sessions(sourced=(0, 1), scale=3)
    with pytest.raises(ValueError):
        call(s)
    assert h.calls == [] and not s.guided


def test_a_guide_needs_the_full_resolution_reservation_and_no_canvases():
    s, h = stub_sessions()
    with pytest.raises(ValueError, match="no full-resolution reservation"):
        s.reserve_guide(4.0)
    assert s.guide() is None
    s.reserve_guide()                                                         # nothing to switch off: no call either
    assert h.calls == []
    s, h = stub_sessions(scale=2)
    s.reserve_canvases(1, 256, 256)
    h.calls.clear()
    with pytest.raises(ValueError, match="canvases are reserved"):
        s.reserve_guide(4.0)
    assert h.calls == []
    s.reserve_canvases(0)
    s.reserve_guide(4.0)
    h.calls.clear()
    with pytest.raises(ValueError, match="a guide is reserved"):
        s.reserve_canvases(1, 256, 256)
    assert h.calls == []


def test_valid_calls_reach_the_library_with_the_table():
    s, h = stub_sessions(sourced=(0, 1), scale=3, args=True)
    s.reserve_guide(4.0)
    assert s.guided
    s.reserve_guide(table=np.float64(N.guide_table(16.0)))                    # any array that converts to float32 (766,)
    s.render([0], (0, 0), 64)                                                 # no new argument anywhere else
    s.reserve_guide()
    assert not s.guided
    names = [c[0] for c in h.calls]
    assert names == ["sessions_reserve_guide", "sessions_reserve_guide", "session_render", "sessions_reserve_guide"]
    assert np.array_equal(h.calls[0][1][0], N.guide_table(4.0)) and h.calls[0][1][0].dtype == np.float32
    assert np.array_equal(h.calls[1][1][0], N.guide_table(16.0)) and h.calls[1][1][0].dtype == np.float32
    assert h.calls[3][1] == (None,)
    s.reserve_guide(2.0)
    s.reserve_hires(0)                                                        # the guide goes with its group
    assert not s.guided and s.guide() is None

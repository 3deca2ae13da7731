"""The edge-aware compose on the host (ian_sessions_reserve_edges, ian_sessions_edges): the numpy function that specifies the
arithmetic (npe_ops.canvas_compose_guided) held against canvas_compose and hires_render_guided, the declarations and the loader, and
EditSessions.reserve_canvas_guide / canvas_guide over a stub (every refusal before the library is reached).  Every comparison of
bytes is np.array_equal."""
import ctypes
import re

import numpy as np
import pytest

from neural_photo_editor_amd import npe_ops as N
from neural_photo_editor_amd import lib as L
from session_helpers import HEADER, header_code, stub_sessions

NEW_EXPORTS = ("ian_sessions_reserve_edges", "ian_sessions_edges")
W, H = 300, 232
TABLE = N.guide_table(8.0)
_cache = {}


def canvas():
    if "c" not in _cache:
        _cache["c"] = np.random.RandomState(3).randint(0, 256, (3, H, W)).astype(np.uint8)
        _cache["c"].setflags(write=False)
    return _cache["c"]


def field(seed):
    return np.random.RandomState(seed).uniform(-0.5, 0.5, (3, 64, 64)).astype(np.float32)


def placement(ox, oy, s, seed, kind=0, zero=False):
    """(ox, oy, s, FIELD, kind, GIM) on the shared canvas: a random field in +-0.5 (or zeros) and the box mean of the square."""
    f = np.zeros((3, 64, 64), np.float32) if zero else field(seed)
    return (ox, oy, s, f, kind, N.canvas_crop_mean(canvas(), ox, oy, s))


def plain(placed):
    return [p[:5] for p in placed]


def crop(ox, oy, s):
    return np.ascontiguousarray(canvas()[:, oy:oy + 64 * s, ox:ox + 64 * s])


# squares at ox % 4 = 1, 1, 3, scales 1, 2, 3
LONE = [(1, 5, 7, 11), (2, 41, 30, 12), (3, 103, 9, 13)]


# ---- 1. the specification ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,ox,oy,seed", LONE)
def test_a_lone_placement_is_the_guided_render_of_the_crop(s, ox, oy, seed):
    c, S = canvas(), 64 * s
    p = placement(ox, oy, s, seed)
    want = N.hires_render_guided(crop(ox, oy, s), p[5], p[3], 0, s, 0, 0, S, S, TABLE)
    outside = np.ones((H, W), bool)
    outside[oy:oy + S, ox:ox + S] = False
    for f in (0, 4):
        got = N.canvas_compose_guided(c, [p], f, 0, 0, W, H, TABLE)
        assert got.dtype == np.uint8 and got.shape == (3, H, W)
        old = N.canvas_compose(c, plain([p]), f, 0, 0, W, H)
        differ = np.count_nonzero(got != old)
        print("scale %d feather %d: %d of %d bytes of the square differ from canvas_compose" % (s, f, differ, 3 * S * S))
        if s >= 2:
            assert differ                                                     # the inputs tell the two functions apart
        m = f * s                                                             # the core: f*s <= u <= 64s-1-f*s
        assert np.array_equal(got[:, oy + m:oy + S - m, ox + m:ox + S - m], want[:, m:S - m, m:S - m]), f
        if f:
            assert not np.array_equal(got[:, oy:oy + S, ox:ox + S], want)     # the rim is feathered
        assert np.array_equal(got[:, outside], c[:, outside]), f              # no byte outside the square changes
        assert (got != c).any()


def test_zero_fields_return_the_canvas_bytes():
    c = canvas()
    placed = [placement(ox, oy, s, 0, zero=True) for (s, ox, oy, _) in LONE]
    placed.append((60, 20, 1, -np.zeros((3, 64, 64), np.float32), 0, N.canvas_crop_mean(c, 60, 20, 1)))
    for f in (0, 4):
        assert np.array_equal(N.canvas_compose_guided(c, placed, f, 0, 0, W, H, TABLE), c)


def test_a_window_is_the_crop_of_the_whole_compose_and_nothing_outside_the_squares_changes():
    c = canvas()
    placed = [placement(ox, oy, s, seed) for (s, ox, oy, seed) in LONE]      # they overlap
    whole = N.canvas_compose_guided(c, placed, 4, 0, 0, W, H, TABLE)
    assert (whole != N.canvas_compose(c, plain(placed), 4, 0, 0, W, H)).any()
    outside = np.ones((H, W), bool)
    for (s, ox, oy, _) in LONE:
        outside[oy:oy + 64 * s, ox:ox + 64 * s] = False
    assert outside.any() and np.array_equal(whole[:, outside], c[:, outside])
    for (vx, vy, vw, vh) in ((0, 0, 4, 1), (W - 4, H - 1, 4, 1), (40, 29, 64, 13), (0, 100, W, 1), (101, 3, 7, 50), (296, 0, 4, H)):
        assert np.array_equal(N.canvas_compose_guided(c, placed, 4, vx, vy, vw, vh, TABLE), whole[:, vy:vy + vh, vx:vx + vw]), (vx, vy)


def test_a_kind_one_placement_inside_a_guided_compose_is_canvas_composes():
    c = canvas()
    for f in (0, 4):
        k1 = placement(41, 30, 2, 21, kind=1)
        assert np.array_equal(N.canvas_compose_guided(c, [k1], f, 0, 0, W, H, TABLE), N.canvas_compose(c, plain([k1]), f, 0, 0, W, H))
        # behind a photo-mode placement it covers entirely, a sample-mode square shows its own bytes in its core, whatever came before
        k0 = placement(103, 9, 3, 22)
        inner = placement(150, 60, 1, 23, kind=1)
        got = N.canvas_compose_guided(c, [k0, inner], f, 0, 0, W, H, TABLE)
        alone = N.canvas_compose(c, plain([inner]), f, 0, 0, W, H)
        core = (slice(None), slice(60 + f, 124 - f), slice(150 + f, 214 - f))
        assert np.array_equal(got[core], alone[core])
        rest = np.ones((H, W), bool)
        rest[60:124, 150:214] = False
        assert np.array_equal(got[:, rest], N.canvas_compose_guided(c, [k0], f, 0, 0, W, H, TABLE)[:, rest])


def test_overlapping_placements_take_their_range_weights_from_the_canvas():
    """acc = canvas + a + b with a, b each placement's own (127.5f*v)*w: if b's field is zero, b adds exactly 0 and the result is the
    lone compose of a -- whatever a wrote under b's square before b was sampled; and a's term does not depend on b's field."""
    c = canvas()
    a, b = placement(41, 30, 2, 31), placement(103, 9, 3, 32)                 # columns 103..168 and rows 30..157 are shared
    a0, b0 = placement(41, 30, 2, 0, zero=True), placement(103, 9, 3, 0, zero=True)
    for f in (0, 4):
        both = N.canvas_compose_guided(c, [a, b], f, 0, 0, W, H, TABLE)
        only_a = N.canvas_compose_guided(c, [a], f, 0, 0, W, H, TABLE)
        only_b = N.canvas_compose_guided(c, [b], f, 0, 0, W, H, TABLE)
        assert np.array_equal(N.canvas_compose_guided(c, [a, b0], f, 0, 0, W, H, TABLE), only_a)
        assert np.array_equal(N.canvas_compose_guided(c, [a0, b], f, 0, 0, W, H, TABLE), only_b)
        shared = (slice(None), slice(30, 158), slice(103, 169))
        assert (both[shared] != only_a[shared]).any() and (both[shared] != only_b[shared]).any()
        # b's sample is computed from the stored bytes: the float sum canvas + a + b, rebuilt from the two lone samples
        va = N.hires_guide_field(crop(41, 30, 2), a[5], a[3], 2, 0, 0, 128, 128, TABLE)
        vb = N.hires_guide_field(crop(103, 9, 3), b[5], b[3], 3, 0, 0, 192, 192, TABLE)
        wa = N.canvas_ramp(2, f, 0, 128)[:, None] * N.canvas_ramp(2, f, 0, 128)[None, :]
        wb = N.canvas_ramp(3, f, 0, 192)[:, None] * N.canvas_ramp(3, f, 0, 192)[None, :]
        acc = np.float32(c)
        acc[:, 30:158, 41:169] = acc[:, 30:158, 41:169] + (np.float32(127.5) * va) * wa
        acc[:, 9:201, 103:295] = acc[:, 9:201, 103:295] + (np.float32(127.5) * vb) * wb
        assert np.array_equal(both, np.uint8(np.clip(np.rint(acc), 0, 255)))


def test_the_edit_stops_at_an_edge_of_the_photo_on_a_canvas():
    """test_sessions_guide_host's edge: scale 8, a photo of 30 | 220 with the edge 3 pixels inside a field block, the field 0.5 left of
    the block's boundary and 0 right of it, sigma 16; here the photo is a square of a canvas at ox % 4 = 3, feather 0.  In the core v
    is hires_guide_field's expression, so its bounds carry over; in bytes: 30 + 127.5 * 0.5 = 93.75 -> 94 up to the edge."""
    s, S, ox, oy = 8, 512, 7, 2
    E = 8 * 20 + 3
    c = np.full((3, 516, 524), 30, np.uint8)
    c[:, :, ox + E:] = 220
    gim = N.canvas_crop_mean(c, ox, oy, s)
    f = np.zeros((3, 64, 64), np.float32)
    f[:, :, :20] = 0.5
    table = N.guide_table(16.0)
    Y = oy + 256
    x0 = ox + E - 12
    got = N.canvas_compose_guided(c, [(ox, oy, s, f, 0, gim)], 0, x0, Y, 24, 1, table)
    old = N.canvas_compose(c, [(ox, oy, s, f, 0)], 0, x0, Y, 24, 1)
    sq = np.ascontiguousarray(c[:, oy:oy + S, ox:ox + S])
    v = N.hires_guide_field(sq, gim, f, s, E - 12, 256, 24, 1, table)
    assert np.array_equal(got, np.uint8(np.clip(np.rint(np.float32(sq[:, 256:257, E - 12:E + 12]) + np.float32(127.5) * v), 0, 255)))
    v = v[0, 0]
    c0, c1, tx = N.hires_axis_taps(s, E - 12, 24)
    b = f[0, 32, c0] + tx * (f[0, 32, c1] - f[0, 32, c0])
    dark_g, dark_b = np.abs(v[:12] - np.float32(0.5)), np.abs(b[:12] - np.float32(0.5))
    assert np.all(dark_g <= dark_b) and np.any(dark_g < dark_b)
    assert np.all(np.abs(v[12:]) <= np.abs(b[12:]))
    assert b[:12].min() < 0.1 and b[12:].max() > 0.03
    assert np.all(dark_g < 1e-5) and np.all(np.abs(v[12:]) < 1e-2)
    assert np.all(got[:, 0, :12] == 94) and np.all(got[:, 0, 12:] <= 221) and np.all(got[:, 0, 12:] >= 220)
    assert old[:, 0, :12].min() < 44 and old[:, 0, 12:].max() > 223            # the plain tap ramps across the edge, on both sides


@pytest.mark.parametrize("call", [
    lambda p: N.canvas_compose_guided(canvas(), [p[:5]], 0, 0, 0, 8, 8, TABLE),                          # a placement without GIM
    lambda p: N.canvas_compose(canvas(), [p], 0, 0, 0, 8, 8),                                            # ... and one too many
    lambda p: N.canvas_compose_guided(canvas(), [p], 0, 0, 0, 8, 8, np.ones(765, np.float32)),           # the table's length
    lambda p: N.canvas_compose_guided(canvas(), [p], 0, 0, 0, 8, 8, np.ones(766, np.float64)),           # ... and type
    lambda p: N.canvas_compose_guided(canvas(), [p], 0, W - 4, 0, 8, 8, TABLE),                          # a window outside the canvas
    lambda p: N.canvas_compose_guided(canvas(), [p] * 9, 0, 0, 0, 8, 8, TABLE),                          # nine placements
    lambda p: N.canvas_compose_guided(canvas(), [p[:4] + (2,) + p[5:]], 0, 0, 0, 8, 8, TABLE),           # kind
])
def test_the_compose_refuses_bad_arguments(call):
    with pytest.raises(ValueError):
        call(placement(5, 7, 1, 1))


# ---- 2. header and loader ----------------------------------------------------------------------------------------------------------
def test_header_and_export_list_agree_on_the_new_names():
    declared = set(re.findall(r"\b(ian_[a-z_0-9]+)\s*\(", header_code()))
    assert {n for n in declared if "edges" in n} == set(NEW_EXPORTS)
    assert {n for n in L.EXPORTS if "edges" in n} == set(NEW_EXPORTS)
    for n in NEW_EXPORTS:                                  # the patterns the other session tests hold their own names to
        assert not any(w in n for w in ("canvas", "guide", "hires", "render", "view", "tip", "clone", "stroke")), n
        assert not n.endswith(("_local", "_fit")), n
    lib = L.load_library()
    protos = {name: argt for _, name, argt in L.parse_header_prototypes(HEADER)}
    assert protos["ian_sessions_reserve_edges"] == ["ptr", "ptr", "int32_t"]
    assert protos["ian_sessions_edges"] == ["ptr", "ptr"]
    for name in NEW_EXPORTS:                               # exported by the built library, prototypes as declared
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == len(protos[name]), name
    assert lib.ian_sessions_reserve_edges.argtypes[2] is ctypes.c_int32


def test_a_null_handle_is_an_error_not_a_crash():
    lib = L.load_library()
    assert lib.ian_sessions_reserve_edges(None, TABLE.ctypes.data, 766) == -1
    assert lib.ian_sessions_reserve_edges(None, None, 0) == -1
    assert lib.ian_sessions_edges(None, None) == -1
    assert lib.ian_sessions_edges(None, TABLE.ctypes.data) == -1


# ---- 3. EditSessions over a stub ---------------------------------------------------------------------------------------------------
ONES = np.ones(766, np.float32)


def bad_table(at, value):
    t = ONES.copy()
    t[at] = value
    return t


def stub_with_canvases(args=False):
    s, h = stub_sessions(scale=2, args=args)
    s.reserve_canvases(1, 256, 256)
    h.calls.clear()
    return s, h


@pytest.mark.parametrize("call", [
    lambda s: s.reserve_canvas_guide(4.0, ONES),                              # both
    lambda s: s.reserve_canvas_guide(sigma=0.0),                              # junk
    lambda s: s.reserve_canvas_guide(sigma=-2.0),
    lambda s: s.reserve_canvas_guide(sigma=float("nan")),
    lambda s: s.reserve_canvas_guide(table=np.ones(5, np.float32)),
    lambda s: s.reserve_canvas_guide(table=np.ones((766, 1), np.float32)),
    lambda s: s.reserve_canvas_guide(table=bad_table(3, 0.0)),
    lambda s: s.reserve_canvas_guide(table=bad_table(765, -1.0)),
    lambda s: s.reserve_canvas_guide(table=bad_table(0, np.nan)),
    lambda s: s.reserve_canvas_guide(table=bad_table(9, np.inf)),
])
def test_invalid_input_raises_before_any_library_call(call):
    s, h = stub_with_canvases()
    with pytest.raises(ValueError):
        call(s)
    assert h.calls == [] and not s.canvas_guided


def test_the_edge_aware_compose_needs_canvases():
    for scale in (0, 2):
        s, h = stub_sessions(scale=scale)
        with pytest.raises(ValueError, match="no canvas"):
            s.reserve_canvas_guide(4.0)
        with pytest.raises(ValueError, match="no canvas"):
            s.reserve_canvas_guide(table=ONES)
        assert s.canvas_guide() is None
        s.reserve_canvas_guide()                                              # nothing to switch off: no call either
        assert h.calls == [] and not s.canvas_guided


def test_valid_calls_reach_the_library_with_the_table_and_a_new_reservation_resets_the_flag():
    s, h = stub_with_canvases(args=True)
    s.reserve_canvas_guide(4.0)
    assert s.canvas_guided and not s.guided
    s.reserve_canvas_guide(table=np.float64(N.guide_table(16.0)))             # any array that converts to float32 (766,)
    s.canvas_put(0, np.zeros((3, 64, 64), np.uint8))
    s.compose([0], (0, 0), 64)                                                # no new argument anywhere else
    s.reserve_canvas_guide()
    assert not s.canvas_guided
    names = [c[0] for c in h.calls]
    assert names == ["sessions_reserve_edges", "sessions_reserve_edges", "canvas_put", "canvas_compose", "sessions_reserve_edges"]
    assert np.array_equal(h.calls[0][1][0], N.guide_table(4.0)) and h.calls[0][1][0].dtype == np.float32
    assert np.array_equal(h.calls[1][1][0], N.guide_table(16.0)) and h.calls[1][1][0].dtype == np.float32
    assert h.calls[4][1] == (None,)
    for count in (2, 0):                                                      # a reservation of any count starts with the plain compose
        if not s.canvases:
            s.reserve_canvases(1, 256, 256)
        s.reserve_canvas_guide(2.0)
        assert s.canvas_guided
        h.calls.clear()
        s.reserve_canvases(count, 128, 128)
        assert not s.canvas_guided and [c[0] for c in h.calls] == ["sessions_reserve_canvas"]
    assert s.canvas_guide() is None
    with pytest.raises(ValueError, match="no canvas"):
        s.reserve_canvas_guide(2.0)
    # the two features still exclude each other at the pool's level, as before
    s.reserve_canvases(1, 256, 256)
    s.reserve_canvas_guide(2.0)
    with pytest.raises(ValueError, match="canvases are reserved"):
        s.reserve_guide(4.0)


def test_the_docstrings_name_the_specification():
    from neural_photo_editor_amd import api
    for fn in (api.EditSessions.compose, api.EditSessions.brush_compose, api.EditSessions.canvas_commit):
        assert "canvas_compose_guided" in fn.__doc__, fn.__name__

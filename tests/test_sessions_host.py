"""CPU tests of the device-resident edit sessions' host side (ian_session_*, IAN.sessions / EditSessions): the event struct's layout
against the header, the event packer (broadcasting, truncation, every validation before any library call), the uint8 -> tanh table
of the open kernel and the brush colour conversion."""
import ctypes
import functools
import shutil

import numpy as np
import pytest

from neural_photo_editor_amd import api, npe_ops
from neural_photo_editor_amd import lib as L
from session_helpers import run_c, stub_sessions

stub_sessions = functools.partial(stub_sessions, opened=(0, 1, 2))


def test_session_event_layout_matches_header(tmp_path):
    """include/ian.h compiles as C and ian_session_event has the size and the field offsets of the ctypes mirror."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    cls = L.SessionEvent
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ian.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(ian_session_event));']
    for fname, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(ian_session_event, %s));' % (fname, fname))
    lines += ['  printf("enum %d %d %d %d %d %d\\n", IAN_SESSION_Z, IAN_SESSION_RECON, IAN_SESSION_ERROR, IAN_SESSION_IM, IAN_SESSION_GIM, '
              'IAN_SESSION_MODE);', '  return 0;', '}']
    out = [l.split() for l in run_c(tmp_path, lines)]
    assert out[0] == ["size", "44"] and ctypes.sizeof(cls) == 44            # 11 words per event
    seen = 0
    for field, val in out[1:-1]:
        assert getattr(cls, field).offset == int(val), field
        seen += 1
    assert seen == len(cls._fields_) == 9
    assert [f for f, _ in cls._fields_] == ["session", "c1", "r1", "c2", "r2", "mode", "coef", "gscale", "rgb"]
    # words 1..7 of an event are an ian_brush_item: the runtime copies them as one
    assert [(f, getattr(cls, f).offset - 4) for f, _ in L.BrushItem._fields_] == [(f, getattr(L.BrushItem, f).offset) for f, _ in L.BrushItem._fields_]
    assert out[-1] == ["enum"] + [str(L.SESSION_FIELDS[k][0]) for k in ("Z", "RECON", "ERROR", "IM", "GIM", "MODE")]


def test_tanh_table_is_the_reference_expression_bit_for_bit():
    """The open kernel maps a uint8 level through this table: NPE.py:257's np.asarray([to_tanh(IM)], dtype=np.float32) per level."""
    tab = L.session_tanh_table()
    ref = np.float32(2.0 * (np.arange(256, dtype=np.uint8) / 255.0) - 1.0)
    assert tab.dtype == np.float32 and np.array_equal(tab.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(tab, np.asarray([npe_ops.to_tanh(np.arange(256, dtype=np.uint8))], dtype=np.float32)[0])


def test_brush_colour_is_paint_events_conversion():
    rs = np.random.RandomState(3)
    for _ in range(20):
        levels = rs.randint(0, 256, 3)
        rgb = np.zeros((3, 64, 64), np.float32)
        rgb[0], rgb[1], rgb[2] = levels                                    # myRGB[0] as tests/session_replay.py builds it
        fed = np.float32(npe_ops.to_tanh(np.float32(rgb)))[None]           # what npe_ops.paint_event feeds brush_step
        c = api.brush_colour(levels)
        assert c.dtype == np.float32
        for ch in range(3):
            assert np.all(fed[0, ch].view(np.uint32) == c[ch:ch + 1].view(np.uint32))
    ev = api.pack_session_events([0], [(1, 2, 3, 4)], [(255, 0, 17)])
    assert np.array_equal(np.float32(list(ev[0].rgb)), api.brush_colour((255, 0, 17)))


def test_packer_broadcasts_truncates_and_forms_coef_gscale():
    ev = api.pack_session_events([7, 2, 9], np.array([(1.9, 2.2, 10.7, 12.0), (0, 0, 64, 64), (5, 5, 5, 9)]), (10, 20, 30), weight=0.05, sign=-1.0)
    assert len(ev) == 3 and [e.session for e in ev] == [7, 2, 9]
    assert (ev[0].c1, ev[0].r1, ev[0].c2, ev[0].r2) == (1, 2, 10, 12)      # floats from Tk are truncated as imgrad's int() does
    assert all(e.mode == 1 for e in ev)
    assert all(np.float32(e.coef) == np.float32(-1.0 * 0.05) for e in ev)
    assert [e.gscale for e in ev] == [10.0, 65.0, 1.0]                     # 1 + (c2 - c1)
    assert all(np.array_equal(np.float32(list(e.rgb)), api.brush_colour((10, 20, 30))) for e in ev)
    # one box for every id, per-item weight / sign, scroll events (no colour: mode 0)
    ev = api.pack_session_events([0, 1], (3, 4, 8, 9), None, None, weight=[0.1, 0.2], sign=[1.0, -1.0])
    assert [(e.c1, e.r1, e.c2, e.r2, e.mode) for e in ev] == [(3, 4, 8, 9, 0)] * 2
    assert np.float32(ev[0].coef) == np.float32(0.1) and np.float32(ev[1].coef) == np.float32(-0.2)
    # mixed modes with per-item colours
    ev = api.pack_session_events([0, 1], [(0, 0, 4, 4)] * 2, [(1, 2, 3), (4, 5, 6)], modes=[0, 1])
    assert [e.mode for e in ev] == [0, 1]
    # the same items as the stateless packer forms
    items = api.pack_brush_items(np.array([(1.9, 2.2, 10.7, 12.0)]), 1, None, 0.05, -1.0)
    e = api.pack_session_events([0], np.array([(1.9, 2.2, 10.7, 12.0)]), (0, 0, 0))[0]
    assert (e.c1, e.r1, e.c2, e.r2, e.mode, e.coef, e.gscale) == tuple(getattr(items[0], f) for f, _ in L.BrushItem._fields_)


@pytest.mark.parametrize("call", [
    lambda s: s.paint([0, 8], (0, 0, 4, 4), (1, 2, 3)),                       # an id outside the pool
    lambda s: s.paint([-1], (0, 0, 4, 4), (1, 2, 3)),
    lambda s: s.paint([0, 5], (0, 0, 4, 4), (1, 2, 3)),                       # an unopened session: brush ...
    lambda s: s.set_latent([5], np.zeros((1, 100), np.float32)),              # ... set_latent ...
    lambda s: s.sample([5], np.zeros((1, 100), np.float32)),
    lambda s: s.reset([5]),                                                   # ... re-open from stored state
    lambda s: s.commit([5]),
    lambda s: s.paint([0, 1, 0], (0, 0, 4, 4), (1, 2, 3)),                    # the same session twice in one call
    lambda s: s.open([3, 3], np.zeros((2, 3, 64, 64), np.uint8)),
    lambda s: s.paint([0], (0, 0, 65, 4), (1, 2, 3)),                         # a rectangle outside the image
    lambda s: s.scroll([0], (-1, 0, 4, 4), 1.0),
    lambda s: s.brush([0], (0, 0, 4, 4), (1, 2, 3), modes=[2]),               # a mode outside {0,1}
    lambda s: s.brush([0], (0, 0, 4, 4), None, modes=[1]),                    # mode 1 without a colour
    lambda s: s.paint([], np.zeros((0, 4)), (1, 2, 3)),                       # n outside 1..256
    lambda s: s.open(np.arange(257), np.zeros((257, 3, 64, 64), np.uint8)),
    lambda s: s.open([3], np.zeros((1, 3, 64, 64), np.float32)),              # photos are uint8
    lambda s: s.read(5),
    lambda s: s.read(8),
])
def test_invalid_input_raises_before_any_library_call(call):
    s, h = stub_sessions()
    with pytest.raises(ValueError):
        call(s)
    assert h.calls == []


def test_valid_calls_reach_the_library_and_track_opened_ids():
    s, h = stub_sessions()
    s.open([3, 4], np.zeros((2, 3, 64, 64), np.uint8))
    s.paint([3, 0], [(0, 0, 4, 4), (1, 1, 2, 2)], (9, 9, 9))
    s.scroll([4], (0, 0, 0, 0), -1.0)                                         # an empty rectangle is valid: zero gradient
    s.reset([3])
    s.commit([4])
    assert h.calls == ["session_open", "session_brush", "session_brush", "session_open", "session_open"]
    with pytest.raises(ValueError, match="257"):
        api.pack_session_events(np.arange(257), (0, 0, 1, 1))
    s.reserve(4)                                                              # shrinking drops the ids that left the pool
    with pytest.raises(ValueError, match="session 4"):
        s.reset([4])

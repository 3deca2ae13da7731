"""What the six session test files share.  Plain functions, no fixtures: each GPU file keeps its own cache of models and pools (their
pools carry different reservations, and the first handle of a pair sees session calls only)."""
import os
import re
import subprocess

import numpy as np
import pytest

from neural_photo_editor_amd import api
from neural_photo_editor_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ian.h")
KEYS64 = ("Z", "RECON", "ERROR", "IM", "GIM", "MODE")


class StubHandle:
    """Records every call that would reach the library: its name, or with args=True (name, arguments)."""

    def __init__(self, args=False):
        self.calls = []
        self.args = args

    def __getattr__(self, name):
        def record(*a, **k):
            self.calls.append((name, a) if self.args else name)
        return record


def stub_sessions(capacity=8, opened=(0, 1, 2, 3), sourced=(), scale=0, reserve=False, args=False):
    """EditSessions over a StubHandle: scale = the full-resolution reservation, reserve = the local one."""
    h = StubHandle(args)
    s = api.EditSessions(h, capacity, 100)
    if scale:
        s.reserve_hires(scale)
    if reserve:
        s.reserve_local()
    s._opened, s._sourced = set(opened), set(sourced)
    h.calls.clear()
    return s, h


def run_c(tmp_path, lines):
    """include/ian.h compiled as strict C99 with `lines` as the program -> the lines it prints."""
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    return [l for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if l]


def header_code():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def model_pool(arch, seed=1, capacity=16):
    """A model with synthetic parameters and its session pool."""
    from neural_photo_editor_amd import IAN
    from oracle import ian_oracle as O
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, seed))
    return m, m.sessions(capacity)


def const_rgb(levels):
    from neural_photo_editor_amd import npe_ops as N
    rgb = np.zeros((3, 64, 64), np.float32)
    rgb[0], rgb[1], rgb[2] = levels                      # myRGB[0] (NPE.py:87,359)
    return np.float32(N.to_tanh(np.float32(rgb)))          # what NPE.py:205 passes to imgradRGB


def sources(n, s, seed):
    """Smooth pictures plus noise at 64*s a side: block means that are no multiples of anything, every byte value present."""
    rs = np.random.RandomState(seed)
    S = 64 * s
    yy, xx = np.mgrid[0:S, 0:S]
    base = 127.5 + 100.0 * np.sin(xx / (5.0 * s) + rs.uniform(0, 6, (n, 3, 1, 1))) * np.cos(yy / (7.0 * s) + rs.uniform(0, 6, (n, 3, 1, 1)))
    return np.uint8(np.clip(base + rs.randint(-40, 41, (n, 3, S, S)), 0, 255))


def assert_fields(got, want, what=KEYS64, tag=None):
    for k in what:
        assert np.array_equal(got[k], want[k]), (tag, k)


def refused(call, needle, code):
    """The library refuses `call` with error `code` and a message that matches `needle`."""
    with pytest.raises(L.IanError, match=needle) as ei:
        call()
    assert "error %d" % code in str(ei.value), str(ei.value)


def session_events(sessions, box=(0, 0, 4, 4), mode=1):
    ev = (L.SessionEvent * len(sessions))()
    for e, sid in zip(ev, sessions):
        e.session, e.mode, e.coef, e.gscale = sid, mode, -0.05, 5.0
        e.c1, e.r1, e.c2, e.r2 = box
    return ev


def session_views(items):
    v = (L.SessionView * len(items))()
    for d, (sid, x, y) in zip(v, items):
        d.session, d.x, d.y = sid, x, y
    return v

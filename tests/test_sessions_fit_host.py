"""ian_session_fit on the host: the declaration and the loader, the Adam step of csrc/ian_fit_step.h compiled for the CPU against its
numpy restatement bit for bit, that restatement against a float64 Adam, the loss helper, and EditSessions.fit over a stub (every
argument error is raised before the library is called)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from neural_photo_editor_amd import api, npe_ops as N
from neural_photo_editor_amd import lib as L
from session_helpers import HEADER, ROOT, header_code, run_c, stub_sessions

CSRC = os.path.join(ROOT, "neural_photo_editor_amd", "csrc")
NEW_EXPORTS = ("ian_session_fit",)


# ---- 1. header and loader ----------------------------------------------------------------------------------------------------------
def test_header_and_export_list_agree_on_the_new_name():
    declared = set(re.findall(r"\b(ian_[a-z_0-9]+)\s*\(", header_code()))
    assert {n for n in declared if n.endswith("_fit")} == set(NEW_EXPORTS)
    assert {n for n in L.EXPORTS if n.endswith("_fit")} == set(NEW_EXPORTS)
    for n in NEW_EXPORTS:       # the patterns the other session tests hold their own names to
        assert not ("hires" in n or "render" in n or "view" in n or "canvas" in n or n.endswith("_local")), n
    lib = L.load_library()
    protos = {name: argt for _, name, argt in L.parse_header_prototypes(HEADER)}
    assert protos["ian_session_fit"] == ["ptr", "int32_t", "ptr", "int32_t", "float", "ptr", "ptr", "ptr"]
    fn = lib.ian_session_fit                           # exported by the built library
    assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == 8
    assert fn.argtypes[3] is ctypes.c_int32 and fn.argtypes[4] is ctypes.c_float


def test_struct_layout_and_prototype_match_the_header(tmp_path):
    """The program defines the function itself: a definition that disagreed with the header's declaration would not compile."""
    assert ctypes.sizeof(L.SessionFitItem) == 20
    assert [(f, getattr(L.SessionFitItem, f).offset) for f, _ in L.SessionFitItem._fields_] == \
        [("session", 0), ("c1", 4), ("r1", 8), ("c2", 12), ("r2", 16)]
    lines = run_c(tmp_path, [
        '#include <stdio.h>', '#include <stddef.h>', '#include "ian.h"',
        'int ian_session_fit(ian_handle* h, int32_t n, const ian_session_fit_item* items, int32_t steps, float lr, double* loss,',
        '                    uint8_t* shown, void* stream) {',
        '  (void)h; (void)items; (void)lr; (void)loss; (void)shown; (void)stream; return n + steps; }',
        'int main(void) {',
        '  printf("%d %d %d %d %d %d\\n", (int)sizeof(ian_session_fit_item), (int)offsetof(ian_session_fit_item, session),',
        '         (int)offsetof(ian_session_fit_item, c1), (int)offsetof(ian_session_fit_item, r1), (int)offsetof(ian_session_fit_item, c2),',
        '         (int)offsetof(ian_session_fit_item, r2));',
        '  printf("%d\\n", ian_session_fit(0, 3, 0, 20, 0.02f, 0, 0, 0));',
        '  return 0;', '}'])
    assert lines == ["20 0 4 8 12 16", "23"]


# ---- 2. the header's step, compiled for the CPU, against numpy: bit for bit ------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fit") / "session_fit"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-I", CSRC, os.path.join(ROOT, "tests", "session_fit_main.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def step_cases(count, seed):
    """(z, g, m, v, lr) float32 arrays and t: magnitudes chosen so that no intermediate of the step is subnormal -- the smallest is
    (0.001f * g) * g >= 1e-3 * 1e-6 * 1e-6 = 1e-15, far above 1.2e-38 -- with exact zeros mixed in (g = 0; m = v = 0, the first step),
    t = 1 and t = 512 among the steps, and both signs."""
    rs = np.random.RandomState(seed)

    def logmag(lo, hi, signed):
        a = 10.0 ** rs.uniform(lo, hi, count)
        return np.float32(a * (rs.choice([-1.0, 1.0], count) if signed else 1.0))

    z = np.float32(rs.uniform(-3, 3, count))
    g = logmag(-6, 2, True)
    m = logmag(-8, 1, True)
    v = logmag(-14, 2, False)
    lr = logmag(-4, 0, False)
    t = rs.randint(1, 513, count)
    g[::7] = 0.0                                        # g = 0
    m[::5] = 0.0
    v[::5] = 0.0                                        # zero moments: the first step of a call
    m[::35], v[::35], z[::35] = 0.0, 0.0, np.float32(1.25)   # g = m = v = 0: Z stays
    t[1::11] = 1
    t[2::11] = 512
    return z, g, m, v, lr, t


def test_header_step_equals_numpy_bitwise(fit_program):
    z, g, m, v, lr, t = step_cases(4000, 11)
    text = "".join("%08x %08x %08x %08x %08x %d\n" % (int(z[i:i + 1].view(np.uint32)[0]), int(g[i:i + 1].view(np.uint32)[0]),
                                                      int(m[i:i + 1].view(np.uint32)[0]), int(v[i:i + 1].view(np.uint32)[0]),
                                                      int(lr[i:i + 1].view(np.uint32)[0]), int(t[i])) for i in range(len(z)))
    r = subprocess.run([fit_program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = np.array([[int(w, 16) for w in line.split()] for line in r.stdout.split("\n")[:-1]], np.uint32)
    assert got.shape == (len(z), 3)
    seen = set()
    for i in range(len(z)):
        zn, mn, vn = N.fit_adam_step(z[i:i + 1], g[i:i + 1], m[i:i + 1], v[i:i + 1], int(t[i]), lr[i])
        want = [int(a.view(np.uint32)[0]) for a in (zn, mn, vn)]
        assert [int(w) for w in got[i]] == want, (i, z[i], g[i], m[i], v[i], lr[i], t[i])
        if g[i] == 0 and m[i] == 0 and v[i] == 0:
            assert zn[0] == z[i]                        # 0 / 1e-8f = 0
            seen.add("still")
        seen.add(int(t[i]) if t[i] in (1, 512) else "mid")
        seen.add("g0" if g[i] == 0 else "g")
    assert seen >= {"still", 1, 512, "mid", "g0", "g"}


def test_consts_are_the_float64_expressions_rounded_once():
    c1, c2 = N.fit_adam_consts(512)
    assert c1.dtype == np.float32 and c2.dtype == np.float32 and c1.shape == c2.shape == (513,)
    assert c1[1] == np.float32(10.0) and c2[1] == np.float32(1.0 / (1.0 - 0.999))
    assert c1[512] == np.float32(1.0) and np.float32(1.0) < c2[512] < np.float32(2.6)
    assert np.all(np.diff(c1[1:].astype(np.float64)) <= 0) and np.all(np.diff(c2[1:].astype(np.float64)) < 0)
    for bad in (0, 513, -1):
        with pytest.raises(ValueError):
            N.fit_adam_consts(bad)


def test_numpy_step_against_a_float64_adam():
    """The float64 Adam uses the same float32 constants (0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, c1[t], c2[t], lr) as exact float64 values, so
    the only difference is the rounding of the float32 operations.  With m and g of one sign (no cancellation in m0 + m1; v's terms
    are never negative) relative errors only add: each float32 operation contributes at most 2^-24, the square root halves what it
    is given, and the chain to the step is m:2, v:3, mh:3, vh:4, lr*mh:4, sqrt:3, +eps:4, the quotient 9 -- inside the 16 x 2^-24
    allowed on the step Z_t - Z_{t-1} (taken with Z_{t-1} = 0, so that the final subtraction is exact)."""
    z, g, m, v, lr, t = step_cases(4000, 12)
    m = np.copysign(m, g)                               # one sign; zeros stay zeros
    z[:] = 0.0
    worst = 0.0
    for i in range(len(z)):
        zn, _, _ = N.fit_adam_step(z[i:i + 1], g[i:i + 1], m[i:i + 1], v[i:i + 1], int(t[i]), lr[i])
        c1, c2 = N.fit_adam_consts(int(t[i]))
        g64, m64, v64 = float(g[i]), float(m[i]), float(v[i])
        mm = float(N.FIT_BETA1) * m64 + float(N.FIT_ONE_M_BETA1) * g64
        vv = float(N.FIT_BETA2) * v64 + float(N.FIT_ONE_M_BETA2) * g64 * g64
        step = (float(lr[i]) * (mm * float(c1[t[i]]))) / (np.sqrt(vv * float(c2[t[i]])) + float(N.FIT_EPS))
        got = -float(zn[0])
        if step == 0.0:
            assert got == 0.0
            continue
        rel = abs(got - step) / abs(step)
        worst = max(worst, rel)
        assert rel <= 16 * 2.0 ** -24, (i, got, step, rel)
    print("fit_adam_step against float64: worst relative error of the step %.3g (bound %.3g)" % (worst, 16 * 2.0 ** -24))


def test_fit_loss():
    rs = np.random.RandomState(3)
    x = np.float32(rs.uniform(-1, 1, (3, 64, 64)))
    T = np.float32(rs.uniform(-1, 1, (3, 64, 64)))
    want = sum((float(x[c, r, k]) - float(T[c, r, k])) ** 2 for c in range(3) for r in range(7, 22) for k in range(5, 30)) / (3 * 15 * 25)
    assert abs(N.fit_loss(x, T, (5, 7, 30, 22)) - want) <= 1125 * 2.0 ** -52 * want
    assert N.fit_loss(x, T, (20, 20, 20, 30)) == 0.0 and N.fit_loss(x, T, (20, 30, 25, 30)) == 0.0
    assert N.fit_loss(x, x, (0, 0, 64, 64)) == 0.0
    assert isinstance(N.fit_loss(x, T, (0, 0, 64, 64)), float)


# ---- 3. EditSessions.fit over a stub -----------------------------------------------------------------------------------------------
def test_packer_broadcasts_and_fills_the_structs():
    items, steps, lr = api.pack_session_fit([3, 1], 7, 0.5)
    assert [(p.session, p.c1, p.r1, p.c2, p.r2) for p in items] == [(3, 0, 0, 64, 64), (1, 0, 0, 64, 64)]
    assert steps == 7 and lr == 0.5
    items, _, lr = api.pack_session_fit([3, 1, 0], 512, 0.02, [(5, 7, 30, 22), (0, 0, 64, 64), (20.9, 20, 20, 30)])
    assert [(p.session, p.c1, p.r1, p.c2, p.r2) for p in items] == [(3, 5, 7, 30, 22), (1, 0, 0, 64, 64), (0, 20, 20, 20, 30)]
    assert lr == float(np.float32(0.02))
    assert [(p.c1, p.r1, p.c2, p.r2) for p in api.pack_session_fit(5, 1, 1.0, (1, 2, 3, 4))[0]] == [(1, 2, 3, 4)]


def test_a_valid_call_reaches_the_library_with_the_packed_arguments():
    s, h = stub_sessions(args=True)
    recon, loss = s.fit([2, 0], steps=3, lr=0.25, boxes=(5, 7, 30, 22))
    (name, (items, steps, lr, loss_arg, shown_arg)), = h.calls
    assert name == "session_fit" and steps == 3 and lr == 0.25
    assert [(p.session, p.c1, p.r1, p.c2, p.r2) for p in items] == [(2, 5, 7, 30, 22), (0, 5, 7, 30, 22)]
    assert recon is shown_arg and recon.shape == (2, 3, 64, 64) and recon.dtype == np.uint8
    assert loss is loss_arg and loss.shape == (2, 4) and loss.dtype == np.float64
    h.calls.clear()
    recon, loss = s.fit([1], want_loss=False)          # the defaults: 20 steps at 0.02
    (name, (items, steps, lr, loss_arg, shown_arg)), = h.calls
    assert loss is None and loss_arg is None and steps == 20 and lr == float(np.float32(0.02)) and recon.shape == (1, 3, 64, 64)
    assert "nobody has measured" in api.EditSessions.fit.__doc__


@pytest.mark.parametrize("call", [
    lambda s: s.fit([0, 1], steps=0),                                  # steps outside 1..512
    lambda s: s.fit([0, 1], steps=513),
    lambda s: s.fit([0, 1], steps=2.5),
    lambda s: s.fit([0, 1], lr=0.0),                                   # lr not finite or not positive
    lambda s: s.fit([0, 1], lr=-0.02),
    lambda s: s.fit([0, 1], lr=float("nan")),
    lambda s: s.fit([0, 1], lr=float("inf")),
    lambda s: s.fit([0, 1], lr=1e-60),                                 # zero as a float32
    lambda s: s.fit([1, 1]),                                           # an id twice
    lambda s: s.fit([0, 5]),                                           # an unopened session
    lambda s: s.fit([0, 8]),                                           # outside the pool
    lambda s: s.fit([]),
    lambda s: s.fit([0, 1], boxes=(10, 10, 65, 20)),                   # a rectangle outside the image
    lambda s: s.fit([0, 1], boxes=(-1, 10, 5, 20)),
    lambda s: s.fit([0, 1], boxes=[(0, 0, 4, 4), (0, 0, 4, 65)]),
    lambda s: s.fit([0, 1], boxes=[(0, 0, 4, 4)]),                     # one box for two sessions
])
def test_invalid_input_raises_before_any_library_call(call):
    s, h = stub_sessions()
    with pytest.raises(ValueError):
        call(s)
    assert h.calls == []

"""Device-resident edit sessions (ian_session_*, IAN.sessions / EditSessions): open, brush, sample, set_latent, reset and commit by
session id.  The reference for equality is always the existing STATELESS public path at the same n and item order (encode_images,
sample_at_uint8, brush_step_batch with constant-colour RGB images, the numpy lines of NPE.py between them) -- bitwise, because the
same kernels run on bit-identical inputs at the same batch -- and the reference-executed NPE.py session of tests/golden."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import ian_oracle as O
from session_helpers import ROOT, assert_fields as assert_session, const_rgb, model_pool, refused, session_events as events

pytestmark = pytest.mark.gpu

CAP = 16

_cache = {}


def model_for(arch):
    """One model and one pool per arch, kept across tests."""
    if arch not in _cache:
        _cache[arch] = model_pool(arch)
    return _cache[arch]


def photos(n, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, 3, 64, 64)).astype(np.uint8)


def host_open(m, ph):
    """NPE.infer (NPE.py:257-264) through the stateless calls at batch n -> list of session dicts."""
    from neural_photo_editor_amd import npe_ops as N
    Z = m.encode_images(np.float32(N.to_tanh(ph)))
    RECON = m.sample_at_uint8(Z)
    return [dict(Z=Z[i].copy(), RECON=RECON[i], ERROR=N.to_tanh(np.float32(ph[i])) - N.to_tanh(np.float32(RECON[i])), IM=ph[i].copy(),
                 GIM=ph[i].copy(), MODE=0) for i in range(len(ph))]


@pytest.mark.parametrize("arch", O.ARCHS)
@pytest.mark.parametrize("n", [1, 5])
def test_open_equals_the_stateless_calls_bitwise(arch, n):
    m, s = model_for(arch)
    ph = photos(n, 10 + n)
    ids = [7, 2, 11, 0, 5][:n]
    shown = s.open(ids, ph)
    want = host_open(m, ph)
    assert np.array_equal(shown, ph)
    for i, sid in enumerate(ids):
        got = s.read(sid)
        assert got["ERROR"].dtype == np.float32 and got["Z"].dtype == np.float32
        assert_session(got, want[i], tag=(arch, n, i))
        assert got["MODE"] == 0


# ---- the brush script: the pool against a host-side model driven by brush_step_batch ----------------------------------------
def model_brush(m, M, ids, boxes, colours, modes, weight, sign):
    """One stateless call on the host-held state of sessions `ids`, in that order -> shown; M is updated as NPE.py updates its globals."""
    from neural_photo_editor_amd import npe_ops as N
    n = len(ids)
    z = np.stack([M[i]["Z"] for i in ids])
    rgb = np.stack([const_rgb(colours[k]) if modes[k] else np.zeros((3, 64, 64), np.float32) for k in range(n)])
    recon = np.stack([M[i]["RECON"] for i in ids])
    error = np.stack([M[i]["ERROR"] for i in ids])
    z_new, x, im, _ = m.brush_step_batch(np.asarray(boxes), z, rgb, weight=weight, sign=sign, modes=modes, photo=(recon, error))
    shown = np.empty((n, 3, 64, 64), np.uint8)
    for k, i in enumerate(ids):
        M[i]["Z"] = z_new[k].copy()
        if M[i]["MODE"] == 0 and modes[k] == 1:            # NPE.paint in photo mode: the blend becomes IM
            M[i]["IM"] = im[k].copy()
            shown[k] = im[k]
        else:                                              # sample mode, and NPE.scroll in either: update_photo(None)
            shown[k] = np.uint8(N.from_tanh(x[k]))
    return shown


def run_brush_script(arch):
    """>= 8 brush calls on 6 sessions: paint and scroll, photo- and sample-mode sessions, the same ids in the same order (residency
    hit), a permuted order, a subset, a set_latent between two calls (version bump), one empty rectangle.  The host model runs the
    whole script first through the stateless calls; then the pool runs it with nothing but ian_session_read between its calls (any
    other call would end the residency), and after every call Z, IM and shown equal the model's.
    -> the pool's per-call (shown, Z rows, IM rows) for a comparison across processes."""
    from neural_photo_editor_amd import npe_ops as N
    m, s = model_for(arch)
    ids = [3, 9, 1, 12, 6, 4]
    ph = photos(6, 77)
    zs = O.make_latents(2, seed=5)
    rs = np.random.RandomState(21)
    script = [
        ("paint", ids),                     # 0
        ("paint", ids),                     # 1: same ids, same order: the forward at Z is skipped
        ("scroll", ids),                    # 2: residency again, lighten events
        ("mixed", ids[::-1]),               # 3: permuted order
        ("paint", [9, 12, 4]),              # 4: a subset
        ("paint", [9, 12, 4]),              # 5: hit
        ("set_latent", [12, 9]),            # a version bump between two calls on the same ids
        ("paint", [9, 12, 4]),              # 6
        ("empty", ids),                     # 7: one empty rectangle among the boxes
        ("scroll", [6]),                    # 8: n = 1 on the batched path
    ]
    plan = []
    for step, (kind, sel) in enumerate(script):
        n = len(sel)
        if kind == "set_latent":
            plan.append((kind, sel, O.make_latents(n, seed=40 + step)))
            continue
        c1, r1 = rs.randint(0, 56, n), rs.randint(0, 56, n)
        boxes = np.stack([c1, r1, c1 + rs.randint(1, 9, n), r1 + rs.randint(1, 9, n)], 1)
        if kind == "empty":
            boxes[2] = (20, 20, 20, 30)
        modes = {"paint": [1] * n, "scroll": [0] * n, "mixed": [k % 2 for k in range(n)], "empty": [1] * n}[kind]
        colours = rs.randint(0, 256, (n, 3))
        weight = np.where(np.array(modes) == 1, 0.05, 0.1)
        sign = np.where(np.array(modes) == 1, -1.0, rs.choice([-1.0, 1.0], n))
        plan.append((kind, sel, (boxes, colours, modes, weight, sign)))
    # ---- the host model, through the stateless calls
    M = dict(zip(ids, host_open(m, ph)))
    rec = m.sample_at_uint8(zs)
    for k, i in enumerate((12, 6)):                       # sessions 12 and 6 go to sample mode (NPE.py:317-327)
        M[i].update(Z=zs[k].copy(), RECON=rec[k], ERROR=N.to_tanh(np.float32(M[i]["IM"])) - N.to_tanh(np.float32(rec[k])), MODE=1)
    want = []
    for kind, sel, arg in plan:
        if kind == "set_latent":
            xs = m.sample_at(arg)
            shown = np.empty((len(sel), 3, 64, 64), np.uint8)
            for k, i in enumerate(sel):
                M[i]["Z"] = arg[k].copy()
                shown[k] = N.photo_blend_host(xs[k], M[i]["RECON"], M[i]["ERROR"])[0] if M[i]["MODE"] == 0 else np.uint8(N.from_tanh(xs[k]))
        else:
            shown = model_brush(m, M, sel, *arg)
        want.append((shown, [{k: np.copy(v) for k, v in M[i].items()} for i in sel]))
    # ---- the pool
    s.open(ids, ph)
    s.sample([12, 6], zs)
    out = []
    for step, ((kind, sel, arg), (shown_w, state_w)) in enumerate(zip(plan, want)):
        shown = s.set_latent(sel, arg) if kind == "set_latent" else s.brush(sel, *arg)
        got = [s.read(i) for i in sel]
        assert np.array_equal(shown, shown_w), (arch, step, kind)
        for k, i in enumerate(sel):
            assert_session(got[k], state_w[k], tag=(arch, step, kind, i))
        if kind != "set_latent":
            out.append((shown, np.stack([g["Z"] for g in got]), np.stack([g["IM"] for g in got])))
    return out


@pytest.mark.parametrize("arch", O.ARCHS)
def test_brush_equals_the_stateless_batch_bitwise(arch, tmp_path):
    t0 = time.time()
    here = run_brush_script(arch)
    assert len(here) >= 8
    print("brush script %s: %.1f s" % (arch, time.time() - t0))
    # the same script with the residency switched off, in a fresh child process: the same checks there, and the same bytes as here
    dump = str(tmp_path / "nocache.npz")
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import test_gpu_sessions as T; out = T.run_brush_script(%r); "
            "np.savez(%r, **{'%%d_%%d' %% (i, j): a for i, o in enumerate(out) for j, a in enumerate(o)})" % (os.path.join(ROOT, "tests"), arch, dump))
    env = dict(os.environ, IAN_NO_DEC_CACHE="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    there = np.load(dump)
    for i, o in enumerate(here):
        for j, a in enumerate(o):
            assert np.array_equal(there["%d_%d" % (i, j)], a), (arch, i, j)


@pytest.mark.parametrize("arch", O.ARCHS)
def test_sample_set_latent_commit(arch):
    from neural_photo_editor_amd import npe_ops as N
    m, s = model_for(arch)
    ids = [8, 13, 2]
    ph = photos(3, 31)
    s.open(ids, ph)
    M = host_open(m, ph)
    # paint_latents in photo mode (NPE.py:296-302): the blend is shown, the stored IM stays
    z = O.make_latents(3, seed=32)
    shown = s.set_latent(ids, z)
    xs = m.sample_at(z)
    for k, sid in enumerate(ids):
        assert np.array_equal(shown[k], N.photo_blend_host(xs[k], M[k]["RECON"], M[k]["ERROR"])[0]), (arch, k)
        got = s.read(sid)
        assert np.array_equal(got["Z"], z[k]) and np.array_equal(got["IM"], ph[k]) and got["MODE"] == 0
        assert_session(got, M[k], ("RECON", "ERROR", "GIM"))
    # a paint event moves IM away from GIM, then UpdateGIM (NPE.py:342-345): GIM := IM, Reset
    s.paint(ids, (20, 20, 40, 40), (250, 10, 10), weight=0.5)
    before = [s.read(sid) for sid in ids]
    assert any((b["IM"] != b["GIM"]).any() for b in before)
    shown = s.commit(ids)
    want = host_open(m, np.stack([b["IM"] for b in before]))
    for k, sid in enumerate(ids):
        assert np.array_equal(shown[k], before[k]["IM"])
        assert_session(s.read(sid), want[k], tag=(arch, "commit", k))
    # sample (NPE.py:317-327) with the caller's z: RECON, ERROR against IM, mode sample
    z2 = O.make_latents(3, seed=33)
    shown = s.sample(ids, z2)
    rec = m.sample_at_uint8(z2)
    assert np.array_equal(shown, rec)
    for k, sid in enumerate(ids):
        got = s.read(sid)
        assert got["MODE"] == 1 and np.array_equal(got["Z"], z2[k]) and np.array_equal(got["RECON"], rec[k])
        assert np.array_equal(got["ERROR"], N.to_tanh(np.float32(want[k]["IM"])) - N.to_tanh(np.float32(rec[k])))
        assert np.array_equal(got["IM"], want[k]["IM"])
    # paint_latents in sample mode: the plain sample
    shown = s.set_latent(ids, z)
    assert np.array_equal(shown, m.sample_at_uint8(z))
    # Reset (NPE.py:330-340): back to photo mode from the stored GIM
    shown = s.reset(ids)
    for k, sid in enumerate(ids):
        assert np.array_equal(shown[k], want[k]["GIM"])
        assert_session(s.read(sid), want[k], tag=(arch, "reset", k))


def replay_sessions(s, sid, fx, others=None):
    """tests/session_replay.replay with one session id carrying the events; others = (ids, rs): unrelated sessions that run unrelated
    events in the same calls, the fixture's session in position 3 of 5."""
    kinds = [str(k) for k in fx["kinds"]]
    out = []
    if others:
        oids, rs = others
        s.open(oids, rs.randint(0, 256, (len(oids), 3, 64, 64)).astype(np.uint8))
        order = oids[:3] + [sid] + oids[3:]
    for k, kind in enumerate(kinds):
        x1, y1, x2, y2, dsize, r, g, b, delta = [int(v) for v in fx["state"][k]]
        rec = {"kind": kind, "shown": None, "MASK": None}
        if kind in ("infer", "reset"):
            shown = s.open([sid], fx["GIM"][None]) if kind == "infer" else s.reset([sid])
            st = s.read(sid)
            rec.update(shown=shown[0], RECON=st["RECON"], ERROR=st["ERROR"])
        elif kind in ("paint", "scroll"):
            paint = kind == "paint"
            if others:
                n = len(order)
                c1, r1 = rs.randint(0, 50, n), rs.randint(0, 50, n)
                boxes = np.stack([c1, r1, c1 + rs.randint(1, 12, n), r1 + rs.randint(1, 12, n)], 1)
                modes = list(rs.randint(0, 2, n))
                colours = rs.randint(0, 256, (n, 3))
                weight, sign = np.full(n, 0.05), np.full(n, -1.0)
                boxes[3], modes[3], colours[3] = (x1, y1, x2, y2), int(paint), (r, g, b)
                weight[3], sign[3] = (0.05, -1.0) if paint else (0.1, float(np.sign(delta)))
                rec["shown"] = s.brush(order, boxes, colours, modes, weight, sign)[3]
            elif paint:
                rec["shown"] = s.paint([sid], (x1, y1, x2, y2), (r, g, b))[0]
            else:
                rec["shown"] = s.scroll([sid], (x1, y1, x2, y2), float(np.sign(delta)))[0]
        rec["Z"] = s.read(sid)["Z"].reshape(10, 10)
        out.append(rec)
    return out


@pytest.mark.parametrize("batched", [False, True])
def test_reference_executed_session_through_sessions(batched):
    """The reference-executed NPE.py session (infer, 6 paints, 3 scrolls, Reset) through EditSessions with one session id, alone and
    as session 3 of a batch of 5 whose other sessions run unrelated events; the bars of the stateless replay test."""
    from session_replay import compare
    fx = np.load(os.path.join(ROOT, "tests", "golden", "ref_session_IAN_simple.npz"))
    _, s = model_for("IAN_simple")
    others = ([1, 4, 6, 9], np.random.RandomState(9)) if batched else None
    events = replay_sessions(s, 14, fx, others)
    assert [e["kind"] for e in events].count("paint") == 6 and [e["kind"] for e in events].count("scroll") == 3
    worst = compare(events, fx, tol=1e-4, max_off_by_one_frac=2e-3)
    print("session replay (batched=%s): %s" % (batched, worst))


@pytest.mark.parametrize("arch", O.ARCHS)
def test_failures_name_the_item_and_leave_state_alone(arch):
    from neural_photo_editor_amd.lib import SessionEvent
    m, s = model_for(arch)
    h = m.handle
    ids = [0, 1, 2]                          # session 15 is opened by no test of this module
    s.open(ids, photos(3, 55))
    s.paint(ids, (10, 10, 20, 20), (200, 100, 50))
    before = [s.read(i) for i in ids]
    z = O.make_latents(2, seed=3)
    shown = np.full((2, 3, 64, 64), 7, np.uint8)

    i32 = lambda v: np.asarray(v, np.int32)
    bad = [
        ("item 1", lambda: h.session_brush(events([0, CAP]), shown)),                      # an id outside the pool
        ("item 1", lambda: h.session_brush(events([0, -1]), shown)),
        ("item 1", lambda: h.session_brush(events([0, 15]), shown)),                       # an unopened session: brush
        ("item 0", lambda: h.session_set_latent(i32([15, 0]), z, 1, shown)),               # ... set_latent
        ("item 1", lambda: h.session_open(i32([0, 15]), None, 0, shown)),                  # ... re-open from stored state
        ("item 1", lambda: h.session_open(i32([0, 15]), None, 1, shown)),
        ("item 1", lambda: h.session_brush(events([1, 1]), shown)),                        # the same session twice
        ("item 1", lambda: h.session_set_latent(i32([2, 2]), z, 0, shown)),
        ("item 1", lambda: h.session_open(i32([2, 2]), photos(2, 1), 0, shown)),
        ("item 0", lambda: h.session_brush(events([0, 1], box=(10, 10, 65, 20)), shown)),  # a rectangle outside the image
        ("item 0", lambda: h.session_brush(events([0, 1], box=(-1, 10, 5, 20)), shown)),
        ("item 0", lambda: h.session_brush(events([0, 1], mode=2), shown)),                # a mode outside {0,1}
        ("n = 0", lambda: h.session_brush((SessionEvent * 0)(), shown)),                   # n outside 1..256
        ("n = 257", lambda: h.session_brush(events(list(range(257))), None)),
        ("n = 257", lambda: h.session_open(i32(np.arange(257)), None, 0, None)),
    ]
    for needle, call in bad:
        refused(call, needle, -7)
        assert np.all(shown == 7)
        for i, b in zip(ids, before):
            assert_session(s.read(i), b, tag=needle)
    # the Python surface refuses the same before the library is called
    with pytest.raises(ValueError):
        s.paint([0, 15], (0, 0, 4, 4), (1, 2, 3))
    # the handle still works
    s.paint(ids, (10, 10, 20, 20), (200, 100, 50))
    assert any((s.read(i)["Z"] != b["Z"]).any() for i, b in zip(ids, before))


@pytest.mark.parametrize("arch", O.ARCHS)
def test_handle_survives_session_calls_and_pool_growth(arch):
    m, s = model_for(arch)
    z1 = O.make_latents(1, seed=61)
    rgb1 = np.random.RandomState(62).uniform(-1, 1, (1, 3, 64, 64)).astype(np.float32)
    zb = O.make_latents(4, seed=63)
    rgbb = np.random.RandomState(64).uniform(-1, 1, (4, 3, 64, 64)).astype(np.float32)
    boxes = np.array([(26, 26, 30, 30), (0, 0, 16, 16), (40, 10, 60, 12), (5, 50, 9, 64)])

    def stateless():
        a = m.brush_step(20, 20, 40, 40, z1, RGB=rgb1)
        b = m.brush_step_batch(boxes, zb, rgbb)
        return list(a) + list(b)

    first = stateless()
    ids = [5, 10]
    s.open(ids, photos(2, 65))
    s.paint(ids, (8, 8, 24, 24), (10, 200, 30))
    s.scroll(ids, (8, 8, 24, 24), 1.0)
    for a, b in zip(first, stateless()):
        assert np.array_equal(a, b)
    # growing the pool keeps the sessions; a brush right after it sees the moved rows
    before = [s.read(i) for i in ids]
    try:
        s.reserve(4096)
        for i, b in zip(ids, before):
            assert_session(s.read(i), b, tag=(arch, "grown", i))
        s.open([4095], photos(1, 66))
        s.paint([4095, 5], (8, 8, 24, 24), (10, 200, 30))
        assert (s.read(5)["Z"] != before[0]["Z"]).any() and np.array_equal(s.read(10)["Z"], before[1]["Z"])
    finally:
        s.reserve(CAP)
    assert_session(s.read(10), before[1], tag=(arch, "shrunk"))
    for a, b in zip(first, stateless()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("arch", O.ARCHS)
def test_several_passes_equal_the_stateless_call(arch):
    """Option brush_pass below n splits a call into passes (items 0..2, 3..5, 6) in the session path as in ian_brush_step_batch:
    bitwise the stateless call under the same option, twice in a row (no residency across passes)."""
    m, s = model_for(arch)
    ids = [0, 2, 5, 7, 8, 11, 13]
    ph = photos(7, 91)
    rs = np.random.RandomState(92)
    c1, r1 = rs.randint(0, 50, 7), rs.randint(0, 50, 7)
    boxes = np.stack([c1, r1, c1 + rs.randint(1, 12, 7), r1 + rs.randint(1, 12, 7)], 1)
    colours, modes = rs.randint(0, 256, (7, 3)), [1, 0, 1, 1, 0, 1, 1]
    weight, sign = np.full(7, 0.05), np.full(7, -1.0)
    m.handle.set_option("brush_pass", 3)
    try:
        M = dict(zip(ids, host_open(m, ph)))
        want = [model_brush(m, M, ids, boxes, colours, modes, weight, sign) for _ in range(2)]
        s.open(ids, ph)
        got = [s.brush(ids, boxes, colours, modes, weight, sign) for _ in range(2)]
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        for i in ids:
            assert_session(s.read(i), M[i], tag=(arch, i))
    finally:
        m.handle.set_option("brush_pass", 256)

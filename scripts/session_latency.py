"""Device-resident edit sessions against the stateless batched call: events/s of EditSessions.paint (photo mode, a steady set of
ids: state in HBM, 11 words up per event, 12 KB down) and of IAN.brush_step_batch with host pointers and photo= (per item a 48 KB
colour image, RECON, ERROR and the latent compared against their shadows, z_new and IM down), in one process, on both configs.
usage (GPU box): python scripts/session_latency.py [--only IAN_simple] [--n 1 4 16 64] [--calls 200] [--repeats 3] [--out FILE] [--local]
                                                    [--history] [--tip D [--local [--footprint]]]
  --local: the same event stream on a pool with the local reservation and flags 3 (user mask + dampen) on every session: per item
           the blend also reads, max-es and writes the session's 32 KB UMASK.  Compare against a run without --local in the same
           process order on the same build.
  --history: the undo history instead of the comparison with the stateless call, sessions only, depth 16:
           mark_paint_undo  one iteration = mark, paint, undo (three calls; events/s counts iterations)
           undo             one ian_session_undo per call, undo and redo alternating on a marked stroke
           set_latent       the same sessions' latents through set_latent (host z): what an undo should cost, less one small launch
           paint_unused_history  paint in the pool with the history reserved but never marked, to hold against paint without --history
  --tip D: brush tips instead of the comparison with the stateless call, sessions only: what a tip costs.
           rectangle  D x D paint events through ian_session_brush
           tip        the same events with npe_ops.round_tip(D, 0.5) through ian_session_brush_tip
           alternating within a repeat; n defaults to 1 16 64, --out to profiles/session_tip_latency.json.  With --trace: both, one after
           the other, for a kernel trace (the two seed kernels are different instantiations and show as two rows).
           With --local the pool has the local reservation and LOCAL bit 0 on every session (the blend max-es the event's footprint into
           UMASK); with --footprint as well two more paths: tip_footprint, the tip events under
           EditSessions.tip_footprint(True), whose footprint is session_tip_umask_kernel's, and a stroke of 64 points with the tip per
           session, setting off and on (stroke_tip, stroke_tip_footprint; a tenth of --calls).  --out defaults to
           profiles/session_soft_mask_latency_D<D>.json then.
  --trace: only the first --n on the first config, sessions only: warm-up, an idle second, then --calls timed calls (for a
           rocprofv3 --kernel-trace --stats run).
Per (config, n, path): the median over --calls calls after warm-up, repeated --repeats times (the two paths alternate within a
repeat); reported are the median of the repeats and their spread (max - min) / median.  Also the host<->device bytes per call of
both paths.  Prints one JSON line and, with --out, writes it there."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_photo_editor_amd import IAN, synthetic as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = 3 * 64 * 64


def boxes_for(n, seed=0):
    rs = np.random.RandomState(seed)
    c1, r1 = rs.randint(0, 56, n), rs.randint(0, 56, n)
    return np.stack([c1, r1, c1 + 4 + rs.randint(0, 5, n), r1 + 4 + rs.randint(0, 5, n)], 1)   # NPE brush boxes: 4..8 pixels


def median_ms(fn, calls, warmup=10):
    for _ in range(warmup):
        fn()
    lat = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        lat.append((time.perf_counter() - t) * 1e3)
    return float(np.median(lat))


def bytes_per_call(n, zl):
    """What crosses the bus per call.  Stateless, steady state: the item table and the latents go up (the latents change every
    call; the colour images, RECON and ERROR are re-uploaded only when their bytes change, but all of them are compared on the
    host every call), z_new and IM come down."""
    return {"sessions": {"h2d": 44 * n, "d2h": IMG * n, "host_compare": 0},
            "stateless": {"h2d": 28 * n + 4 * zl * n, "d2h": 4 * zl * n + IMG * n, "host_compare": n * (4 * IMG + IMG + 4 * IMG)}}


def run_arch(arch, ns, calls, repeats, local=False):
    from neural_photo_editor_amd import npe_ops as N
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))
    zl = m.get_zdim()
    s = m.sessions(max(ns))
    if local:
        s.reserve_local()
    rows = []
    for n in ns:
        ids = np.arange(n)
        boxes = boxes_for(n)
        levels = (255, 0, 0)
        ph = np.random.RandomState(n).randint(0, 256, (n, 3, 64, 64)).astype(np.uint8)
        s.open(ids, ph)
        if local:
            s.set_local(ids, flags=3)
        st = [s.read(i) for i in ids]
        recon, error = np.stack([t["RECON"] for t in st]), np.stack([t["ERROR"] for t in st])
        z = [np.stack([t["Z"] for t in st])]
        rgb = np.empty((n, 3, 64, 64), np.float32)
        rgb[:] = N.to_tanh(np.float32(levels)).astype(np.float32)[None, :, None, None]

        def sess():
            s.paint(ids, boxes, levels)

        def stateless():
            z[0] = m.brush_step_batch(boxes, z[0], rgb, image=False, photo=(recon, error))[0]
        res = {"sessions": [], "stateless": []}
        for _ in range(repeats):
            res["sessions"].append(median_ms(sess, calls))
            res["stateless"].append(median_ms(stateless, calls))
        row = {"n": n, "bytes_per_call": bytes_per_call(n, zl)}
        for k, v in res.items():
            med = float(np.median(v))
            row[k] = {"p50_ms": round(med, 4), "events_per_s": round(n * 1e3 / med, 1), "spread": round((max(v) - min(v)) / med, 4),
                      "repeats_ms": [round(t, 4) for t in v]}
        row["sessions_over_stateless"] = round(row["sessions"]["events_per_s"] / row["stateless"]["events_per_s"], 3)
        rows.append(row)
    m.close()
    return rows


def run_history(arch, ns, calls, repeats, depth=16):
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))
    s = m.sessions(max(ns))
    s.reserve_history(depth)
    rows = []
    for n in ns:
        ids = np.arange(n)
        boxes = boxes_for(n)
        levels = (255, 0, 0)
        s.open(ids, np.random.RandomState(n).randint(0, 256, (n, 3, 64, 64)).astype(np.uint8))
        z = np.stack([s.read(i)["Z"] for i in ids])
        back = [True]

        def paint_unused():
            s.paint(ids, boxes, levels)

        def mark_paint_undo():
            s.mark(ids)
            s.paint(ids, boxes, levels)
            s.undo(ids)

        def undo():
            (s.undo if back[0] else s.redo)(ids)
            back[0] = not back[0]

        def set_latent():
            s.set_latent(ids, z)
        res = {"paint_unused_history": [], "mark_paint_undo": [], "undo": [], "set_latent": []}
        for _ in range(repeats):
            res["paint_unused_history"].append(median_ms(paint_unused, calls))      # first: nothing has been marked yet
        for _ in range(repeats):
            res["mark_paint_undo"].append(median_ms(mark_paint_undo, calls))
            s.mark(ids)
            s.paint(ids, boxes, levels)
            back[0] = True
            res["undo"].append(median_ms(undo, 2 * (calls // 2), warmup=10))         # an even number of calls: ends where it began
            res["set_latent"].append(median_ms(set_latent, calls))
        row = {"n": n, "depth": depth, "ring_bytes_per_session": (depth + 1) * 4 * m.get_zdim()}
        for k, v in res.items():
            med = float(np.median(v))
            row[k] = {"p50_ms": round(med, 4), "events_per_s": round(n * 1e3 / med, 1), "spread": round((max(v) - min(v)) / med, 4),
                      "repeats_ms": [round(t, 4) for t in v]}
        row["undo_over_set_latent"] = round(row["undo"]["p50_ms"] / row["set_latent"]["p50_ms"], 3)
        rows.append(row)
    m.close()
    return rows


def tip_boxes(n, D, seed=0):
    rs = np.random.RandomState(seed)
    c1, r1 = rs.randint(0, 64 - D + 1, n), rs.randint(0, 64 - D + 1, n)
    return np.stack([c1, r1, c1 + D, r1 + D], 1)


def tip_pool(arch, cap, D):
    from neural_photo_editor_amd import npe_ops as N
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))
    s = m.sessions(cap)
    s.reserve_tips(1)
    s.set_tip(0, N.round_tip(D, 0.5))
    return m, s


def run_tip(arch, ns, calls, repeats, D, local=False, footprint=False):
    m, s = tip_pool(arch, max(ns), D)
    if local:
        s.reserve_local()
    rows = []
    for n in ns:
        ids, boxes, levels = np.arange(n), tip_boxes(n, D), (255, 0, 0)
        s.open(ids, np.random.RandomState(n).randint(0, 256, (n, 3, 64, 64)).astype(np.uint8))
        if local:
            s.set_local(ids, flags=1)
        paths = [tip_boxes(64, D, seed=100 + i) for i in range(n)]          # a drag of 64 points per session

        def rectangle():
            s.paint(ids, boxes, levels)

        def tip():
            s.paint(ids, boxes, levels, tips=0)

        def stroke_tip():
            s.stroke(ids, paths, levels, None, 0.01, -1.0, tips=0)
        res = {"rectangle": [], "tip": []}
        if footprint:
            res.update({"tip_footprint": [], "stroke_tip": [], "stroke_tip_footprint": []})
        for _ in range(repeats):
            res["rectangle"].append(median_ms(rectangle, calls))
            res["tip"].append(median_ms(tip, calls))
            if footprint:                                                      # the setting synchronises: switched outside the timed calls
                res["stroke_tip"].append(median_ms(stroke_tip, max(calls // 10, 3), warmup=2))
                s.tip_footprint(True)
                res["tip_footprint"].append(median_ms(tip, calls))
                res["stroke_tip_footprint"].append(median_ms(stroke_tip, max(calls // 10, 3), warmup=2))
                s.tip_footprint(False)
        row = {"n": n, "D": D}
        for k, v in res.items():
            med = float(np.median(v))
            row[k] = {"p50_ms": round(med, 4), "events_per_s": round(n * 1e3 / med, 1), "spread": round((max(v) - min(v)) / med, 4),
                      "repeats_ms": [round(t, 4) for t in v]}
        row["tip_over_rectangle"] = round(row["tip"]["p50_ms"] / row["rectangle"]["p50_ms"], 4)
        row["tip_inside_rectangle_repeats"] = bool(min(res["rectangle"]) <= row["tip"]["p50_ms"] <= max(res["rectangle"]))
        if footprint:
            row["footprint_over_tip"] = round(row["tip_footprint"]["p50_ms"] / row["tip"]["p50_ms"], 4)
            row["stroke_footprint_over_stroke"] = round(row["stroke_tip_footprint"]["p50_ms"] / row["stroke_tip"]["p50_ms"], 4)
        rows.append(row)
    m.close()
    return rows


def trace_tip(arch, n, calls, D):
    m, s = tip_pool(arch, n, D)
    ids, boxes, levels = np.arange(n), tip_boxes(n, D), (255, 0, 0)
    s.open(ids, np.random.RandomState(n).randint(0, 256, (n, 3, 64, 64)).astype(np.uint8))
    out = {"arch": arch, "n": n, "calls": calls, "D": D}
    for name, kw in (("rectangle", {}), ("tip", {"tips": 0})):
        for _ in range(5):
            s.paint(ids, boxes, levels, **kw)
        t = time.perf_counter()
        for _ in range(calls):
            s.paint(ids, boxes, levels, **kw)
        out[name + "_ms_per_call"] = round((time.perf_counter() - t) * 1e3 / calls, 4)
    return out


def trace_run(arch, n, calls, local=False):
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))
    s = m.sessions(n)
    ids, boxes = np.arange(n), boxes_for(n)
    s.open(ids, np.random.RandomState(n).randint(0, 256, (n, 3, 64, 64)).astype(np.uint8))
    if local:
        s.reserve_local()
        s.set_local(ids, flags=3)
    for _ in range(5):
        s.paint(ids, boxes, (255, 0, 0))
    time.sleep(1.0)
    t = time.perf_counter()
    for _ in range(calls):
        s.paint(ids, boxes, (255, 0, 0))
    return {"arch": arch, "n": n, "calls": calls, "local": bool(local), "ms_per_call": round((time.perf_counter() - t) * 1e3 / calls, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="one config (IAN_simple or IAN)")
    ap.add_argument("--n", type=int, nargs="*", default=None, help="default 1 4 16 64; with --tip 1 16 64")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--local", action="store_true", help="local reservation, flags 3 (user mask + dampen) on every session")
    ap.add_argument("--history", action="store_true", help="undo history: mark + paint + undo, undo alone, set_latent, paint with an unused history")
    ap.add_argument("--tip", type=int, default=0, metavar="D", help="brush tips: D x D rectangle events against the same events with round_tip(D, 0.5)")
    ap.add_argument("--footprint", action="store_true", help="with --tip D --local: also the tip events and a 64-point stroke under tip_footprint(True)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    archs = [a.only] if a.only else ["IAN_simple", "IAN"]
    if a.tip and not 1 <= a.tip <= 64:
        ap.error("--tip D: a tip has 1..64 pixels a side")
    if a.footprint and not (a.tip and a.local):
        ap.error("--footprint goes with --tip D --local")
    if a.n is None:
        a.n = [1, 16, 64] if a.tip else [1, 4, 16, 64]
    if a.tip and a.trace:
        print(json.dumps(trace_tip(archs[0], a.n[0], a.calls, a.tip)))
        return
    if a.tip:
        res = {"metric": "session_soft_mask_latency" if a.footprint else "session_tip_latency", "calls": a.calls, "repeats": a.repeats, "D": a.tip,
               "local": bool(a.local)}
        for arch in archs:
            res[arch] = run_tip(arch, a.n, a.calls, a.repeats, a.tip, a.local, a.footprint)
        print(json.dumps(res))
        default = ("session_soft_mask_latency_D%d.json" % a.tip) if a.footprint else "session_tip_latency.json"
        with open(a.out or os.path.join(ROOT, "profiles", default), "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        return
    if a.trace:
        print(json.dumps(trace_run(archs[0], a.n[0], a.calls, a.local)))
        return
    res = {"metric": "session_history_latency" if a.history else "session_latency", "calls": a.calls, "repeats": a.repeats, "local": bool(a.local)}
    for arch in archs:
        res[arch] = run_history(arch, a.n, a.calls, a.repeats) if a.history else run_arch(arch, a.n, a.calls, a.repeats, a.local)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

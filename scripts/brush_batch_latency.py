"""Several editors on one device: events/s and p50 latency of ian_brush_step_batch (gradient + update + decoder [+ photo blend]
for n sessions in one call) against the batch-1 ian_brush_step loop, on both configs.  Prints one JSON line.
usage (GPU box): python scripts/brush_batch_latency.py [--tune] [--only IAN_simple] [--n 64] [--events 30]
  --tune: ian_autotune the forward at each n first (the batch-1 loop is tuned as in scripts/edit_latency.py either way).
  --trace: only the first --n on the first config, no batch-1 loop: warm-up, an idle second, then --events timed calls (the
           layout scripts/summarize_brush_batch_trace.py expects under rocprofv3 --kernel-trace).
Each batched call continues the sessions of the previous one (z = the z_new it returned); "cache" says whether the
resident-activation cache can skip the forward at z (n <= the handle's brush_pass); "cold" repeats the largest n with
IAN_NO_DEC_CACHE=1."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_photo_editor_amd import IAN, synthetic as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def boxes_for(n, seed=0):
    rs = np.random.RandomState(seed)
    c1, r1 = rs.randint(0, 56, n), rs.randint(0, 56, n)
    return np.stack([c1, r1, c1 + 4 + rs.randint(0, 5, n), r1 + 4 + rs.randint(0, 5, n)], 1)   # NPE brush boxes: 4..8 pixels


def timed(fn, events, warmup=5):
    for _ in range(warmup):
        fn()
    lat = []
    for _ in range(events):
        t = time.perf_counter()
        fn()
        lat.append((time.perf_counter() - t) * 1e3)
    return float(np.percentile(lat, 50))


PASS = 256   # the handle's default brush_pass (items per forward / backward / forward pass)


def new_model(arch):
    return IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))


def trace_run(arch, n, events):
    m = new_model(arch)
    boxes, rgb, z = boxes_for(n), np.full((n, 3, 64, 64), -1.0, np.float32), [O.make_latents(n, seed=4)]
    rgb[:, 0] = 1.0

    def step():
        z[0] = m.brush_step_batch(boxes, z[0], rgb)[0]
    for _ in range(5):
        step()
    time.sleep(1.0)                      # host outputs: each call has synchronised; this idle gap is where the summariser cuts
    t = time.perf_counter()
    for _ in range(events):
        step()
    return {"arch": arch, "n": n, "events": events, "ms_per_call": round((time.perf_counter() - t) * 1e3 / events, 4)}


def run_arch(arch, ns, events, tune):
    m = new_model(arch)
    rgb1 = np.full((1, 3, 64, 64), -1.0, np.float32)
    rgb1[:, 0] = 1.0
    z1 = [O.make_latents(1, seed=2)]
    m.reconstruct(O.make_images(1, seed=0))
    m.imgradRGB(26, 26, 30, 30, rgb1, z1[0])
    m.handle.autotune(1, 3)

    def b1():
        z1[0], _ = m.brush_step(26, 26, 30, 30, z1[0], RGB=rgb1, weight=0.05)
    p50 = timed(b1, 200, warmup=50)
    out = {"batch1_loop": {"p50_ms": round(p50, 4), "events_per_s": round(1e3 / p50, 1)}, "batched": []}
    for n in ns:
        if tune:
            m.sample_at(O.make_latents(n, seed=3))
            m.handle.autotune(n, 1)
        boxes = boxes_for(n)
        rgb = np.repeat(rgb1, n, 0)
        rs = np.random.RandomState(n)
        photo = (rs.randint(0, 256, (n, 3, 64, 64)).astype(np.uint8), rs.uniform(-0.1, 0.1, (n, 3, 64, 64)).astype(np.float32))
        for ph in (False, True):
            z = [O.make_latents(n, seed=4)]

            def step():
                r = m.brush_step_batch(boxes, z[0], rgb, photo=photo if ph else None)
                z[0] = r[0]
            p50 = timed(step, events)
            out["batched"].append({"n": n, "photo": ph, "cache": n <= PASS, "p50_ms": round(p50, 4), "events_per_s": round(n * 1e3 / p50, 1)})
        if n == max(ns):
            os.environ["IAN_NO_DEC_CACHE"] = "1"
            try:
                z = [O.make_latents(n, seed=4)]

                def cold():
                    z[0] = m.brush_step_batch(boxes, z[0], rgb)[0]
                p50 = timed(cold, events)
            finally:
                del os.environ["IAN_NO_DEC_CACHE"]
            out["batched"].append({"n": n, "photo": False, "cache": False, "p50_ms": round(p50, 4),
                                   "events_per_s": round(n * 1e3 / p50, 1)})
    best = max(r["events_per_s"] for r in out["batched"] if r["n"] == max(ns) and not r["photo"])
    out["speedup_vs_batch1_loop_at_n%d" % max(ns)] = round(best / out["batch1_loop"]["events_per_s"], 2)
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="one config (IAN_simple or IAN)")
    ap.add_argument("--n", type=int, nargs="*", default=[1, 4, 16, 64])
    ap.add_argument("--events", type=int, default=30)
    ap.add_argument("--tune", action="store_true")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    archs = [a.only] if a.only else ["IAN_simple", "IAN"]
    if a.trace:
        print(json.dumps(trace_run(archs[0], a.n[0], a.events)))
        return
    res = {"metric": "brush_batch_latency", "tuned_forward": a.tune}
    for arch in archs:
        res[arch] = run_arch(arch, a.n, a.events, a.tune)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Full-resolution edit sessions: what a window costs.  Per scale s in --scales and n in --n sessions, for a 256 x 256 window and the
whole S x S picture (S = 64 s):
  render_device   ian_session_render into a DEVICE buffer, --calls calls back to back and one device synchronisation: microseconds per
                  call and achieved GB/s against the bytes the kernel has to move, 2 * 3 * vw * vh per view (one uchar4 load of SRC and
                  one uchar4 store per lane; the staged field rows are noise next to that);
  render_host     EditSessions.render (host result: the same plus the device -> host copy of 3 * vw * vh bytes per view), median;
  brush / brush_view   EditSessions.paint without and with view=: the price of the window inside the event's submission, medians.
usage (GPU box): python scripts/session_hires_latency.py [--scales 4 16] [--n 1 16] [--calls 200] [--repeats 3] [--out FILE]
--guided: the same cases, render_device only, with the guide of ian_sessions_reserve_guide (--sigma, default 8) on and off in the
same run, alternating per repeat: the edge-aware kernel against the bilinear one, which moves the same bytes.
Medians over --calls calls after warm-up, repeated --repeats times; reported are the median of the repeats and their spread
(max - min) / median.  Prints one JSON line and, with --out, writes it there."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_photo_editor_amd import IAN, api, synthetic as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def render_bytes(n, vw, vh):
    """Device bytes of one render call at kind 0: SRC read once, the window written once."""
    return 2 * 3 * vw * vh * n


def median_us(fn, calls, warmup=10):
    for _ in range(warmup):
        fn()
    lat = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        lat.append((time.perf_counter() - t) * 1e6)
    return float(np.median(lat))


def stat(v):
    med = float(np.median(v))
    return {"p50_us": round(med, 2), "spread": round((max(v) - min(v)) / med, 4), "repeats_us": [round(t, 2) for t in v]}


def run(arch, scales, ns, calls, repeats):
    import torch
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))
    s = m.sessions(max(ns))
    rows = []
    for scale in scales:
        s.reserve_hires(scale)
        S = 64 * scale
        for n in ns:
            ids = np.arange(n)
            rs = np.random.RandomState(n)
            s.open_hires(ids, rs.randint(0, 256, (n, 3, S, S)).astype(np.uint8))
            c1, r1 = rs.randint(0, 56, n), rs.randint(0, 56, n)
            boxes = np.stack([c1, r1, c1 + 4 + rs.randint(0, 5, n), r1 + 4 + rs.randint(0, 5, n)], 1)
            s.paint(ids, boxes, (255, 0, 0))                            # FIELD_KIND 0 with a non-zero field: the photo path
            for vw in sorted({min(256, S), S}):
                vh = vw
                origin = ((S - vw) // 8 * 4, (S - vh) // 2)
                views, _, _ = api.pack_session_views(ids, origin, (vw, vh), scale)
                d_out = torch.empty((n, 3, vh, vw), dtype=torch.uint8, device="cuda")

                def device_calls():
                    for _ in range(calls):
                        m.handle.session_render(views, vw, vh, d_out)
                    torch.cuda.synchronize()

                dev = []
                for _ in range(repeats):
                    device_calls()
                    t = time.perf_counter()
                    device_calls()
                    dev.append((time.perf_counter() - t) * 1e6 / calls)
                res = {"render_host": [], "brush": [], "brush_view": []}
                for _ in range(repeats):
                    res["render_host"].append(median_us(lambda: s.render(ids, origin, (vw, vh)), calls))
                    res["brush"].append(median_us(lambda: s.paint(ids, boxes, (255, 0, 0)), calls))
                    res["brush_view"].append(median_us(lambda: s.paint(ids, boxes, (255, 0, 0), view=(origin, (vw, vh))), calls))
                row = {"scale": scale, "n": n, "window": [vw, vh], "device_bytes": render_bytes(n, vw, vh), "d2h_bytes": 3 * vw * vh * n,
                       "render_device": stat(dev)}
                row["render_device"]["GBps"] = round(render_bytes(n, vw, vh) / (row["render_device"]["p50_us"] * 1e-6) / 1e9, 1)
                for k, v in res.items():
                    row[k] = stat(v)
                row["view_adds_us"] = round(row["brush_view"]["p50_us"] - row["brush"]["p50_us"], 2)
                rows.append(row)
    m.close()
    return rows


def run_guided(arch, scales, ns, calls, repeats, sigma):
    """Per case: ian_session_render into a device buffer, --calls calls back to back and one device synchronisation, with the guide
    off (session_render_kernel<false>) and on (session_render_kernel<true>), off / on / off / on ... so that drift hits both alike."""
    import torch
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))
    s = m.sessions(max(ns))
    rows = []
    for scale in scales:
        s.reserve_guide()
        s.reserve_hires(scale)
        S = 64 * scale
        for n in ns:
            ids = np.arange(n)
            rs = np.random.RandomState(n)
            s.open_hires(ids, rs.randint(0, 256, (n, 3, S, S)).astype(np.uint8))
            c1, r1 = rs.randint(0, 56, n), rs.randint(0, 56, n)
            boxes = np.stack([c1, r1, c1 + 4 + rs.randint(0, 5, n), r1 + 4 + rs.randint(0, 5, n)], 1)
            s.paint(ids, boxes, (255, 0, 0))                            # FIELD_KIND 0 with a non-zero field: the photo path
            for vw in sorted({min(256, S), S}):
                vh = vw
                origin = ((S - vw) // 8 * 4, (S - vh) // 2)
                views, _, _ = api.pack_session_views(ids, origin, (vw, vh), scale)
                d_out = torch.empty((n, 3, vh, vw), dtype=torch.uint8, device="cuda")

                def device_calls():
                    for _ in range(calls):
                        m.handle.session_render(views, vw, vh, d_out)
                    torch.cuda.synchronize()

                t_us = {"bilinear": [], "guided": []}
                for _ in range(repeats):
                    for name in ("bilinear", "guided"):
                        s.reserve_guide(sigma if name == "guided" else None)
                        device_calls()
                        t = time.perf_counter()
                        device_calls()
                        t_us[name].append((time.perf_counter() - t) * 1e6 / calls)
                s.reserve_guide()
                row = {"scale": scale, "n": n, "window": [vw, vh], "device_bytes": render_bytes(n, vw, vh)}
                for name, v in t_us.items():
                    row[name] = stat(v)
                    row[name]["GBps"] = round(render_bytes(n, vw, vh) / (row[name]["p50_us"] * 1e-6) / 1e9, 1)
                row["guided_over_bilinear"] = round(row["guided"]["p50_us"] / row["bilinear"]["p50_us"], 3)
                rows.append(row)
    m.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="IAN_simple")
    ap.add_argument("--scales", type=int, nargs="*", default=[4, 16])
    ap.add_argument("--n", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--guided", action="store_true", help="the guided render against the bilinear one, both into a device buffer")
    ap.add_argument("--sigma", type=float, default=8.0, help="--guided: the range sigma, in levels per channel")
    a = ap.parse_args()
    if a.guided:
        res = {"metric": "session_hires_guided_latency", "arch": a.arch, "calls": a.calls, "repeats": a.repeats, "sigma": a.sigma,
               "rows": run_guided(a.arch, a.scales, a.n, a.calls, a.repeats, a.sigma)}
    else:
        res = {"metric": "session_hires_latency", "arch": a.arch, "calls": a.calls, "repeats": a.repeats,
               "rows": run(a.arch, a.scales, a.n, a.calls, a.repeats)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

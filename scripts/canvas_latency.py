"""Canvases: what a composed window costs.  On a 2048 x 1536 canvas with 1 and 8 placed sessions (scale 4, overlapping in a row, every
one painted: kind 0 with a non-zero field), for a 256 x 256 window inside the squares and for the whole canvas:
  compose_device  ian_canvas_compose into a DEVICE buffer, --calls calls back to back and one device synchronisation: microseconds per
                  call and achieved GB/s against the bytes the kernel has to move, 2 * 3 * vw * vh (one uchar4 load of the canvas and
                  one uchar4 store per lane; the staged field rows are noise next to that);
  compose_host    EditSessions.compose (host result: the same plus the device -> host copy of 3 * vw * vh bytes), median;
  brush / brush_compose   EditSessions.paint of one placed session without and with the window: the price of the window inside the
                  event's submission, medians.
The one comparison with something older (`against_render`): one placement at scale 16 and feather 0 composed over a 1024 x 1024 window,
against ian_session_render of a 1024 x 1024 picture (scale 16) in the same run, both into device buffers, alternating: the two move
the same bytes.
--guided measures the edge-aware compose (ian_sessions_reserve_edges) instead: the same four rows, device buffers only,
plain and guided compose alternating per repeat in one run (the table is switched between the bursts, outside the timing), the
ratio guided / plain per row; and the comparison above with the guide on both sides: the guided compose of the scale-16 placement
against ian_session_render under ian_sessions_reserve_guide with the same table on a second pool (a pool has a guide or canvases).
--oriented measures the compose over oriented placements (ian_place_oriented): two canvases with the same photo, one
with 1 / 8 upright squares of 256 pixels (scale 4), one with 1 / 8 squares of side 256 at 23 degrees around the same centres, every
session painted; the same two windows, device buffers only, the aligned and the oriented compose alternating per repeat in one run,
and the ratio oriented / aligned per row.
usage (GPU box): python scripts/canvas_latency.py [--guided | --oriented] [--calls 200] [--repeats 3] [--out FILE]
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
CW, CH = 2048, 1536


def compose_bytes(n, vw, vh):
    """Device bytes of one compose call: the canvas read once, the window written once."""
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


def device_us(call, calls, repeats):
    """`call` enqueues one launch into a device buffer: microseconds per call over `calls` calls and one synchronisation."""
    import torch

    def burst():
        for _ in range(calls):
            call()
        torch.cuda.synchronize()

    out = []
    for _ in range(repeats):
        burst()
        t = time.perf_counter()
        burst()
        out.append((time.perf_counter() - t) * 1e6 / calls)
    return out


def run(arch, calls, repeats):
    import torch
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))
    s = m.sessions(16)
    s.reserve_hires(16)
    rs = np.random.RandomState(0)
    rows = []
    s.reserve_canvases(1, CW, CH, 4)
    photo = rs.randint(0, 256, (3, CH, CW)).astype(np.uint8)
    for placed in (1, 8):
        s.canvas_put(0, photo)                                              # drops the placements of the round before
        ids = np.arange(placed)
        origins = [(301 + 200 * k, 403 + 40 * k) for k in range(placed)]       # squares of 256 pixels, neighbours overlap; ox % 4 = 1
        s.place(ids, 0, origins, 4)
        s.paint(ids, (20, 20, 44, 44), (255, 0, 0))
        box = (20, 20, 44, 44)
        for (vw, vh, origin) in ((256, 256, (400, 450)), (CW, CH, (0, 0))):
            win, _, _ = api.pack_canvas_windows([0], origin, (vw, vh), [(CW, CH)])
            d_out = torch.empty((1, 3, vh, vw), dtype=torch.uint8, device="cuda")
            dev = device_us(lambda: m.handle.canvas_compose(win, vw, vh, d_out), calls, repeats)
            res = {"compose_host": [], "brush": [], "brush_compose": []}
            for _ in range(repeats):
                res["compose_host"].append(median_us(lambda: s.compose([0], origin, (vw, vh)), calls))
                res["brush"].append(median_us(lambda: s.paint([0], box, (255, 0, 0)), calls))
                res["brush_compose"].append(median_us(
                    lambda: s.brush_compose([0], box, (255, 0, 0), windows=([0], origin, (vw, vh))), calls))
            row = {"placed": placed, "window": [vw, vh], "device_bytes": compose_bytes(1, vw, vh), "d2h_bytes": 3 * vw * vh,
                   "compose_device": stat(dev)}
            row["compose_device"]["GBps"] = round(compose_bytes(1, vw, vh) / (row["compose_device"]["p50_us"] * 1e-6) / 1e9, 1)
            for k, v in res.items():
                row[k] = stat(v)
            row["window_adds_us"] = round(row["brush_compose"]["p50_us"] - row["brush"]["p50_us"], 2)
            rows.append(row)
    # compose against render: the same 2 * 3 * 1024 * 1024 bytes
    s.reserve_canvases(1, CW, CH, 0)
    s.canvas_put(0, photo)
    s.place([0], 0, (512, 256), 16)
    s.open_hires([1], rs.randint(0, 256, (1, 3, 1024, 1024)).astype(np.uint8))
    s.paint([0, 1], (20, 20, 44, 44), (255, 0, 0))
    win, _, _ = api.pack_canvas_windows([0], (512, 256), 1024, [(CW, CH)])
    views, _, _ = api.pack_session_views([1], (0, 0), 1024, 16)
    d_out = torch.empty((1, 3, 1024, 1024), dtype=torch.uint8, device="cuda")
    comp, rend = [], []
    for _ in range(repeats):                                                # alternating: the two see the same machine
        comp += device_us(lambda: m.handle.canvas_compose(win, 1024, 1024, d_out), calls, 1)
        rend += device_us(lambda: m.handle.session_render(views, 1024, 1024, d_out), calls, 1)
    against = {"window": [1024, 1024], "device_bytes": compose_bytes(1, 1024, 1024), "compose_device": stat(comp), "render_device": stat(rend)}
    against["compose_over_render"] = round(against["compose_device"]["p50_us"] / against["render_device"]["p50_us"], 3)
    m.close()
    return rows, against


def run_guided(arch, calls, repeats, sigma=8.0):
    import torch
    from neural_photo_editor_amd import npe_ops
    cfg = os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py")
    m = IAN(cfg, True, params=O.make_params(arch, 1))
    s = m.sessions(16)
    s.reserve_hires(16)
    table = npe_ops.guide_table(sigma)
    rs = np.random.RandomState(0)
    photo = rs.randint(0, 256, (3, CH, CW)).astype(np.uint8)
    s.reserve_canvases(1, CW, CH, 4)

    def alternate(win, vw, vh, d_out, also=None):
        plain, guided, other = [], [], []
        for _ in range(repeats):                                            # alternating: all see the same machine
            s.reserve_canvas_guide()
            plain += device_us(lambda: m.handle.canvas_compose(win, vw, vh, d_out), calls, 1)
            s.reserve_canvas_guide(table=table)
            guided += device_us(lambda: m.handle.canvas_compose(win, vw, vh, d_out), calls, 1)
            if also:
                other += device_us(also, calls, 1)
        return plain, guided, other

    rows = []
    for placed in (1, 8):
        s.canvas_put(0, photo)
        ids = np.arange(placed)
        s.place(ids, 0, [(301 + 200 * k, 403 + 40 * k) for k in range(placed)], 4)
        s.paint(ids, (20, 20, 44, 44), (255, 0, 0))
        for (vw, vh, origin) in ((256, 256, (400, 450)), (CW, CH, (0, 0))):
            win, _, _ = api.pack_canvas_windows([0], origin, (vw, vh), [(CW, CH)])
            d_out = torch.empty((1, 3, vh, vw), dtype=torch.uint8, device="cuda")
            plain, guided, _ = alternate(win, vw, vh, d_out)
            row = {"placed": placed, "window": [vw, vh], "device_bytes": compose_bytes(1, vw, vh), "plain_device": stat(plain),
                   "guided_device": stat(guided)}
            row["guided_over_plain"] = round(row["guided_device"]["p50_us"] / row["plain_device"]["p50_us"], 3)
            rows.append(row)
    # one placement at scale 16, feather 0, a 1024 x 1024 window: plain and guided compose, and the guided render of a second pool
    s.reserve_canvases(1, CW, CH, 0)
    s.canvas_put(0, photo)
    s.place([0], 0, (512, 256), 16)
    s.paint([0], (20, 20, 44, 44), (255, 0, 0))
    m2 = IAN(cfg, True, params=O.make_params(arch, 1))
    r = m2.sessions(16)
    r.reserve_hires(16)
    r.reserve_guide(table=table)
    r.open_hires([1], np.ascontiguousarray(photo[None, :, 256:1280, 512:1536]))
    r.paint([1], (20, 20, 44, 44), (255, 0, 0))
    win, _, _ = api.pack_canvas_windows([0], (512, 256), 1024, [(CW, CH)])
    views, _, _ = api.pack_session_views([1], (0, 0), 1024, 16)
    d_out = torch.empty((1, 3, 1024, 1024), dtype=torch.uint8, device="cuda")
    d_ref = torch.empty((1, 3, 1024, 1024), dtype=torch.uint8, device="cuda")
    plain, guided, rend = alternate(win, 1024, 1024, d_out, lambda: m2.handle.session_render(views, 1024, 1024, d_ref))
    # the last bursts left the guided compose in d_out and the guided render in d_ref: the same bytes, so the same work
    against = {"window": [1024, 1024], "device_bytes": compose_bytes(1, 1024, 1024), "plain_device": stat(plain),
               "guided_device": stat(guided), "render_guided_device": stat(rend), "same_bytes": bool(torch.equal(d_out, d_ref))}
    against["guided_over_plain"] = round(against["guided_device"]["p50_us"] / against["plain_device"]["p50_us"], 3)
    against["guided_compose_over_guided_render"] = round(against["guided_device"]["p50_us"] / against["render_guided_device"]["p50_us"], 3)
    m.close()
    m2.close()
    return rows, against


def run_oriented(arch, calls, repeats, side=256.0, angle=23.0):
    import torch
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))
    s = m.sessions(16)
    s.reserve_hires(16)
    rs = np.random.RandomState(0)
    photo = rs.randint(0, 256, (3, CH, CW)).astype(np.uint8)
    s.reserve_canvases(2, CW, CH, 4)
    rows = []
    for placed in (1, 8):
        for cid in (0, 1):
            s.canvas_put(cid, photo)                                        # drops the placements of the round before
        origins = [(301 + 200 * k, 403 + 40 * k) for k in range(placed)]
        s.place(np.arange(placed), 0, origins, 4)
        s.place_oriented(8 + np.arange(placed), 1, [(x + 128, y + 128) for (x, y) in origins], side, angle)
        s.paint(np.arange(placed), (20, 20, 44, 44), (255, 0, 0))
        s.paint(8 + np.arange(placed), (20, 20, 44, 44), (255, 0, 0))
        for (vw, vh, origin) in ((256, 256, (400, 450)), (CW, CH, (0, 0))):
            wa, _, _ = api.pack_canvas_windows([0], origin, (vw, vh), [(CW, CH)] * 2)
            wo, _, _ = api.pack_canvas_windows([1], origin, (vw, vh), [(CW, CH)] * 2)
            d_out = torch.empty((1, 3, vh, vw), dtype=torch.uint8, device="cuda")
            al, orr = [], []
            for _ in range(repeats):                                        # alternating: the two see the same machine
                al += device_us(lambda: m.handle.canvas_compose(wa, vw, vh, d_out), calls, 1)
                orr += device_us(lambda: m.handle.canvas_compose(wo, vw, vh, d_out), calls, 1)
            row = {"placed": placed, "window": [vw, vh], "side": side, "angle": angle, "device_bytes": compose_bytes(1, vw, vh),
                   "aligned_device": stat(al), "oriented_device": stat(orr)}
            row["oriented_over_aligned"] = round(row["oriented_device"]["p50_us"] / row["aligned_device"]["p50_us"], 3)
            rows.append(row)
    m.close()
    return rows, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="IAN_simple")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--guided", action="store_true", help="the edge-aware compose against the plain one (DESIGN.md 4.13)")
    ap.add_argument("--oriented", action="store_true", help="the compose over oriented placements against the aligned one (DESIGN.md 4.16)")
    a = ap.parse_args()
    if a.guided and a.oriented:
        ap.error("--guided and --oriented are two runs")
    rows, against = (run_oriented if a.oriented else run_guided if a.guided else run)(a.arch, a.calls, a.repeats)
    metric = "canvas_oriented_latency" if a.oriented else "canvas_guided_latency" if a.guided else "canvas_latency"
    res = {"metric": metric, "arch": a.arch, "canvas": [CW, CH], "calls": a.calls, "repeats": a.repeats, "rows": rows}
    if against is not None:
        res["against_render"] = against
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

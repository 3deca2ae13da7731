"""Packed window pixels (ian_sessions_set_pixels): what the interleaved store costs against the planar one, and what
it saves the caller.  Rows:
  render    ian_session_render of one 1024 x 1024 picture (scale 16), plain and under a guide, at 1:1 and at 1/4 (256 x 256);
  compose   ian_canvas_compose of a whole 2048 x 1536 canvas with 1 and 8 placed sessions (squares of 256 pixels, every one painted):
            plain, edge-aware (ian_sessions_reserve_edges) and oriented (23 degrees), at 1:1 and at 1/4 (512 x 384).
Every row is measured under formats 0 (planar: the kernel as it was before the formats, the baseline of every ratio), 1 (rgb) and
2 (rgba): --calls calls into a DEVICE buffer back to back and one device synchronisation, after a warm-up burst; the formats alternate
inside each of the --repeats repeats, in one process, so all see the same machine.  Reported per format: the median of the repeats
in microseconds per call and their spread (max - min) / median; and the ratios rgb / planar and rgba / planar.
Beside each row, `host_transpose_us`: what the packed format replaces, np.ascontiguousarray(planar.transpose(1, 2, 0)) of the
downloaded planar window, the median of --repeats runs ON ONE CPU CORE OF THE MACHINE THAT RUNS THIS SCRIPT: a host number, not a
device one.
usage (GPU box): python scripts/window_format_latency.py [--calls 100] [--repeats 3] [--out FILE]
Prints one JSON line and, with --out, writes it there."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_photo_editor_amd import IAN, api, npe_ops, synthetic as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CW, CH = 2048, 1536
FORMATS = (0, 1, 2)
ZOOM = 4


def stat(v):
    med = float(np.median(v))
    return {"p50_us": round(med, 2), "spread": round((max(v) - min(v)) / med, 4), "repeats_us": [round(t, 2) for t in v]}


def burst_us(call, calls):
    """`call` enqueues one launch into a device buffer: a warm-up burst, then microseconds per call over `calls` calls and one
    synchronisation."""
    import torch

    def burst():
        for _ in range(calls):
            call()
        torch.cuda.synchronize()

    burst()
    t = time.perf_counter()
    burst()
    return (time.perf_counter() - t) * 1e6 / calls


def host_transpose_us(planar, repeats):
    """planar uint8 (3, vh, vw) on the host -> the median time of the interleaving copy a caller of the planar format has to make."""
    out = []
    for _ in range(max(repeats, 3)):
        t = time.perf_counter()
        np.ascontiguousarray(planar.transpose(1, 2, 0))
        out.append((time.perf_counter() - t) * 1e6)
    return round(float(np.median(out)), 1)


def measure(s, label, launch, vw, vh, calls, repeats, extra):
    """One row: launch(d_out) under every format, alternating per repeat; d_out has the format's shape."""
    import torch
    bufs = {f: torch.empty(npe_ops.window_shape(1, vw, vh, f), dtype=torch.uint8, device="cuda") for f in FORMATS}
    times = {f: [] for f in FORMATS}
    for _ in range(repeats):
        for f in FORMATS:
            s.pixel_format(f)
            times[f].append(burst_us(lambda: launch(bufs[f]), calls))
    s.pixel_format(0)
    planar = bufs[0].cpu().numpy()
    same = all(np.array_equal(bufs[f].cpu().numpy(), npe_ops.pack_window(planar, f)) for f in FORMATS)
    row = dict(extra, row=label, window=[vw, vh], same_pixels=bool(same), host_transpose_us=host_transpose_us(planar[0], repeats))
    for f in FORMATS:
        row[npe_ops.PIXEL_FORMATS[f]] = stat(times[f])
    for f in FORMATS[1:]:
        row[npe_ops.PIXEL_FORMATS[f] + "_over_planar"] = round(row[npe_ops.PIXEL_FORMATS[f]]["p50_us"] / row["planar"]["p50_us"], 3)
    return row


def run(arch, calls, repeats, sigma=8.0):
    cfg = os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py")
    table = npe_ops.guide_table(sigma)
    rs = np.random.RandomState(0)
    photo = rs.randint(0, 256, (3, CH, CW)).astype(np.uint8)
    box, red = (20, 20, 44, 44), (255, 0, 0)
    rows = []
    # render: a pool has a guide or canvases, so the pictures get a handle of their own
    m = IAN(cfg, True, params=O.make_params(arch, 1))
    s = m.sessions(16)
    s.reserve_hires(16)
    s.open_hires([1], np.ascontiguousarray(photo[None, :, 256:1280, 512:1536]))
    s.paint([1], box, red)
    for guided in (False, True):
        s.reserve_guide(table=table) if guided else s.reserve_guide()
        for zoom in (1, ZOOM):
            vw = vh = 1024 // zoom
            views, _, _ = api.pack_session_views([1], (0, 0), vw, 16, zoom=zoom)
            if zoom == 1:
                launch = lambda d, views=views, vw=vw, vh=vh: m.handle.session_render(views, vw, vh, d)
            else:
                launch = lambda d, views=views, vw=vw, vh=vh: m.handle.session_zoom(views, vw, vh, ZOOM, d)
            rows.append(measure(s, "render", launch, vw, vh, calls, repeats, {"guided": guided, "zoom": zoom}))
    m.close()
    # compose: canvas 0 holds upright squares, canvas 1 oriented ones around the same centres
    m = IAN(cfg, True, params=O.make_params(arch, 1))
    s = m.sessions(16)
    s.reserve_hires(16)
    s.reserve_canvases(2, CW, CH, 4)
    for placed in (1, 8):
        origins = [(301 + 200 * k, 403 + 40 * k) for k in range(placed)]
        for form in ("plain", "oriented", "guided"):
            s.reserve_canvas_guide()
            for cid in (0, 1):
                s.canvas_put(cid, photo)                                        # drops the placements of the round before
            if form == "oriented":
                ids, cid = 8 + np.arange(placed), 1
                s.place_oriented(ids, 1, [(x + 128, y + 128) for (x, y) in origins], 256.0, 23.0)
            else:
                ids, cid = np.arange(placed), 0
                s.place(ids, 0, origins, 4)
            s.paint(ids, box, red)
            if form == "guided":
                s.reserve_canvas_guide(table=table)
            for zoom in (1, ZOOM):
                vw, vh = CW // zoom, CH // zoom
                win, _, _ = api.pack_canvas_windows([cid], (0, 0), (vw, vh), [(CW, CH)] * 2, zoom)
                if zoom == 1:
                    launch = lambda d, win=win, vw=vw, vh=vh: m.handle.canvas_compose(win, vw, vh, d)
                else:
                    launch = lambda d, win=win, vw=vw, vh=vh: m.handle.compose_zoom(win, vw, vh, ZOOM, d)
                rows.append(measure(s, "compose", launch, vw, vh, calls, repeats, {"form": form, "placed": placed, "zoom": zoom}))
    m.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="IAN_simple")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = run(a.arch, a.calls, a.repeats)
    res = {"metric": "window_format_latency", "arch": a.arch, "canvas": [CW, CH], "calls": a.calls, "repeats": a.repeats,
           "host_transpose": "numpy on one CPU core of the machine that ran this script", "rows": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

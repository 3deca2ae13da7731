"""Zoomed views: what a view at 1/k costs against the 1:1 call on the same source window.  Per k in 2, 4, 16 and per
source -- the 2048 x 1536 canvas of scripts/canvas_latency.py with 1 and with 8 placed sessions (scale 4, every one painted), and one
1024 x 1024 session (scale 16, painted) -- the whole source at 1/k (npe_ops.zoom_window):
  (a) device   the zoomed call into a DEVICE buffer against the 1:1 call on the same source window, --calls calls back to back and one
               device synchronisation, the two alternating per repeat: both read the same bytes, the zoomed one writes 1/k^2 of
               them.  zoom_over_plain is the ratio of the medians.
  (b) host     the zoomed call with a HOST result against what a caller had to do before: the 1:1 call with a host result plus
               npe_ops.zoom_box_mean in numpy, medians.
  (c) event    the paint event with the zoomed window in its submission (brush_compose / brush_view) against the plain brush, medians:
               window_adds_us is what the view costs inside the event.
usage (GPU box): python scripts/zoom_latency.py [--calls 200] [--repeats 3] [--device-only] [--guided] [--out FILE]
--device-only measures (a) alone, for comparing two builds of the kernels.
--guided: every call under the guide (reserve_canvas_guide / reserve_guide, --sigma, default 8, as in canvas_latency.py --guided and
session_hires_latency.py --guided): the guided zoomed kernels against the guided 1:1 kernels.
Medians over --calls calls after warm-up, repeated --repeats times; reported are the median of the repeats and their spread
(max - min) / median.  Prints one JSON line and, with --out, writes it there."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from neural_photo_editor_amd import IAN, api, npe_ops, synthetic as O  # noqa: E402
from canvas_latency import device_us, median_us, stat  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CW, CH = 2048, 1536
ZOOMS = (2, 4, 16)
BOX, RED = (20, 20, 44, 44), (255, 0, 0)


def measure(name, k, size, plain_dev, zoom_dev, plain_host, zoom_host, brush, brush_zoom, calls, repeats, device_only):
    """One row: the six callables of a source at zoom k, whose view is size = (vw, vh)."""
    vw, vh = size
    pd, zd = [], []
    for _ in range(repeats):                                                # alternating: the two see the same machine
        pd += device_us(plain_dev, calls, 1)
        zd += device_us(zoom_dev, calls, 1)
    res = {"plain_host_plus_numpy": [], "zoom_host": [], "brush": [], "brush_zoom": []}
    for _ in range(0 if device_only else repeats):
        res["plain_host_plus_numpy"].append(median_us(lambda: npe_ops.zoom_box_mean(plain_host()[0], k), calls))
        res["zoom_host"].append(median_us(zoom_host, calls))
        res["brush"].append(median_us(brush, calls))
        res["brush_zoom"].append(median_us(brush_zoom, calls))
    row = {"source": name, "zoom": k, "view": [vw, vh], "read_bytes": 3 * k * k * vw * vh, "written_bytes": 3 * vw * vh,
           "plain_device": stat(pd), "zoom_device": stat(zd)}
    row["zoom_over_plain"] = round(row["zoom_device"]["p50_us"] / row["plain_device"]["p50_us"], 3)
    if device_only:
        return row
    for key, v in res.items():
        row[key] = stat(v)
    row["host_speedup"] = round(row["plain_host_plus_numpy"]["p50_us"] / row["zoom_host"]["p50_us"], 2)
    row["window_adds_us"] = round(row["brush_zoom"]["p50_us"] - row["brush"]["p50_us"], 2)
    return row


def run(arch, calls, repeats, device_only=False, sigma=None):
    import torch
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))
    h = m.handle
    s = m.sessions(16)
    s.reserve_hires(16)
    rs = np.random.RandomState(0)
    rows = []
    s.reserve_canvases(1, CW, CH, 4)
    if sigma is not None:
        s.reserve_canvas_guide(sigma)
    photo = rs.randint(0, 256, (3, CH, CW)).astype(np.uint8)
    for placed in (1, 8):
        s.canvas_put(0, photo)                                              # drops the placements of the round before
        ids = np.arange(placed)
        s.place(ids, 0, [(301 + 200 * k, 403 + 40 * k) for k in range(placed)], 4)
        s.paint(ids, BOX, RED)
        for k in ZOOMS:
            vw, vh = npe_ops.zoom_window(CW, CH, k)
            win, _, _ = api.pack_canvas_windows([0], (0, 0), (vw, vh), [(CW, CH)], zoom=k)
            d_full = torch.empty((1, 3, k * vh, k * vw), dtype=torch.uint8, device="cuda")
            d_view = torch.empty((1, 3, vh, vw), dtype=torch.uint8, device="cuda")
            rows.append(measure(
                "canvas %d x %d, %d placed" % (CW, CH, placed), k, (vw, vh),
                lambda: h.canvas_compose(win, k * vw, k * vh, d_full), lambda: h.compose_zoom(win, vw, vh, k, d_view),
                lambda: s.compose([0], (0, 0), (k * vw, k * vh)), lambda: s.compose([0], (0, 0), (vw, vh), zoom=k),
                lambda: s.paint([0], BOX, RED), lambda: s.brush_compose([0], BOX, RED, windows=([0], (0, 0), (vw, vh), k)),
                calls, repeats, device_only))
    s.reserve_canvases(0)
    if sigma is not None:
        s.reserve_guide(sigma)
    s.open_hires([1], rs.randint(0, 256, (1, 3, 1024, 1024)).astype(np.uint8))
    s.paint([1], BOX, RED)
    for k in ZOOMS:
        vw, vh = npe_ops.zoom_window(1024, 1024, k)
        views, _, _ = api.pack_session_views([1], (0, 0), (vw, vh), 16, zoom=k)
        d_full = torch.empty((1, 3, k * vh, k * vw), dtype=torch.uint8, device="cuda")
        d_view = torch.empty((1, 3, vh, vw), dtype=torch.uint8, device="cuda")
        rows.append(measure(
            "session 1024 x 1024", k, (vw, vh),
            lambda: h.session_render(views, k * vw, k * vh, d_full), lambda: h.session_zoom(views, vw, vh, k, d_view),
            lambda: s.render([1], (0, 0), (k * vw, k * vh)), lambda: s.render([1], (0, 0), (vw, vh), zoom=k),
            lambda: s.paint([1], BOX, RED), lambda: s.paint([1], BOX, RED, view=((0, 0), (vw, vh), k)),
            calls, repeats, device_only))
    m.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="IAN_simple")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--guided", action="store_true", help="the guided zoomed kernels against the guided 1:1 kernels")
    ap.add_argument("--sigma", type=float, default=8.0, help="--guided: the range sigma, in levels per channel")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"metric": "zoom_guided_latency" if a.guided else "zoom_latency", "arch": a.arch, "canvas": [CW, CH], "calls": a.calls,
           "repeats": a.repeats, "rows": run(a.arch, a.calls, a.repeats, a.device_only, a.sigma if a.guided else None)}
    if a.guided:
        res["sigma"] = a.sigma
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

"""ian_session_fit against the host loop it replaces: milliseconds per Adam step for n = 1, 8, 64 sessions and 20 steps, IAN_simple.
  device  EditSessions.fit(ids, steps, lr): every step on the device, one submission, one synchronisation (loss trace and RECON down)
  host    per step imgrad_batch (the target images go up, the gradients come down) and npe_ops.fit_adam_step in numpy; after the
          last step one set_latent(as_sample=1).  What a caller had to write before the call existed.
Both start from freshly opened sessions on the same photos.  The median of --repeats runs of each, ms per step = run / steps.
Writes one JSON line to profiles/session_fit_latency.json and prints it.  No threshold: the numbers are a report.
usage (GPU box): python scripts/session_fit_latency.py [--n 1 8 64] [--steps 20] [--lr 0.02] [--repeats 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_photo_editor_amd import IAN, npe_ops as N, synthetic as O  # noqa: E402
from neural_photo_editor_amd import lib as L  # noqa: E402


def photos(n, seed):
    """Smooth pictures plus noise, every byte value present."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:64, 0:64]
    base = 127.5 + 100.0 * np.sin(xx / 5.0 + rs.uniform(0, 6, (n, 3, 1, 1))) * np.cos(yy / 7.0 + rs.uniform(0, 6, (n, 3, 1, 1)))
    return np.uint8(np.clip(base + rs.randint(-40, 41, (n, 3, 64, 64)), 0, 255))


def host_loop(m, s, ids, T, boxes, steps, lr):
    z = np.stack([s.read(i)["Z"] for i in ids])
    t0 = time.perf_counter()
    mm, vv = np.zeros_like(z), np.zeros_like(z)
    for t in range(1, steps + 1):
        g = m.imgrad_batch(boxes, z, RGB=T)
        z, mm, vv = N.fit_adam_step(z, g, mm, vv, t, lr)
    s.sample(ids, z)
    return (time.perf_counter() - t0) * 1e3


def device_loop(s, ids, steps, lr):
    t0 = time.perf_counter()
    s.fit(ids, steps=steps, lr=lr)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    arch = "IAN_simple"
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))
    s = m.sessions(max(a.n))
    tab = L.session_tanh_table()
    rows = []
    for n in a.n:
        ids = list(range(n))
        ph = photos(n, 100 + n)
        T = tab[ph]
        boxes = np.tile(np.array([(0, 0, 64, 64)]), (n, 1))
        dev, host = [], []
        for rep in range(a.repeats + 1):       # the first run of each warms up (allocations, first launches) and is dropped
            s.open(ids, ph)
            d = device_loop(s, ids, a.steps, a.lr)
            s.open(ids, ph)
            h = host_loop(m, s, ids, T, boxes, a.steps, a.lr)
            if rep:
                dev.append(d)
                host.append(h)
        d50, h50 = float(np.median(dev)), float(np.median(host))
        rows.append({"n": n, "device_ms_per_step": round(d50 / a.steps, 4), "host_ms_per_step": round(h50 / a.steps, 4),
                     "host_over_device": round(h50 / d50, 2),
                     "device_min_max": [round(min(dev) / a.steps, 4), round(max(dev) / a.steps, 4)],
                     "host_min_max": [round(min(host) / a.steps, 4), round(max(host) / a.steps, 4)]})
    res = {"metric": "session_fit_latency", "arch": arch, "steps": a.steps, "lr": a.lr, "repeats": a.repeats, "rows": rows}
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "session_fit_latency.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)
    m.close()


if __name__ == "__main__":
    main()

"""Saved edit sessions: what parking and resuming editors costs.  Per pool layout -- scale in --scales (0 = no full-resolution
reservation), without and with the local reservation plus a history of --depth -- and n in --n sessions, each opened, painted and
(with a history) marked until its ring is full:
  save_host / load_host       ian_session_save / ian_session_load with the bodies in host memory (staging passes, one synchronisation);
  save_device / load_device   the same with the bodies in device memory, the device synchronised after every call;
  read_loop                   ian_session_read of every readable field of every session, one synchronising copy each: the only way
                              out of the pool without the two calls above -- and it reaches neither the rings nor the host's counters.
Reported per call: microseconds (median over --calls calls after warm-up) and GB/s against n * body_bytes, the bytes of the records
(read_loop: against the bytes it does move).  Repeated --repeats times: the median of the repeats and their spread (max - min) / median.
usage (GPU box): python scripts/session_park_latency.py [--scales 0 1 4] [--n 1 16 64] [--depth 16] [--calls 200] [--repeats 3] [--out FILE]
Prints one JSON line and, with --out, writes it there."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_photo_editor_amd import IAN, npe_ops as N, synthetic as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def median_us(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    lat = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        lat.append((time.perf_counter() - t) * 1e6)
    return float(np.median(lat))


def stat(v, nbytes):
    med = float(np.median(v))
    return {"p50_us": round(med, 2), "spread": round((max(v) - min(v)) / med, 4), "GBps": round(nbytes / (med * 1e-6) / 1e9, 2),
            "repeats_us": [round(t, 2) for t in v]}


def run(arch, scales, ns, depth, calls, repeats):
    import torch
    m = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))
    h = m.handle
    cap = max(ns)
    s = m.sessions(cap)
    rows = []
    for scale in scales:
        for full in (False, True):
            s.reserve_history(0)
            s.reserve_hires(scale)
            s.reserve_local(full)
            s.reserve_history(depth if full else 0)
            zl = m.get_zdim()
            bb = N.session_record_layout(zl, scale, full, depth if full else 0)[1]
            S = 64 * max(scale, 1)
            for n in ns:
                ids = np.arange(n, dtype=np.int32)
                rs = np.random.RandomState(n)
                photos = rs.randint(0, 256, (n, 3, S, S)).astype(np.uint8)
                (s.open_hires if scale else s.open)(ids, photos)
                if full:
                    s.set_local(ids, flags=1)
                for _ in range(depth + 1 if full else 1):                 # a full history: `depth` entries of the record carry data
                    if full:
                        s.mark(ids)
                    s.paint(ids, (20, 20, 28, 28), (255, 0, 0))
                meta = np.zeros(n, N.SESSION_META_DTYPE)
                body = np.empty((n, bb), np.uint8)
                d_body = torch.empty((n, bb), dtype=torch.uint8, device="cuda")
                keys = ["Z", "RECON", "ERROR", "IM", "GIM", "MODE"] + (["FIELD", "FIELD_KIND", "SOURCE"] if scale else []) + \
                    (["UMASK", "LOCAL"] if full else [])
                read_bytes = n * sum(h.session_read(0, k, scale=scale).nbytes for k in keys)

                def dev(fn):
                    fn()
                    torch.cuda.synchronize()

                def read_loop():
                    for sid in range(n):
                        for k in keys:
                            h.session_read(sid, k, scale=scale)

                h.session_save(ids, meta, body)
                h.session_save(ids, meta, d_body)
                torch.cuda.synchronize()
                calls_of = {"save_host": lambda: h.session_save(ids, meta, body), "load_host": lambda: h.session_load(ids, meta, body),
                            "save_device": lambda: dev(lambda: h.session_save(ids, meta, d_body)),
                            "load_device": lambda: dev(lambda: h.session_load(ids, meta, d_body)), "read_loop": read_loop}
                res = {k: [] for k in calls_of}
                for _ in range(repeats):
                    for k, fn in calls_of.items():
                        res[k].append(median_us(fn, calls if k != "read_loop" else max(calls // 10, 5)))
                row = {"scale": scale, "local": int(full), "depth": depth if full else 0, "n": n, "body_bytes": bb, "record_bytes": n * bb,
                       "read_loop_bytes": read_bytes, "read_loop_calls": n * len(keys)}
                for k, v in res.items():
                    row[k] = stat(v, read_bytes if k == "read_loop" else n * bb)
                rows.append(row)
                print("scale %d local %d n %d: done" % (scale, int(full), n), file=sys.stderr, flush=True)
    m.close()
    return rows


def table(rows):
    """The rows as a markdown table."""
    out = ["| scale | local + depth | n | record bytes | save host | load host | save device | load device | read loop (bytes, calls) |",
           "|---|---|---|---|---|---|---|---|---|"]
    cell = lambda r: "%.0f us, %.1f GB/s" % (r["p50_us"], r["GBps"])
    for r in rows:
        out.append("| %d | %s | %d | %d | %s | %s | %s | %s | %s (%d, %d) |" % (
            r["scale"], "%d" % r["depth"] if r["local"] else "-", r["n"], r["record_bytes"], cell(r["save_host"]), cell(r["load_host"]),
            cell(r["save_device"]), cell(r["load_device"]), cell(r["read_loop"]), r["read_loop_bytes"], r["read_loop_calls"]))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="IAN_simple")
    ap.add_argument("--scales", type=int, nargs="*", default=[0, 1, 4])
    ap.add_argument("--n", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--depth", type=int, default=16)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = run(a.arch, a.scales, a.n, a.depth, a.calls, a.repeats)
    res = {"metric": "session_park_latency", "arch": a.arch, "calls": a.calls, "repeats": a.repeats, "rows": rows}
    print(json.dumps(res))
    print(table(rows), file=sys.stderr)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

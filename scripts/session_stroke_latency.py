"""ian_session_stroke against the loop of ian_session_brush calls it replaces: both architectures, n = 1, 16, 64 sessions, K = 4, 16 points.
  stroke  EditSessions.stroke(ids, paths): the K steps in one submission, one table up, one synchronisation, shown down once
  loop    for k in range(K): EditSessions.brush(ids, paths[:, k]): what a caller had to write before the call existed (existing code,
          the yardstick); from its second call on it hits the residency, so neither side runs a forward the other does not
Both run on the same handle and pool, on two id ranges opened from the same photos, every stroke of a case with the same K for all n
sessions and its own random rectangles.  Per case --repeats repeats of --strokes strokes of each, alternating; a repeat's figure is the
median over its strokes, the case's the median of the repeats, with their spread (min, max).  events/s = n * K / the median.
Writes one JSON line to profiles/session_stroke_latency.json and prints it, with a table for DESIGN.md 4.9.  No threshold: a report.

Launches and copies per stroke come from a trace, not from a stopwatch:
  rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -o t -- python scripts/session_stroke_latency.py --trace ARCH N K
      warm-up, a second of idleness, 20 strokes as the loop, a second of idleness, 20 strokes as the call
  python scripts/session_stroke_latency.py --summarize DIR
      splits the kernel trace at its two longest gaps and counts, per stroke, the dispatches and the copies of either phase (and the
      device time of every kernel) -> one JSON line
usage (GPU box): python scripts/session_stroke_latency.py [--archs IAN_simple IAN] [--n 1 16 64] [--k 4 16] [--strokes 200] [--repeats 3]"""
import argparse
import csv
import glob
import json
import os
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRACE_STROKES = 20


def photos(n, seed):
    """Smooth pictures plus noise, every byte value present."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:64, 0:64]
    base = 127.5 + 100.0 * np.sin(xx / 5.0 + rs.uniform(0, 6, (n, 3, 1, 1))) * np.cos(yy / 7.0 + rs.uniform(0, 6, (n, 3, 1, 1)))
    return np.uint8(np.clip(base + rs.randint(-40, 41, (n, 3, 64, 64)), 0, 255))


def drag(n, K, rs):
    """(n, K, 4): per session a mouse track of K points, a 4x4 brush (d = 12) moving a pixel or two per event."""
    from neural_photo_editor_amd import npe_ops as N
    start = rs.randint(4, 60, (n, 2))
    steps = np.cumsum(rs.randint(-2, 3, (n, K, 2)), axis=1)
    pts = np.clip(start[:, None, :] + steps, 0, 63)
    return np.array([[N.brush_rect(x, y, 12) for x, y in p] for p in pts])


def one_stroke(s, ids, paths, col):
    t0 = time.perf_counter()
    s.stroke(ids, paths, col, weight=0.01)
    return (time.perf_counter() - t0) * 1e3


def one_loop(s, ids, paths, col):
    t0 = time.perf_counter()
    for k in range(paths.shape[1]):
        s.brush(ids, paths[:, k], col, weight=0.01)
    return (time.perf_counter() - t0) * 1e3


def model(arch):
    from neural_photo_editor_amd import IAN, synthetic as O
    return IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))


def setup(m, n):
    s = m.sessions(2 * n)
    A, B = list(range(n)), list(range(n, 2 * n))
    ph = photos(n, 100 + n)
    s.open(A, ph)
    s.open(B, ph)
    col = np.tile(np.array([(220, 60, 40)]), (n, 1))
    return s, A, B, col, ph


def measure(a):
    rows = []
    for arch in a.archs:
        m = model(arch)
        for n in a.n:
            s, A, B, col, ph = setup(m, n)
            for K in a.k:
                rs = np.random.RandomState(1000 * n + K)
                for _ in range(3):                        # warm-up: allocations, the first launches at this batch, the tuner
                    p = drag(n, K, rs)
                    one_loop(s, A, p, col)
                    one_stroke(s, B, p, col)
                reps = {"stroke": [], "loop": []}
                for _ in range(a.repeats):
                    s.open(A, ph)                         # every repeat starts from the photos again: the latents do not drift away
                    s.open(B, ph)
                    ts, tl = [], []
                    for _ in range(a.strokes):
                        p = drag(n, K, rs)
                        tl.append(one_loop(s, A, p, col))
                        ts.append(one_stroke(s, B, p, col))
                    reps["stroke"].append(float(np.median(ts)))
                    reps["loop"].append(float(np.median(tl)))
                st, lp = float(np.median(reps["stroke"])), float(np.median(reps["loop"]))
                rows.append({"arch": arch, "n": n, "K": K,
                             "stroke_ms": round(st, 4), "stroke_min_max": [round(min(reps["stroke"]), 4), round(max(reps["stroke"]), 4)],
                             "loop_ms": round(lp, 4), "loop_min_max": [round(min(reps["loop"]), 4), round(max(reps["loop"]), 4)],
                             "loop_over_stroke": round(lp / st, 3),
                             "stroke_events_per_s": round(n * K / st * 1e3, 1), "loop_events_per_s": round(n * K / lp * 1e3, 1),
                             "saved_us_per_step": round((lp - st) / K * 1e3, 1)})
                print(json.dumps(rows[-1]), flush=True)
            s.close()
        m.close()
    res = {"metric": "session_stroke_latency", "strokes": a.strokes, "repeats": a.repeats, "rows": rows}
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "session_stroke_latency.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)
    print("| arch | n | K | stroke ms (min..max) | loop ms (min..max) | loop / stroke | events/s stroke | events/s loop | saved us / step |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %.3f (%.3f..%.3f) | %.3f (%.3f..%.3f) | %.2f | %.0f | %.0f | %.0f |" % (
            r["arch"], r["n"], r["K"], r["stroke_ms"], r["stroke_min_max"][0], r["stroke_min_max"][1], r["loop_ms"], r["loop_min_max"][0],
            r["loop_min_max"][1], r["loop_over_stroke"], r["stroke_events_per_s"], r["loop_events_per_s"], r["saved_us_per_step"]))


def trace(arch, n, K):
    m = model(arch)
    s, A, B, col, ph = setup(m, n)
    rs = np.random.RandomState(7)
    for _ in range(3):
        p = drag(n, K, rs)
        one_loop(s, A, p, col)
        one_stroke(s, B, p, col)
    time.sleep(1.0)
    for _ in range(TRACE_STROKES):
        one_loop(s, A, drag(n, K, rs), col)
    time.sleep(1.0)
    for _ in range(TRACE_STROKES):
        one_stroke(s, B, drag(n, K, rs), col)
    s.close()
    m.close()


def summarize(d):
    def table(pattern):
        files = glob.glob(os.path.join(d, "**", pattern), recursive=True)
        return sorted((r for f in files for r in csv.DictReader(open(f))), key=lambda r: int(r["Start_Timestamp"]))

    kern, copies = table("*kernel_trace.csv"), table("*memory_copy_trace.csv")
    gaps = sorted(range(1, len(kern)), key=lambda i: int(kern[i]["Start_Timestamp"]) - int(kern[i - 1]["End_Timestamp"]))[-2:]
    lo, hi = sorted(gaps)
    t_loop, t_stroke = int(kern[lo]["Start_Timestamp"]), int(kern[hi]["Start_Timestamp"])
    out = {"strokes_per_phase": TRACE_STROKES}
    for name, rows, (t0, t1) in (("loop", kern[lo:hi], (t_loop, t_stroke)), ("stroke", kern[hi:], (t_stroke, 1 << 62))):
        per = defaultdict(lambda: [0, 0])
        for r in rows:
            k = r["Kernel_Name"].split("(")[0].replace("void ", "")
            per[k][0] += 1
            per[k][1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        # A copy is a row of the memory-copy trace (a phase's copies start before its next kernel: counted from a millisecond before
        # the phase's first dispatch) or, for the small pageable copies of these calls, a dispatch of the runtime's own copy kernel.
        ncopy = sum(1 for r in copies if t0 - 1000000 <= int(r["Start_Timestamp"]) < t1 - 1000000)
        nblit = sum(v[0] for k, v in per.items() if "copyBuffer" in k)
        out[name] = {"launches_per_stroke": round((len(rows) - nblit) / TRACE_STROKES, 2),
                     "copies_per_stroke": round((ncopy + nblit) / TRACE_STROKES, 2),
                     "kernel_us_per_stroke": round(sum(v[1] for v in per.values()) / TRACE_STROKES / 1e3, 1),
                     "kernels": sorted(({"kernel": k, "launches_per_stroke": round(v[0] / TRACE_STROKES, 2),
                                         "us_per_stroke": round(v[1] / TRACE_STROKES / 1e3, 2)} for k, v in per.items()),
                                       key=lambda q: -q["us_per_stroke"])}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--archs", nargs="*", default=["IAN_simple", "IAN"])
    ap.add_argument("--n", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--k", type=int, nargs="*", default=[4, 16])
    ap.add_argument("--strokes", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", nargs=3, metavar=("ARCH", "N", "K"))
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.trace:
        trace(a.trace[0], int(a.trace[1]), int(a.trace[2]))
    else:
        measure(a)


if __name__ == "__main__":
    main()

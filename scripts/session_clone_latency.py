"""ian_session_clone against the two ways to do without it: both architectures, n = 1, 16, 64 sessions, steps = 1, 8.
  clone   (a) EditSessions.clone(ids, boxes, sources, offsets, steps=K): the K steps in one submission, 44 n bytes up, shown down once
  loop    (b) for k in range(K): EditSessions.clone(..., steps=1): K submissions, K tables, K blends, K copies of shown; from its second
          call on it hits the residency, so neither side runs a forward the other does not
  host    (c) what a caller does without the call: ian_session_read of every source's GIM (12 KB each, once per event: the sources do not
          change), npe_ops.clone_target on the host, K times IAN.brush_step_batch with the 48 KB float images and photo = (RECON,
          ERROR) kept on the host since the open (its own residency skips the forward from the second step on), then set_latent
          with the last z.  It leaves the stored IM, the user mask and the edit field of the session path behind.
(b) and (c) are the yardsticks: (c) is existing code, (b) the call under test at steps = 1 only.  All three run on the same handle and
pool, on three id ranges opened from the same photos; item i of a range reads the GIM of item (i + 1) % n of the same range (n = 1: its own)
at a random offset.  Per case --repeats repeats of --calls calls of each, alternating; a repeat's figure is the median over its calls,
the case's the median of the repeats, with their spread (min, max).
Writes one JSON line to profiles/session_clone_latency.json and prints it, with a table for DESIGN.md 4.10.  No threshold: a report.

Launches and copies per call come from a trace, not from a stopwatch:
  rocprofv3 --kernel-trace --stats -d DIR -o t -- python scripts/session_clone_latency.py --trace ARCH N K
      warm-up, then 20 calls of each of the three paths (host, loop, clone), a second of idleness before each phase
  python scripts/session_clone_latency.py --summarize DIR
      splits the kernel trace at its three longest gaps and counts, per call, the dispatches of every phase (the small pageable copies
      of these calls are dispatches of the runtime's copy kernel and are counted as copies) and their device time -> one JSON line
  python scripts/session_clone_latency.py --tip D [--n 1 64] [--steps 1]
      the weighted clone instead: D x D clone events through ian_session_clone (plain) against the same events under
      npe_ops.round_tip(D, 0.5) through ian_session_stamp_soft (tip), alternating within a repeat on one id range
      -> profiles/session_soft_clone_latency_D<D>.json
usage (GPU box): python scripts/session_clone_latency.py [--archs IAN_simple IAN] [--n 1 16 64] [--steps 1 8] [--calls 200] [--repeats 3]"""
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

TRACE_CALLS = 20
WEIGHT = 0.01


def photos(n, seed):
    """Smooth pictures plus noise, every byte value present."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:64, 0:64]
    base = 127.5 + 100.0 * np.sin(xx / 5.0 + rs.uniform(0, 6, (n, 3, 1, 1))) * np.cos(yy / 7.0 + rs.uniform(0, 6, (n, 3, 1, 1)))
    return np.uint8(np.clip(base + rs.randint(-40, 41, (n, 3, 64, 64)), 0, 255))


def events(n, rs):
    """(boxes (n,4), offsets (n,2)): a 16x16 rectangle per session and a shift that keeps its copy inside the picture."""
    c1, r1 = rs.randint(0, 49, n), rs.randint(0, 49, n)
    boxes = np.stack([c1, r1, c1 + 16, r1 + 16], axis=1)
    offs = np.stack([rs.randint(0, 49, n) - c1, rs.randint(0, 49, n) - r1], axis=1)
    return boxes, offs


def model(arch):
    from neural_photo_editor_amd import IAN, synthetic as O
    return IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=O.make_params(arch, 1))


class Case:
    """One handle, one pool, three id ranges opened from the same photos."""

    def __init__(self, m, n):
        self.m, self.n = m, n
        self.s = m.sessions(3 * n)
        self.ids = [list(range(k * n, (k + 1) * n)) for k in range(3)]
        self.src = [[r[(i + 1) % n] for i in range(n)] for r in self.ids]
        self.ph = photos(n, 100 + n)
        self.reopen()

    def reopen(self):
        for r in self.ids:
            self.s.open(r, self.ph)
        st = [self.s.read(i) for i in self.ids[2]]          # what the host path keeps per session since the open
        self.recon = np.stack([t["RECON"] for t in st])
        self.error = np.stack([t["ERROR"] for t in st])
        self.z = np.stack([t["Z"] for t in st])

    def clone(self, boxes, offs, K):
        t0 = time.perf_counter()
        self.s.clone(self.ids[0], boxes, self.src[0], offs, "GIM", steps=K, weight=WEIGHT)
        return (time.perf_counter() - t0) * 1e3

    def loop(self, boxes, offs, K):
        t0 = time.perf_counter()
        for _ in range(K):
            self.s.clone(self.ids[1], boxes, self.src[1], offs, "GIM", steps=1, weight=WEIGHT)
        return (time.perf_counter() - t0) * 1e3

    def host(self, boxes, offs, K):
        from neural_photo_editor_amd import npe_ops as N
        t0 = time.perf_counter()
        T = np.stack([N.clone_target(self.m.handle.session_read(sid, "GIM"), b, o) for sid, b, o in zip(self.src[2], boxes, offs)])
        z = self.z
        for _ in range(K):
            z = self.m.brush_step_batch(boxes, z, T, weight=WEIGHT, sign=-1.0, modes=[1] * self.n, image=False, photo=(self.recon, self.error))[0]
        self.s.set_latent(self.ids[2], z)
        self.z = z
        return (time.perf_counter() - t0) * 1e3

    PATHS = ("clone", "loop", "host")


def measure(a):
    rows = []
    for arch in a.archs:
        m = model(arch)
        for n in a.n:
            c = Case(m, n)
            for K in a.steps:
                rs = np.random.RandomState(1000 * n + K)
                for _ in range(3):                        # warm-up: allocations, the first launches at this batch, the tuner
                    b, o = events(n, rs)
                    for p in Case.PATHS:
                        getattr(c, p)(b, o, K)
                reps = {p: [] for p in Case.PATHS}
                for _ in range(a.repeats):
                    c.reopen()                            # every repeat starts from the photos again: the latents do not drift away
                    t = {p: [] for p in Case.PATHS}
                    for _ in range(a.calls):
                        b, o = events(n, rs)
                        for p in Case.PATHS[::-1]:
                            t[p].append(getattr(c, p)(b, o, K))
                    for p in Case.PATHS:
                        reps[p].append(float(np.median(t[p])))
                med = {p: float(np.median(reps[p])) for p in Case.PATHS}
                row = {"arch": arch, "n": n, "steps": K}
                for p in Case.PATHS:
                    row[p + "_ms"] = round(med[p], 4)
                    row[p + "_min_max"] = [round(min(reps[p]), 4), round(max(reps[p]), 4)]
                row["loop_over_clone"] = round(med["loop"] / med["clone"], 3)
                row["host_over_clone"] = round(med["host"] / med["clone"], 3)
                row["bytes_up_clone"], row["bytes_down_clone"] = 44 * n, 12288 * n
                row["bytes_up_host"] = K * (28 + 400 + 49152) * n    # per step the 7-word items, RECON / ERROR compared, the images (cached when equal)
                rows.append(row)
                print(json.dumps(row), flush=True)
            c.s.close()
        m.close()
    res = {"metric": "session_clone_latency", "calls": a.calls, "repeats": a.repeats, "rows": rows}
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "session_clone_latency.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)
    print("| arch | n | steps | (a) clone ms (min..max) | (b) loop ms (min..max) | (c) host ms (min..max) | b / a | c / a |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %.3f (%.3f..%.3f) | %.3f (%.3f..%.3f) | %.3f (%.3f..%.3f) | %.2f | %.2f |" % (
            r["arch"], r["n"], r["steps"], r["clone_ms"], *r["clone_min_max"], r["loop_ms"], *r["loop_min_max"], r["host_ms"],
            *r["host_min_max"], r["loop_over_clone"], r["host_over_clone"]))


def measure_tip(a):
    """plain clone against the weighted clone of the same D x D rectangles, one pool, the same ids: what the tip costs a clone event."""
    from neural_photo_editor_amd import npe_ops as N
    D, rows = a.tip, []
    for arch in a.archs:
        m = model(arch)
        for n in a.n:
            s = m.sessions(n)
            s.reserve_tips(1)
            s.set_tip(0, N.round_tip(D, 0.5))
            ids = list(range(n))
            src = [ids[(i + 1) % n] for i in range(n)]
            s.open(ids, photos(n, 100 + n))
            rs = np.random.RandomState(n)
            c1, r1 = rs.randint(0, 65 - D, n), rs.randint(0, 65 - D, n)
            boxes = np.stack([c1, r1, c1 + D, r1 + D], axis=1)
            offs = np.stack([rs.randint(0, 65 - D, n) - c1, rs.randint(0, 65 - D, n) - r1], axis=1)
            for K in a.steps:
                def call(tips):
                    t0 = time.perf_counter()
                    s.clone(ids, boxes, src, offs, "GIM", steps=K, weight=WEIGHT, tips=tips)
                    return (time.perf_counter() - t0) * 1e3
                for _ in range(5):
                    call(None), call(0)
                reps = {"plain": [], "tip": []}
                for _ in range(a.repeats):
                    s.open(ids, photos(n, 100 + n))
                    t = {"plain": [], "tip": []}
                    for _ in range(a.calls):
                        t["tip"].append(call(0))
                        t["plain"].append(call(None))
                    for p in t:
                        reps[p].append(float(np.median(t[p])))
                row = {"arch": arch, "n": n, "steps": K, "D": D}
                for p in reps:
                    row[p + "_ms"] = round(float(np.median(reps[p])), 4)
                    row[p + "_min_max"] = [round(min(reps[p]), 4), round(max(reps[p]), 4)]
                row["tip_over_plain"] = round(row["tip_ms"] / row["plain_ms"], 4)
                rows.append(row)
                print(json.dumps(row), flush=True)
            s.close()
        m.close()
    res = {"metric": "session_soft_clone_latency", "calls": a.calls, "repeats": a.repeats, "D": D, "rows": rows}
    with open(os.path.join(ROOT, "profiles", "session_soft_clone_latency_D%d.json" % D), "w") as fh:
        fh.write(json.dumps(res) + "\n")
    print(json.dumps(res))


def trace(arch, n, K):
    m = model(arch)
    c = Case(m, n)
    rs = np.random.RandomState(7)
    for _ in range(3):
        b, o = events(n, rs)
        for p in Case.PATHS:
            getattr(c, p)(b, o, K)
    for p in Case.PATHS[::-1]:                            # host, loop, clone
        time.sleep(1.0)
        for _ in range(TRACE_CALLS):
            getattr(c, p)(*events(n, rs), K)
    c.s.close()
    m.close()


def summarize(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    kern = sorted((r for f in files for r in csv.DictReader(open(f))), key=lambda r: int(r["Start_Timestamp"]))
    gaps = sorted(range(1, len(kern)), key=lambda i: int(kern[i]["Start_Timestamp"]) - int(kern[i - 1]["End_Timestamp"]))[-3:]
    a, b, c = sorted(gaps)
    out = {"calls_per_phase": TRACE_CALLS}
    for name, rows in (("host", kern[a:b]), ("loop", kern[b:c]), ("clone", kern[c:])):
        per = defaultdict(lambda: [0, 0])
        for r in rows:
            k = r["Kernel_Name"].split("(")[0].replace("void ", "")
            per[k][0] += 1
            per[k][1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        nblit = sum(v[0] for k, v in per.items() if "copyBuffer" in k or "fillBuffer" in k)
        out[name] = {"launches_per_call": round((len(rows) - nblit) / TRACE_CALLS, 2),
                     "copy_kernels_per_call": round(nblit / TRACE_CALLS, 2),
                     "kernel_us_per_call": round(sum(v[1] for v in per.values()) / TRACE_CALLS / 1e3, 1),
                     "kernels": sorted(({"kernel": k, "launches_per_call": round(v[0] / TRACE_CALLS, 2),
                                         "us_per_call": round(v[1] / TRACE_CALLS / 1e3, 2)} for k, v in per.items()),
                                       key=lambda q: -q["us_per_call"])}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--archs", nargs="*", default=["IAN_simple", "IAN"])
    ap.add_argument("--n", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--steps", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tip", type=int, default=0, metavar="D", help="the weighted clone: D x D plain clone events against the same under round_tip(D, 0.5)")
    ap.add_argument("--trace", nargs=3, metavar=("ARCH", "N", "K"))
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.tip:
        measure_tip(a)
    elif a.trace:
        trace(a.trace[0], int(a.trace[1]), int(a.trace[2]))
    else:
        measure(a)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Benchmark of the IAN hot path on MI355X (contract: see the task statement / DESIGN.md section 6).

A "step" = one pass of the hot path over one batch of synthetic input already resident in HBM:
encode -> z -> decode of IAN_simple at batch 64 (BASELINE.json configs[1]).  `value` = whole-job
64x64 reconstructions per second over all ranks (replicas: the path has no data-path collective).

A plain run sets up, warms up, times the --steps steps and prints the headline line (value, ms_per_step, step_ms).
--dump-outputs DIR also writes what the last timed step computed (DIR/reconstruction.npy, float32, rank 0's seeded inputs).
--full adds every secondary measurement below to the same JSON line:
  roofline      dominant kernel (tapgemm, fp32 MFMA): algorithmic FLOP per launch / mean launch duration,
                measured with HIP events recorded on the launch stream inside libian (ian_profile_*),
                in a separate profiled pass of the same workload (event records perturb the timed pass);
  cpu_baseline  the torch-CPU twin of the oracle ("port": the reference's Theano path cannot run here),
                rank 0, N=1 only, bounded sample;
  step_ms       p50/p95 of the K timed steps (device time between consecutive steps; plain runs too);
  full_ian      the same measurement for BASELINE.json configs[2]: full IAN, batch 256 per GPU, with its own roofline;
  edit_step     p50/p95 latency of one NPE latent-brush step (BASELINE.json configs[3]): imgradRGB +
                Z update (reference gradient descent, NPE.py:199-209) + sample_at, batch 1.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense, spec
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_bf16, dense, spec (the opt-in tg_bf16x3 secondary only)
FLOP_PER_RECON = {"IAN_simple": 2.592e9, "IAN": 8.463e9}  # ALGORITHMIC (every MDCL branch counted separately)
# what the kernels EXECUTE: an MDCL is one composite stencil whose centre tap is shared by its branches (SURVEY App. A:
# 3298.1 M MAC per decoder instead of 3576.1 M) -> 7.907 GFLOP per full-IAN reconstruction; IAN_simple has no MDCL
FLOP_EXECUTED = {"IAN_simple": 2.592e9, "IAN": 7.907e9}
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E spec (6290 GB/s measured achievable)
EDIT_STEP_BYTES = 232e6         # one brush event = 2 decoder forwards + 1 backward-data, batch 1, uncached weights
EDIT_STEP_BYTES_EXECUTED = 151e6  # what a brush event executes with the decoder-forward cache: 1 forward (77 MB) + 1 backward-data (74 MB)
B1_RECON_BYTES = 214e6          # IAN_simple encoder B=1 137 MB + decoder B=1 77 MB (weights dominate), floors 17.2 + 9.7 us
# train_IAN.py step, FLOP per image: E = encoder + discriminator forward, D = decoder forward (executed);
# data-gradient and weight-gradient passes each cost one forward.  Both updates run 3 E + 2 D forward (train_IAN.py:116,140,149).
#   update_gen     backward: decoder x2 passes (data + weight) = 4 D, encoder data-gradient for X_hat and X_gen = 2 E
#   update_discrim backward: encoder x3 passes (data + weight) = 6 E, + the Z group's path: 1 E (data, X_hat) + 1 D (data)
E_FLOP, D_FLOP = 2 * 0.6582e9, 2 * 3.2981e9
TRAIN_FLOP_PER_IMAGE = {"gen": 5 * E_FLOP + 6 * D_FLOP, "discrim": 10 * E_FLOP + 3 * D_FLOP}


def _cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "?"


def cpu_baseline(arch, P, batch, budget_s=22.0):
    """the torch-CPU restatement (NOT Theano) on this host, >=5 warm-up and >=20 timed passes
    (or as many as the stated time budget allows, never fewer than 5), median and p95, batch 1 (1 thread and all
    threads) and the GPU workload's batch.  When one pass at the GPU batch takes longer than 0.5 s the batch case
    falls back to 16 images so that the whole baseline stays within ~budget_s seconds; the sample string says so."""
    import torch
    from oracle.torch_twin import TorchTwin      # the ONLY use of oracle/ in this file: the timed CPU baseline
    from neural_photo_editor_amd import synthetic as O
    cores = os.cpu_count() or 1
    tw = TorchTwin(arch, P)

    def run(b, threads, budget, min_timed=5, want=20):
        torch.set_num_threads(threads)
        x = torch.from_numpy(O.make_images(b, seed=0))
        with torch.no_grad():
            t0 = time.perf_counter()
            tw.decode(tw.encode(x))
            first = time.perf_counter() - t0
            warm = 1
            while warm < 5 and (time.perf_counter() - t0) < 0.25 * budget:
                tw.decode(tw.encode(x)); warm += 1
            ts = []
            t1 = time.perf_counter()
            while len(ts) < want and (len(ts) < min_timed or time.perf_counter() - t1 < budget):
                t = time.perf_counter(); tw.decode(tw.encode(x)); ts.append(time.perf_counter() - t)
        ts = np.array(ts)
        return {"batch": b, "threads": threads, "warmup": warm, "timed": len(ts), "p50_ms": float(np.percentile(ts, 50) * 1e3),
                "p95_ms": float(np.percentile(ts, 95) * 1e3), "value": float(b / np.percentile(ts, 50)), "first_pass_ms": first * 1e3}

    # thread count for the multi-threaded cases: the fastest of {all, a quarter, a sixteenth of the} logical CPUs on a
    # short probe (oneDNN scales poorly past the physical core count on wide hosts: batch 1 on 256 threads measured 6 s
    # per pass against 53 ms on one thread)
    probe_b = 16
    cand = sorted({cores, max(1, cores // 4), max(1, cores // 16)}, reverse=True)
    probes = {}
    for t in reversed(cand):                                   # small thread counts first; skip hopeless wide ones
        probes[t] = run(probe_b, t, 0.0, min_timed=1, want=1)
        if probes[t]["first_pass_ms"] > 4000:
            break
    best_t = min(probes, key=lambda t: probes[t]["p50_ms"])
    cases = [run(1, 1, 3.0), run(1, best_t, 3.0)]
    per_img = probes[best_t]["p50_ms"] / probe_b
    b_main = batch if per_img * batch < 500.0 else probe_b
    main = run(b_main, best_t, budget_s - 10.0)
    cases.append(main)
    note = "" if b_main == batch else " (one pass at batch %d would take ~%.1f s: batch %d used to keep the baseline within its time budget)" % (batch, per_img * batch / 1e3, b_main)
    return {"value": main["value"], "unit": "reconstructions/s", "cores": best_t, "kind": "port",
            "p50_ms": main["p50_ms"], "p95_ms": main["p95_ms"], "host_logical_cpus": cores, "cpu": _cpu_model_name(),
            "sample": "%s encode->decode through the torch-CPU restatement (not Theano): %d warm-up + %d timed passes of batch %d on %d threads, median%s"
                      % (arch, main["warmup"], main["timed"], b_main, best_t, note),
            "cases": cases}


def pmc_traffic(arch, B):
    """HBM bytes per tapgemm launch from the committed rocprofv3 PMC passes of this same command (profiles/, made by
    scripts/profile_round.sh + scripts/summarize_profile.py; FETCH_SIZE x2-corrected per MI355X_MICROARCH.md).
    PMC counters cannot be read from inside the process, so the latest committed summary is quoted; None if absent."""
    import glob
    tag = "ian_simple_b64" if (arch, B) == ("IAN_simple", 64) else ("ian_b256" if (arch, B) == ("IAN", 256) else None)
    if tag is None:
        return None, None
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s.json" % tag)))
    if not files:
        return None, None
    try:
        from neural_photo_editor_amd import build as _b
        with open(files[-1]) as fh:
            js = json.load(fh)
        v = js.get("tapgemm_traffic_bytes_per_launch")
        src = os.path.relpath(files[-1], ROOT)
        cur = _b._digest("inference")     # the sources a reconstruction kernel can depend on (training-only files excluded)
        if js.get("csrc_digest") not in (cur, _b._digest()):
            # the profile was taken on other kernel sources than the ones running now: do not quote it as this build's traffic
            return None, "%s is stale (csrc digest %s != current %s)" % (src, str(js.get("csrc_digest"))[:12], cur[:12])
        return (float(v) if v else None), src
    except Exception:
        return None, None


def b1_pmc_traffic(which):
    """HBM bytes per brush event ('edit') / per batch-1 reconstruction ('b1_recon') from the committed rocprofv3 PMC passes of
    scripts/b1_chain_profile.py (profiles/r*_batch1_chains.json: scripts/profile_b1.sh + scripts/summarize_b1_profile.py); None when
    absent or taken on other kernel sources than the ones running now (csrc digest)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_batch1_chains.json")))
    if not files:
        return None, None
    try:
        from neural_photo_editor_amd import build as _b
        js = json.load(open(files[-1]))
        src = os.path.relpath(files[-1], ROOT)
        cur = _b._digest("inference")
        if js.get("csrc_digest") not in (cur, _b._digest()):
            return None, "%s is stale (csrc digest %s != current %s)" % (src, str(js.get("csrc_digest"))[:12], cur[:12])
        v = js.get(which, {}).get("hbm_bytes_per_unit")
        return (float(v) if v else None), "bytes per %s (rocprofv3 PMC FETCH_SIZE x2 + WRITE_SIZE, %s)" % ("brush event" if which == "edit" else "reconstruction", src)
    except Exception:
        return None, None


def train_pmc_traffic(batch):
    """HBM bytes per update of the training step from the committed rocprofv3 PMC passes (profiles/r*_train_ian_b128.json, written by
    scripts/profile_train.sh + scripts/summarize_train_profile.py); None when absent, taken at another batch, or taken on other kernel
    sources than the ones running now (csrc digest)."""
    import glob
    if batch != 128:
        return None, "PMC profile exists for 128 images per GPU only"
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_train_ian_b128.json")))
    if not files:
        return None, None
    try:
        from neural_photo_editor_amd import build as _b
        js = json.load(open(files[-1]))
        src = os.path.relpath(files[-1], ROOT)
        if js.get("csrc_digest") != _b._digest():
            return None, "%s is stale (csrc digest %s != current %s)" % (src, str(js.get("csrc_digest"))[:12], _b._digest()[:12])
        return float(js["hbm_bytes_per_update"]), "bytes per update, mean of update_gen and update_discrim (rocprofv3 PMC FETCH_SIZE x2 + WRITE_SIZE, %s)" % src
    except Exception:
        return None, None


def train_step_bench(batch, rank, world, iters=3, comm_mode=None):
    """ms per update_gen / update_discrim (train_IAN.py:309-329) of the full IAN at `batch` images per GPU.  The SAME entry
    at every world size: ian_train_step (csrc/ian_trainer.cpp); at N > 1 its collectives arrive through the ian_comm_ops
    table filled from torch.distributed (RCCL), SyncBN + MinibatchLayer all-gather on ("exact")."""
    import torch
    from neural_photo_editor_amd.trainer import Trainer, default_comm
    from neural_photo_editor_amd import synthetic as O
    P = O.make_train_params(O.make_params("IAN", 1))
    cfg_path = os.path.join(ROOT, "neural_photo_editor_amd", "configs", "IAN.py")
    comm = default_comm(mode=comm_mode)   # N > 1 on RCCL: the torch-free librccl filler (csrc/ian_comm_rccl.cpp), 2 or 1 communicators; or torch.distributed
    tr = Trainer(cfg_path, P, batch=batch, comm=comm, exact=True)
    rs = np.random.RandomState(50 + rank)
    X = torch.from_numpy(O.make_images(batch, seed=200 + rank)).cuda()
    Z = torch.from_numpy(rs.randn(batch, 100).astype(np.float32)).cuda()
    eps = torch.from_numpy(rs.randn(batch, 100).astype(np.float32)).cuda()
    out = {}
    if not os.environ.get("IAN_NO_AUTOTUNE"):
        tr.autotune()                                            # untimed: per-layer schedules for this batch on this GPU
    if world > 1:
        tr.measure_exposed = True
    for which in ("gen", "discrim"):
        tr.step(which, X, Z, eps, return_metrics=False)          # warm-up (schedules, workspaces, all-reduce plan)
        tr.step(which, X, Z, eps, return_metrics=False)          # second warm-up: first step with the overlapped all-reduce
        torch.cuda.synchronize()
        if world > 1:
            tr.measure_exposed = True                            # resets the counters: only the timed steps are averaged
        t = time.perf_counter()
        for _ in range(iters):
            tr.step(which, X, Z, eps, return_metrics=False)
        torch.cuda.synchronize()
        out["update_%s_ms" % which] = (time.perf_counter() - t) / iters * 1e3
        if world > 1:   # compute-stream stall at wait_all (the part of the gradient all-reduce backward did not hide -- that stall ONLY),
                        # and the time the compute stream spends inside the exact-mode all-gathers; means per update of this kind
            out.setdefault("allreduce_exposed_ms", {})[which] = tr.allreduce_exposed_ms()[which]
            out.setdefault("allgather_ms", {})[which] = tr.allgather_ms()[which]
    pair = out["update_gen_ms"] + out["update_discrim_ms"]
    flops = batch * (TRAIN_FLOP_PER_IMAGE["gen"] + TRAIN_FLOP_PER_IMAGE["discrim"])
    ach = flops / (pair * 1e-3) / 1e12
    out["roofline"] = {"bound": "mfma", "unit": "TFLOP/s", "peak": FP32_MFMA_PEAK_TFLOPS, "achieved": ach, "frac": ach / FP32_MFMA_PEAK_TFLOPS,
                       "traffic": train_pmc_traffic(batch)[0], "traffic_unit": train_pmc_traffic(batch)[1], "per_gpu": True,
                       "flop_per_image": {"update_gen": TRAIN_FLOP_PER_IMAGE["gen"], "update_discrim": TRAIN_FLOP_PER_IMAGE["discrim"]},
                       "frac_update_gen": batch * TRAIN_FLOP_PER_IMAGE["gen"] / (out["update_gen_ms"] * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                       "frac_update_discrim": batch * TRAIN_FLOP_PER_IMAGE["discrim"] / (out["update_discrim_ms"] * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                       "basis": "executed FLOP of the GEMM-shaped passes (5 E + 6 D per image for update_gen, 10 E + 3 D for update_discrim; "
                                "E = 1.316 G encoder+discriminator forward, D = 6.596 G decoder forward) over the measured update time"}
    out.update({"images_per_s": 2 * batch * world / (pair * 1e-3), "per_gpu_batch": batch, "global_batch": batch * world,
                "parallelism": ("single GPU" if world == 1 else
                                "dp%d, %s all-reduce of flat gradient groups in 16 MB buckets overlapped with backward, SyncBN statistics + "
                                "MinibatchLayer all-gather (exact)"
                                % (world, "RCCL" if os.environ.get("IAN_BENCH_BACKEND", "nccl") == "nccl" else os.environ["IAN_BENCH_BACKEND"] + " (test backend)")),
                "entry": "ian_train_step (C, csrc/ian_trainer.cpp)%s" % ("" if world == 1 else "; collectives through ian_comm_ops <- " + comm.filler),
                "collectives": None if world == 1 else comm.filler,
                "note": "one update_gen + one update_discrim (strict alternation, train_IAN.py:497-504) over synthetic data"})
    tr.close()
    return out


TRAIN_MARK = "@@IAN_TRAIN_LEG@@ "
COMM_LADDER = ("native2", "native1", "torch")     # == trainer.COMM_MODES: librccl with 2 communicators, with 1, torch.distributed


def train_child_main(args):
    """`bench.py --train-child MODE`: ONE attempt of the data-parallel training leg in its own process (one per rank, started by
    train_ladder below with RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* of its own rendezvous).  Rank 0 prints TRAIN_MARK + JSON."""
    import torch
    import torch.distributed as dist
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    mode = args.train_child
    backend = os.environ.get("IAN_BENCH_BACKEND", "gloo" if args.dry_run else "nccl")
    hang = mode in os.environ.get("IAN_BENCH_FAKE_HANG", "").split(",") and rank == world - 1   # tests: this rank never arrives
    if args.dry_run:
        dist.init_process_group(backend, rank=rank, world_size=world)
        if hang:
            time.sleep(3600)
        t = torch.ones(1)
        dist.all_reduce(t)
        out = {"dry_run": True, "ranks_seen": int(t.item()), "comm_mode": mode}
    else:
        torch.cuda.set_device(local % torch.cuda.device_count() if backend != "nccl" else local)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(backend, rank=rank, world_size=world)
        if hang:
            time.sleep(3600)
        out = train_step_bench(args.train_batch, rank, world, comm_mode=mode)
        out["comm_mode"] = mode
    dist.barrier()
    if rank == 0:
        print(TRAIN_MARK + json.dumps(out), flush=True)
    dist.destroy_process_group()
    return 0


def train_ladder(args, rank, world, local, agree, share):
    """The N > 1 training leg, hang-proof (round-5 verdict item 4).  No RCCL collective of this path had ever run with N > 1 when this
    was written, and its default uses two communicators on one device -- so every attempt runs in CHILD processes (one per rank, own
    rendezvous) under a per-attempt timeout: a child stuck in a collective is killed with its process group, the parents (whose own
    process group never touched the stuck communicator) agree on the outcome and walk down the ladder
        native2 (librccl, all-gathers on a second communicator) -> native1 (librccl, ONE communicator) -> torch (torch.distributed filler)
    before `timeout` is printed.  agree(ok) -> ok on every rank; share(obj) -> rank 0's obj on every rank.
    -> dict for the bench line: the winning attempt's numbers + comm_mode + the list of attempts."""
    import signal
    import subprocess
    attempts = []
    for mode in COMM_LADDER:
        port = share(_free_port() if rank == 0 else None)
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(local), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        for k in ("TORCHELASTIC_RUN_ID", "TORCHELASTIC_USE_AGENT_STORE"):   # the child rendezvous is its own (env://), not the launcher's store
            env.pop(k, None)
        cmd = [sys.executable, os.path.abspath(__file__), "--train-child", mode, "--train-batch", str(args.train_batch)]
        if args.dry_run:
            cmd.append("--dry-run")
        t0 = time.perf_counter()
        p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, start_new_session=True)
        try:
            out, _ = p.communicate(timeout=args.train_timeout)
            outcome = "ok" if p.returncode == 0 else "exit code %d" % p.returncode
        except subprocess.TimeoutExpired:
            try:
                os.killpg(p.pid, signal.SIGKILL)
            except OSError:
                pass
            out, _ = p.communicate()
            outcome = "timeout after %d s (killed)" % args.train_timeout
        payload = None
        for line in (out or b"").decode(errors="replace").splitlines():
            if line.startswith(TRAIN_MARK):
                payload = json.loads(line[len(TRAIN_MARK):])
        if rank == 0 and outcome == "ok" and payload is None:
            outcome = "no result line"
        ok_all = agree(outcome == "ok")
        attempts.append({"mode": mode, "outcome_rank0": outcome, "ok_on_all_ranks": bool(ok_all), "seconds": time.perf_counter() - t0})
        if ok_all:
            res = payload if rank == 0 else {}
            res["comm_mode"] = mode
            res["attempts"] = attempts
            return res
    return {"error": "the data-parallel training leg did not finish in any collective mode (headline unaffected)", "attempts": attempts}


def guarded_train_leg(args, rank, world, result, backend, local=0):
    """The training-step leg must never take the reconstruction headline down.  N = 1: in this process.  N > 1:
    train_ladder -- child processes per attempt, per-attempt timeout, three collective modes; plus a last-resort watchdog around
    the whole ladder that prints the stashed headline line with train_step = timeout and ends the process."""
    import threading
    import torch
    import torch.distributed as dist
    done = threading.Event()

    def bail():
        if done.is_set():
            return
        if rank == 0 and result is not None:
            result["train_step"] = {"error": "timeout: the data-parallel training leg did not finish within %d s (headline unaffected)" % (len(COMM_LADDER) * args.train_timeout + 120)}
            _finalize_secondary(result)
            print(json.dumps(result), flush=True)
        os._exit(0 if rank == 0 else 3)

    timer = None
    if world > 1:
        timer = threading.Timer(len(COMM_LADDER) * args.train_timeout + 120, bail)
        timer.daemon = True
        timer.start()
    try:
        ok = 1
        try:
            from neural_photo_editor_amd.trainer import Trainer  # noqa: F401  (import / library errors surface on every rank alike)
            free, _ = torch.cuda.mem_get_info()
            if free < (12 << 30):
                raise RuntimeError("only %.1f GB of HBM free" % (free / 2 ** 30))
        except Exception as exc:
            ok, why = 0, "%s: %s" % (type(exc).__name__, exc)
        dev = "cuda" if backend == "nccl" else "cpu"

        def agree(flag):
            t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return int(t.item()) == 1

        def share(obj):
            box = [obj]
            dist.broadcast_object_list(box, src=0)
            return box[0]

        if world > 1:
            if not agree(ok):
                return {"error": "skipped on all ranks: %s" % (why if not ok else "another rank could not set the training step up")}
            return train_ladder(args, rank, world, local, agree, share)
        if not ok:
            return {"error": why}
        try:
            return train_step_bench(args.train_batch, rank, world)
        except Exception as exc:
            return {"error": "%s: %s" % (type(exc).__name__, exc)}
    finally:
        done.set()
        if timer is not None:
            timer.cancel()


def _finalize_secondary(result):
    """roofline.secondary: the scalars of the other BASELINE.json configs, inside the object the driver's record keeps."""
    sec = {}
    e = result.get("edit_step") or {}
    if "p50_ms_one_call" in e:
        sec["edit_p50_ms"] = e["p50_ms_one_call"]
        sec["edit_frac"] = e["roofline"]["frac"]
        sec["edit_frac_executed_bytes"] = e["roofline"].get("frac_executed")
        sec["edit_p50_ms_two_calls"] = e.get("p50_ms")
    f = result.get("full_ian") or {}
    if "value" in f:
        sec["full_ian_value"] = f["value"]
        sec["full_ian_frac"] = (f.get("roofline") or {}).get("frac")
    t = result.get("train_step") or {}
    if "images_per_s" in t:
        sec["train_images_per_s"] = t["images_per_s"]
        sec["train_frac"] = t["roofline"]["frac"]
        sec["train_update_gen_ms"], sec["train_update_discrim_ms"] = t["update_gen_ms"], t["update_discrim_ms"]
        if "allreduce_exposed_ms" in t:
            sec["train_allreduce_exposed_ms"] = sum(t["allreduce_exposed_ms"].values())
    b = result.get("b1_recon") or {}
    if "device_ms" in b:
        sec["b1_recon_ms"] = b["device_ms"]
        sec["b1_recon_frac"] = b["roofline"]["frac"]
        sec["b1_recon_api_p50_ms"] = b.get("api_p50_ms")
    sec.update(result.pop("_bf16x3", None) or {})
    if isinstance(result.get("roofline"), dict):
        result["roofline"]["secondary"] = sec


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(d, arrays):
    """--dump-outputs: each array as d/<name>.npy in float32, DUMP_LIMIT_BYTES in all.  An array over its share keeps its leading
    entries along axis 0 (the same ones at every run: the inputs are seeded)."""
    os.makedirs(d, exist_ok=True)
    share = DUMP_LIMIT_BYTES // max(1, len(arrays))
    for name, a in arrays.items():
        a = np.asarray(a, np.float32)
        if a.nbytes > share:
            a = a[:max(1, share // max(1, a[:1].nbytes))]
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(a))


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn_ranks(n, argv):
    """`python bench.py --gpus N` with no launcher around it: re-run this file as N ranks (one per GPU) under
    torch.distributed.run -- exactly the command line the driver itself uses -- and relay rank 0's JSON line."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def _dry_run(args, rank, world):
    """The multi-rank control flow without the GPU: rendezvous (IAN_BENCH_BACKEND, default gloo here), barrier,
    max-over-ranks of the timed region, one JSON line from rank 0 carrying n_gpus = the number of ranks that ran."""
    import torch
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(os.environ.get("IAN_BENCH_BACKEND", "gloo"), rank=rank, world_size=world)
        dist.barrier()
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))
    dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    ranks = torch.ones(1, dtype=torch.float64)
    train = None
    if world > 1:
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        dist.all_reduce(ranks)
        if args.train:      # the retry ladder of the data-parallel training leg with stand-in children (tests/test_comm.py)
            def agree(flag):
                t = torch.tensor([1 if flag else 0], dtype=torch.int32)
                dist.all_reduce(t, op=dist.ReduceOp.MIN)
                return int(t.item()) == 1

            def share(obj):
                box = [obj]
                dist.broadcast_object_list(box, src=0)
                return box[0]
            train = train_ladder(args, rank, world, int(os.environ.get("LOCAL_RANK", "0")), agree, share)
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "64x64 IAN reconstructions/sec", "value": None, "unit": "reconstructions/s", "n_gpus": world,
                          "ranks_seen": int(ranks.item()), "steps": args.steps, "warmup": args.warmup, "ms_per_step": float(dt.item()) * 1e3,
                          "dry_run": True, "higher_is_better": True, "scaling": "weak", "train_step": train}))
    return 0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--arch", default="IAN_simple", choices=["IAN_simple", "IAN"])
    ap.add_argument("--full", action="store_true", help="also run the secondary measurements: roofline (profiled pass), box probe, split-bf16 "
                                                       "secondary, edit_step, b1_recon, cpu_baseline, full_ian, train_step (the --no-* options "
                                                       "below drop single ones)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps write what the last one computed as "
                                                                        "DIR/<name>.npy (float32; rank 0)")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default 64 for IAN_simple, 256 for IAN)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-edit", action="store_true")
    ap.add_argument("--no-bf16x3", action="store_true", help="skip the labelled split-bf16 secondary (roofline.secondary.bf16x3_*)")
    ap.add_argument("--no-full-ian", action="store_true", help="skip the full-IAN batch-256 block (BASELINE.json configs[2])")
    ap.add_argument("--train", action="store_true", help="also time the train_IAN.py step (default: only on 1 GPU)")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--train-batch", type=int, default=128, help="per-GPU minibatch of the training step (config 5: 1024 over 8 GPUs)")
    ap.add_argument("--train-timeout", type=int, default=240, help="N > 1: seconds after which ONE attempt of the training leg (one collective mode of "
                                                                 "the ladder native2 -> native1 -> torch) is killed and the next one tried; the headline line is printed whatever happens")
    ap.add_argument("--train-child", default=None, choices=list(COMM_LADDER), help=argparse.SUPPRESS)   # internal: one attempt of the N > 1 training leg
    ap.add_argument("--host-io", action="store_true", help="also time the API.py-style call: host numpy in, host numpy out (PCIe inclusive)")
    ap.add_argument("--dry-run", action="store_true", help="launch / rendezvous / aggregation plumbing only: no GPU work, value null "
                                                           "(tests/test_comm.py runs this with 2 gloo ranks on CPU)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.train_child:
        return train_child_main(args)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return _spawn_ranks(args.gpus, argv)        # no launcher around us: become one

    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:
        print("bench.py: --gpus %d but the launcher started %d rank(s); reporting n_gpus=%d" % (args.gpus, world, world), file=sys.stderr)
    if args.dry_run:
        return _dry_run(args, rank, world)
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    # IAN_BENCH_BACKEND=gloo lets the multi-rank control flow be exercised on a single-GPU box (ranks share cuda:0)
    backend = os.environ.get("IAN_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local % torch.cuda.device_count() if backend != "nccl" else local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(backend, rank=rank, world_size=world)

    from neural_photo_editor_amd import IAN
    from neural_photo_editor_amd import synthetic as O   # seeded synthetic parameters / images (no trained weights exist)

    stream = torch.cuda.current_stream().cuda_stream

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def measure(arch, B, steps, warmup, profile=True, keep_output=False):
        """W warm-up + K timed reconstruction steps of `arch` at batch B (inputs resident in HBM); on rank 0 and with `profile`
        also the profiled pass for the roofline; with `keep_output` the last timed step's output as host numpy ("_last").
        -> (model, params, dict)"""
        P = O.make_params(arch, seed=1)
        model = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=P)
        h = model.handle
        for kv in filter(None, os.environ.get("IAN_OPTS", "").split(",")):  # tuning knobs, e.g. IAN_OPTS=tg_cfg=0
            k, v = kv.split("=")
            h.set_option(k, int(v))
        x = torch.from_numpy(O.make_images(B, seed=100 + rank)).cuda()
        out = torch.empty_like(x)

        def step():
            h.call("ian_reconstruct", x, B, out, stream=stream)

        step()
        if not os.environ.get("IAN_NO_AUTOTUNE"):
            h.autotune(B, 1, stream=stream)  # untimed: pick tile shape / split-K per layer for this batch on this GPU
        for _ in range(warmup):
            step()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        barrier()
        t0 = time.perf_counter()
        evs[0].record()
        for i in range(steps):
            step()
            evs[i + 1].record()          # device-side step boundaries: no host synchronisation inside the timed region
        barrier()
        dt = time.perf_counter() - t0
        tmax = torch.tensor([dt], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        if world > 1:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        per = np.array([evs[i].elapsed_time(evs[i + 1]) for i in range(steps)])
        r = {"ms_per_step": dt / steps * 1e3, "value": world * B * steps / dt,
             "step_ms": {"p50": float(np.percentile(per, 50)), "p95": float(np.percentile(per, 95)), "min": float(per.min()),
                         "max": float(per.max()), "how": "HIP events on the launch stream between consecutive steps (device time)"}}
        if keep_output:
            r["_last"] = out.cpu().numpy()
        if rank == 0 and profile:
            # --- roofline: profiled pass (HIP events around every tapgemm launch, on the launch stream) ---
            nprof = min(steps, 20)
            h.profile_enable(True)
            for _ in range(nprof):
                step()
            pr = h.profile_read()
            h.profile_enable(False)
            launches = max(pr["tapgemm_launches"], 1)
            flops_per_launch = pr["tapgemm_flops"] / launches
            avg_ms = pr["tapgemm_ms"] / launches
            achieved = flops_per_launch / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
            traffic, traffic_src = pmc_traffic(arch, B)
            r["roofline"] = {"bound": "mfma", "kernel": "tapgemm_kernel (fp32 v_mfma_f32_32x32x2_f32)", "achieved": achieved,
                             "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / FP32_MFMA_PEAK_TFLOPS,
                             "traffic": traffic, "traffic_unit": ("bytes per launch (rocprofv3 PMC, %s)" % traffic_src) if traffic else traffic_src,
                             "flop_per_launch": flops_per_launch, "launches_per_step": launches / nprof,
                             "avg_launch_ms": avg_ms, "tapgemm_share_of_step": pr["tapgemm_ms"] / max(pr["total_ms"], 1e-9),
                             "whole_step_tflops": FLOP_EXECUTED[arch] * B / (r["ms_per_step"] * 1e-3) / 1e12,
                             "whole_step_frac_of_peak": FLOP_EXECUTED[arch] * B / (r["ms_per_step"] * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                             "whole_step_flop_basis": "executed %.3f GFLOP per reconstruction (algorithmic %.3f: SURVEY 8d counts every MDCL "
                                                      "branch separately, the kernels run one composite stencil)" % (FLOP_EXECUTED[arch] / 1e9, FLOP_PER_RECON[arch] / 1e9),
                             "whole_step_frac_algorithmic": FLOP_PER_RECON[arch] * B / (r["ms_per_step"] * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS}
        r["_x"], r["_out"] = x, out
        return model, P, r

    def bf16x3_secondary(arch, B, steps, warmup, ref_out, x):
        """LABELLED SECONDARY (rulings of the round-3 / round-5 verdicts: never `value`, `dtype` stays f32): the same reconstruction step
        with the opt-in split-bf16 tap-GEMMs (ian_set_option("tg_bf16x3", 1): three bf16 MFMAs per fp32 product, fp32 accumulation;
        kernels_tapgemm.hip tapgemm_bf16x3_kernel) -- what the part does inside the north star's 1e-4 tolerance when exact fp32 is not
        required.  Errors: against this run's exact-fp32 output on the same images, and against the reference-executed fixture."""
        try:
            P2 = O.make_params(arch, seed=1)
            m2 = IAN(os.path.join(ROOT, "neural_photo_editor_amd", "configs", arch + ".py"), True, params=P2)
            h2 = m2.handle
            h2.set_option("tg_bf16x3", 1)
            o2 = torch.empty_like(x)
            h2.call("ian_reconstruct", x, B, o2, stream=stream)
            if not os.environ.get("IAN_NO_AUTOTUNE"):
                h2.autotune(B, 1, stream=stream)
            for _ in range(warmup):
                h2.call("ian_reconstruct", x, B, o2, stream=stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                h2.call("ian_reconstruct", x, B, o2, stream=stream)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / steps
            h2.profile_enable(True)
            for _ in range(10):
                h2.call("ian_reconstruct", x, B, o2, stream=stream)
            pr = h2.profile_read()
            h2.profile_enable(False)
            a, b = o2.double(), ref_out.double()
            err32 = float((a - b).abs().max() / b.abs().max())
            fx = np.load(os.path.join(ROOT, "tests", "golden", "ref_%s.npz" % arch))
            got = m2.reconstruct(fx["x"]).astype(np.float64)
            errfx = float(np.abs(got - fx["xhat"]).max() / np.abs(fx["xhat"]).max())
            tf = pr["tapgemm_flops"] / max(pr["tapgemm_ms"], 1e-9) / 1e9
            m2.close()
            return {"bf16x3_value": B / (ms * 1e-3), "bf16x3_ms_per_step": ms, "bf16x3_tapgemm_avg_launch_ms": pr["tapgemm_ms"] / max(pr["tapgemm_launches"], 1),
                    "bf16x3_tapgemm_fp32_equivalent_tflops": tf, "bf16x3_frac_of_bf16_peak": 3.0 * tf / BF16_MFMA_PEAK_TFLOPS,
                    "bf16x3_max_rel_err_vs_fp32_same_inputs": err32, "bf16x3_max_rel_err_vs_reference_fixture": errfx,
                    "bf16x3_note": "opt-in tg_bf16x3 (off by default; batch-1 chains stay exact fp32): labelled secondary, never `value`; frac = 3 bf16 MFMA "
                                   "flops per fp32 flop over the %.0f TFLOP/s dense bf16 peak" % BF16_MFMA_PEAK_TFLOPS}
        except Exception as exc:
            return {"bf16x3_error": "%s: %s" % (type(exc).__name__, exc)}

    def box_probe():
        """Fingerprint of THIS box (round-5 verdict item 1b): what its fp32 matrix pipe sustains on a register-only MFMA loop at the
        launch length of one batch-64 layer (~200 us) and at ~700 us -- 50 ms of launches each.  Driver numbers from different boxes
        (+-7 % seen for one commit) become comparable through `whole_step_frac_of_sustained`."""
        from neural_photo_editor_amd import lib as L
        try:
            a = L.box_probe(900, 250, stream=stream)       # ~200 us per launch
            b = L.box_probe(3200, 70, stream=stream)       # ~700 us per launch
            return {"sustained_f32_mfma_tflops": a["tflops"], "launch_us": a["us_per_launch"],
                    "sustained_f32_mfma_tflops_long_launches": b["tflops"], "long_launch_us": b["us_per_launch"],
                    "frac_of_spec_peak": a["tflops"] / FP32_MFMA_PEAK_TFLOPS,
                    "how": "ian_box_probe: v_mfma_f32_32x32x2_f32 back to back from registers, 2 x 4 waves per CU, non-zero operands, no memory "
                           "traffic; 250 launches of 900 x 4 MFMAs per wave (~200 us: the launch length of one IAN_simple batch-64 layer) and 70 of 3200 x 4 (~700 us)"}
        except Exception as exc:
            return {"error": "%s: %s" % (type(exc).__name__, exc)}

    arch = args.arch
    B = args.batch or (64 if arch == "IAN_simple" else 256)
    model, P, main_r = measure(arch, B, args.steps, args.warmup, profile=args.full, keep_output=bool(args.dump_outputs) and rank == 0)
    h = model.handle
    ms_per_step, value = main_r["ms_per_step"], main_r["value"]
    box = box_probe() if (rank == 0 and args.full) else None   # right after the timed region: the clocks / temperature the headline just ran at
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"reconstruction": main_r["_last"]})
    main_r.pop("_last", None)
    main_x, main_out = main_r.pop("_x"), main_r.pop("_out")
    bf_sec = bf16x3_secondary(arch, B, min(args.steps, 50), 5, main_out, main_x) if (rank == 0 and args.full and not args.no_bf16x3) else {}
    if rank == 0 and box and "sustained_f32_mfma_tflops" in box and "roofline" in main_r:
        sus = box["sustained_f32_mfma_tflops"]
        main_r["roofline"]["frac_of_sustained"] = main_r["roofline"]["achieved"] / sus
        main_r["roofline"]["whole_step_frac_of_sustained"] = main_r["roofline"]["whole_step_tflops"] / sus

    result = None
    if rank == 0:
        roofline = main_r.get("roofline")
        edit = None
        if arch == "IAN_simple" and args.full and not args.no_edit:
            try:   # secondary measurement: never let it take the headline number down
                z = O.make_latents(1, seed=2)
                rgb = np.full((1, 3, 64, 64), -1.0, np.float32); rgb[:, 0] = 1.0
                c1, r1, c2, r2 = 26, 26, 30, 30
                model.imgradRGB(c1, r1, c2, r2, rgb, z)
                if not os.environ.get("IAN_NO_AUTOTUNE"):
                    h.autotune(1, 3)
                lat = []
                for i in range(120):
                    t = time.perf_counter()
                    g = model.imgradRGB(c1, r1, c2, r2, rgb, z)
                    z = z - 0.05 * g * (1 + (c2 - c1))
                    model.sample_at(z)
                    lat.append((time.perf_counter() - t) * 1e3)
                lat = np.array(lat[20:])
                os.environ["IAN_NO_DEC_CACHE"] = "1"   # every call recomputes the decoder forward (2 fwd + 1 bwd per step)
                lat2 = []
                for i in range(60):
                    t = time.perf_counter()
                    g = model.imgradRGB(c1, r1, c2, r2, rgb, z)
                    z = z - 0.05 * g * (1 + (c2 - c1))
                    model.sample_at(z)
                    lat2.append((time.perf_counter() - t) * 1e3)
                del os.environ["IAN_NO_DEC_CACHE"]
                # photo mode (NPE.py:218-231): brush step + blend; the blend runs on the device chained after the decoder
                from neural_photo_editor_amd import npe_ops
                IMG = np.uint8((O.make_images(1, seed=9)[0] + 1.0) * 127.5)
                RECON = model.sample_at_uint8(model.encode_images(np.asarray([npe_ops.to_tanh(IMG)], dtype=np.float32)))[0]
                ERROR = npe_ops.to_tanh(np.float32(IMG)) - npe_ops.to_tanh(np.float32(RECON))
                lat3 = []
                for i in range(80):
                    t = time.perf_counter()
                    g = model.imgradRGB(c1, r1, c2, r2, rgb, z)
                    z = z - 0.05 * g * (1 + (c2 - c1))
                    model.photo_blend(z, RECON, ERROR)
                    lat3.append((time.perf_counter() - t) * 1e3)
                # the whole brush event as ONE submission (ian_brush_step: gradient + latent update + decoder, one sync)
                lat5, lat6 = [], []
                for i in range(100):
                    t = time.perf_counter()
                    z, _ = model.brush_step(c1, r1, c2, r2, z, RGB=rgb, weight=0.05)
                    lat5.append((time.perf_counter() - t) * 1e3)
                for i in range(80):
                    t = time.perf_counter()
                    z = model.brush_step(c1, r1, c2, r2, z, RGB=rgb, weight=0.05, image=False, photo=(RECON, ERROR))[0]
                    lat6.append((time.perf_counter() - t) * 1e3)
                # the C caller's view of one event ("interactive entry"): bare ian_brush_step through ctypes on preallocated
                # buffers, with and without the 48 KB float image copied out (a UI takes the uint8 image: ian_decode_u8 / photo args)
                import ctypes as C
                zin, zout, ximg = np.ascontiguousarray(z[:1]), np.empty((1, 100), np.float32), np.empty((1, 3, 64, 64), np.float32)
                pz, pzo, px, prgb, null = [C.c_void_p(v.ctypes.data) for v in (zin, zout, ximg, rgb)] + [C.c_void_p(0)]
                fn, hh = h.lib.ian_brush_step, h._h

                def c_caller(img, n=160, skip=40):
                    ts = []
                    for _ in range(n):
                        t = time.perf_counter()
                        rc = fn(hh, c1, r1, c2, r2, prgb, pz, -0.05, float(1 + (c2 - c1)), pzo, null, px if img else null, None, null)
                        ts.append((time.perf_counter() - t) * 1e3)
                        assert rc == 0
                        zin[:] = zout
                    return float(np.percentile(ts[skip:], 50))
                c_img, c_noimg = c_caller(True), c_caller(False)
                # EXPERIMENT (round-5 verdict item 5a): a one-wave keep-warm kernel holds the interactive queue busy until the next event
                keep_warm = None
                try:
                    h.set_option("edit_keep_warm_us", 400)
                    kw = c_caller(False, n=200, skip=60)
                    h.set_option("edit_keep_warm_us", 0)
                    again = c_caller(False, n=200, skip=60)
                    keep_warm = {"p50_ms_c_caller_keep_warm_400us": kw, "p50_ms_c_caller_without_in_the_same_loop": again,
                                 "what": "option edit_keep_warm_us (off by default): after each event one wave spins on a flag in the mapped "
                                         "pinned block for up to 400 us; the next event releases it and launches its graph behind it"}
                except Exception as exc:
                    keep_warm = {"error": "%s: %s" % (type(exc).__name__, exc)}
                    try:
                        h.set_option("edit_keep_warm_us", 0)
                    except Exception:
                        pass
                z = zin.copy()
                # BASELINE.json configs[3] words it as an "Adam edit loop" (the reference brush is plain gradient
                # descent; Adam only exists in training): the same 100-step loop with an Adam update of the latent on the host
                za, ma, va, lat7 = z.copy(), np.zeros_like(z), np.zeros_like(z), []
                for i in range(100):
                    t = time.perf_counter()
                    g = model.imgradRGB(c1, r1, c2, r2, rgb, za)
                    ma = 0.9 * ma + 0.1 * g
                    va = 0.999 * va + 0.001 * g * g
                    za = (za - 0.01 * (ma / (1 - 0.9 ** (i + 1))) / (np.sqrt(va / (1 - 0.999 ** (i + 1))) + 1e-8)).astype(np.float32)
                    model.sample_at(za)
                    lat7.append((time.perf_counter() - t) * 1e3)
                h.set_option("edit_graph", 0)       # the same loop with eager launches (round-1 behaviour) for comparison
                lat4 = []
                for i in range(60):
                    t = time.perf_counter()
                    g = model.imgradRGB(c1, r1, c2, r2, rgb, z)
                    z = z - 0.05 * g * (1 + (c2 - c1))
                    model.sample_at(z)
                    lat4.append((time.perf_counter() - t) * 1e3)
                h.set_option("edit_graph", 1)
                edit = {"p50_ms": float(np.percentile(lat, 50)), "p95_ms": float(np.percentile(lat, 95)), "steps": len(lat),
                        "p50_ms_no_forward_cache": float(np.percentile(lat2[10:], 50)),
                        "p50_ms_eager_launches": float(np.percentile(lat4[10:], 50)),
                        "p50_ms_photo_mode": float(np.percentile(lat3[20:], 50)),
                        "p50_ms_one_call": float(np.percentile(lat5[20:], 50)), "p95_ms_one_call": float(np.percentile(lat5[20:], 95)),
                        "p50_ms_one_call_photo_mode": float(np.percentile(lat6[20:], 50)),
                        "p50_ms_c_caller": c_noimg, "p50_ms_c_caller_with_float_image": c_img, "keep_warm": keep_warm,
                        "update": "gradient descent (reference, NPE.py:199-209)",
                        "adam_variant": {"p50_ms": float(np.percentile(lat7[20:], 50)), "p95_ms": float(np.percentile(lat7[20:], 95)), "steps": 100,
                                         "update": "Adam(lr 0.01, 0.9, 0.999) on the host between imgradRGB and sample_at (two calls per step)"},
                        "roofline": {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS,
                                     "achieved": EDIT_STEP_BYTES / (float(np.percentile(lat5[20:], 50)) * 1e-3) / 1e9,
                                     "frac": EDIT_STEP_BYTES / (float(np.percentile(lat5[20:], 50)) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                     "achieved_executed": EDIT_STEP_BYTES_EXECUTED / (float(np.percentile(lat5[20:], 50)) * 1e-3) / 1e9,
                                     "frac_executed": EDIT_STEP_BYTES_EXECUTED / (float(np.percentile(lat5[20:], 50)) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                     "executed_basis": "151 MB: with the decoder-forward cache an event runs ONE decoder forward (77 MB) + one "
                                                       "backward-data sweep (74 MB); reported beside the 232 MB algorithmic basis",
                                     "traffic": b1_pmc_traffic("edit")[0], "traffic_unit": b1_pmc_traffic("edit")[1],
                                     "basis": "SURVEY 8(d): 232 MB algorithmic per brush event (2 decoder forwards + 1 backward-data at batch 1, "
                                              "weights uncached) over the p50 of one ian_brush_step call (host copies and the sync included); the "
                                              "event is latency-bound (13-17 dependent launches), not bandwidth-bound"},
                        "calls": "imgradRGB + sample_at through the API.py surface (host numpy in/out); batch-1 host calls replay captured "
                                 "hipGraphs on an internal stream; imgradRGB reuses the decoder activations sample_at left for the same "
                                 "latent; photo mode = imgradRGB + the device blend of NPE.py:218-231 (12 KB uint8 image back); "
                                 "one_call = ian_brush_step: gradient + latent update + decoder (+ blend) in one graph replay, one sync",
                        "includes": "host<->device copies of z, rgb, image"}
            except Exception as exc:
                edit = {"error": "%s: %s" % (type(exc).__name__, exc)}
                os.environ.pop("IAN_NO_DEC_CACHE", None)
                try:
                    h.set_option("edit_graph", 1)
                except Exception:
                    pass
        # ---- batch-1 reconstruction latency (BASELINE.json configs[0]'s GPU twin; NPE.py:257-261 encode_images -> sample_at) ----
        b1 = None
        if arch == "IAN_simple" and args.full and not args.no_edit:   # --no-edit (scripts/profile_round.sh): batch-64 launches only in the trace
            try:
                x1 = torch.from_numpy(O.make_images(1, seed=5)).cuda()
                o1 = torch.empty_like(x1)
                h.call("ian_reconstruct", x1, 1, o1, stream=stream)
                if not os.environ.get("IAN_NO_AUTOTUNE"):
                    h.autotune(1, 1, stream=stream)
                for _ in range(20):
                    h.call("ian_reconstruct", x1, 1, o1, stream=stream)
                reps = 200
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    h.call("ian_reconstruct", x1, 1, o1, stream=stream)
                e1.record()
                torch.cuda.synchronize()
                dev_ms = e0.elapsed_time(e1) / reps
                xh1 = O.make_images(1, seed=5)
                lat_api = []
                for _ in range(80):
                    t = time.perf_counter()
                    model.sample_at(model.encode_images(xh1))
                    lat_api.append((time.perf_counter() - t) * 1e3)
                ach = B1_RECON_BYTES / (dev_ms * 1e-3) / 1e9
                b1 = {"device_ms": dev_ms, "api_p50_ms": float(np.percentile(lat_api[20:], 50)), "api_p95_ms": float(np.percentile(lat_api[20:], 95)),
                      "roofline": {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS, "achieved": ach, "frac": ach / HBM_PEAK_GBS,
                                   "traffic": b1_pmc_traffic("b1_recon")[0], "traffic_unit": b1_pmc_traffic("b1_recon")[1],
                                   "basis": "SURVEY 8(d): 214 MB per batch-1 reconstruction (encoder 137 MB + decoder 77 MB, the weights), "
                                            "floor 26.9 us at 8 TB/s; device_ms = HIP-event time of %d back-to-back ian_reconstruct calls on "
                                            "device buffers / %d; api = encode_images + sample_at through the API.py surface (host numpy in/out, "
                                            "two calls, two syncs)" % (reps, reps)}}
            except Exception as exc:
                b1 = {"error": "%s: %s" % (type(exc).__name__, exc)}
        host_io = None
        if args.host_io:
            xh = O.make_images(B, seed=100 + rank)
            model.reconstruct(xh)
            t = time.perf_counter()
            for _ in range(10):
                model.reconstruct(xh)
            host_io = {"value": 10 * B / (time.perf_counter() - t), "unit": "reconstructions/s",
                       "note": "host numpy in -> host numpy out per call (pageable memory, PCIe inclusive); never `value`"}
        cpu = None
        if world == 1 and args.full and not args.no_cpu_baseline:
            try:
                cpu = cpu_baseline(arch, P, B if arch == "IAN_simple" else 32)
            except Exception as exc:
                cpu = {"error": "%s: %s" % (type(exc).__name__, exc)}
        result = {
            "metric": "64x64 IAN reconstructions/sec", "value": value, "unit": "reconstructions/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s encode->z->decode reconstruction, batch %d per GPU, inputs resident in HBM"
                                   % (arch, B), "parallelism": "replicas x%d (no data-path collective)" % world},
            "step_ms": main_r["step_ms"],
        }
        if args.full:
            result.update({"roofline": roofline, "box": box, "cpu_baseline": cpu, "edit_step": edit, "b1_recon": b1, "_bf16x3": bf_sec})
        if host_io:
            result["host_io"] = host_io
    # ---- BASELINE.json configs[2]: full IAN (MDC + RGB-Beta blocks), batch 256 per GPU, same protocol --------------
    if arch == "IAN_simple" and args.full and not args.no_full_ian:
        fsteps, fwarm = min(args.steps, 20), min(args.warmup, 5)
        try:
            fmodel, fP, fr = measure("IAN", 256, fsteps, fwarm)
            fr.pop("_x", None), fr.pop("_out", None)
            fmodel.close()
            del fmodel
            torch.cuda.empty_cache()
            full = {"workload": "IAN (IAN.py: MDBLOCKs + RGB-Beta head + MADE/IAF) encode->z->decode reconstruction, batch 256 per GPU, inputs resident in HBM",
                    "metric": "64x64 IAN reconstructions/sec", "value": fr["value"], "unit": "reconstructions/s", "steps": fsteps, "warmup": fwarm,
                    "ms_per_step": fr["ms_per_step"], "step_ms": fr["step_ms"], "roofline": fr.get("roofline")}
            if rank == 0 and world == 1 and not args.no_cpu_baseline:
                try:
                    full["cpu_baseline"] = cpu_baseline("IAN", fP, 32, budget_s=16.0)
                except Exception as exc:
                    full["cpu_baseline"] = {"error": "%s: %s" % (type(exc).__name__, exc)}
        except Exception as exc:
            full = {"error": "%s: %s" % (type(exc).__name__, exc)}
        if rank == 0 and result is not None:
            result["full_ian"] = full
    # ---- train_IAN.py step (BASELINE.json configs[4]): full IAN, data parallel, RCCL gradient all-reduce ----------
    train = None
    if args.full and not args.no_train:   # at N > 1 this is the data-parallel step: 128 images per GPU, SyncBN + MinibatchLayer all-gather ("exact")
        train = guarded_train_leg(args, rank, world, result, backend, local)
    if rank == 0 and result is not None and args.full:
        result["train_step"] = train
        _finalize_secondary(result)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(result), flush=True)


if __name__ == "__main__":
    sys.exit(main() or 0)

"""CPU tests of the training sequencer csrc/ian_trainer.cpp: tests/trainer_trace_main.cpp, a stand-alone program built under AddressSanitizer
and UBSan together with the trainer, stubs every ian_k_* / ian_layer_* / hip* symbol the trainer calls and prints the calls (see its head
comment for the line format).  The properties below hold the launch order, the streams and the bucket plan without a GPU and without a
golden file; the leak check runs at the end of every scenario."""
import bisect
import os
import re
import subprocess

import numpy as np
import pytest

from neural_photo_editor_amd import build as npe_build
from neural_photo_editor_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural_photo_editor_amd", "csrc")
DP = ("world=2", "overlap=1", "bucket_bytes=1048576")          # rank 0 of two, 1 MiB buckets
EVENT_CALLS = ("hipEventCreateWithFlags", "hipEventRecord", "hipStreamWaitEvent")


@pytest.fixture(scope="module")
def tracer(tmp_path_factory):
    """run(*args) -> Trace of one scenario; every scenario is traced once."""
    d = tmp_path_factory.mktemp("trainer_trace")
    exe, params = str(d / "trainer_trace"), str(d / "params.txt")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I" + npe_build._rocm_include(), os.path.join(ROOT, "tests", "trainer_trace_main.cpp"),
                    os.path.join(CSRC, "ian_trainer.cpp"), "-o", exe], check=True)
    shapes = dict(synthetic.param_shapes("IAN"))
    shapes.update(synthetic.train_param_shapes())
    with open(params, "w") as f:
        f.writelines("%s %d\n" % (k, int(np.prod(v))) for k, v in shapes.items())
    cache = {}

    def run(*args):
        if args not in cache:
            r = subprocess.run([exe, params, "--dump"] + list(args), capture_output=True, text=True,
                               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
            assert r.returncode == 0 and r.stderr == "", (args, r.stderr[-3000:])
            cache[args] = Trace(r.stdout)
        return cache[args]
    return run


class Trace:
    """text: the whole dump; steps[i]: the lines of step i as token lists; grad[g] = ordinal of group g's gradient allocation;
    params[g] = sorted (offset, numel) of the group's parameters (elements)."""

    def __init__(self, text):
        self.text = text
        self.steps, self.grad, self.numel, self.params = [], {}, {}, {0: [], 1: [], 2: [], 3: []}
        cur = None
        for line in text.splitlines():
            tok = line.split()
            if tok[0] == "==":
                if tok[1] == "group" and tok[2] != "3":
                    self.grad[int(tok[2])] = int(tok[4][1:].split("+")[0])
                    self.numel[int(tok[2])] = int(tok[7])
                elif tok[1] == "param":
                    self.params[int(tok[3])].append((int(tok[4]), int(tok[5])))
                cur = None
                if tok[1] == "step":
                    cur = []
                    self.steps.append(cur)
            elif cur is not None:
                cur.append(tok)
        for v in self.params.values():
            v.sort()
        self.group_of = {o: g for g, o in self.grad.items()}

    def grad_extents(self, tok):
        """(group, lo, hi) in elements of every parameter gradient a pointer argument of the call points into."""
        out = []
        for a in tok[1:]:
            m = re.fullmatch(r"#(\d+)\+(\d+)", a)
            if m and int(m.group(1)) in self.group_of:
                g, off = self.group_of[int(m.group(1))], int(m.group(2)) // 4
                lo, n = self.params[g][bisect.bisect_right(self.params[g], (off, 1 << 62)) - 1]
                assert lo <= off < lo + n, tok
                out.append((g, lo, lo + n))
        return out

    def sweep(self, i):
        """Step i up to the wait_all that closes its gradient all-reduce -> (lines, indices of the gradient all-reduces, indices of the
        other calls that point into a gradient buffer)."""
        lines = self.steps[i]
        end = max(k for k, t in enumerate(lines) if t[0] == "wait_all")
        red = [k for k in range(end) if lines[k][0] == "allreduce_sum" and self.grad_extents(lines[k])]
        wr = [k for k in range(end) if lines[k][0] != "allreduce_sum" and self.grad_extents(lines[k])]
        return lines[:end + 1], red, wr


def test_one_call_step_equals_the_piecewise_step(tracer):
    assert tracer("mode=step").text == tracer("mode=pieces").text
    assert len(tracer("mode=step").steps) == 4 and all(len(s) > 300 for s in tracer("mode=step").steps)


def test_overlap_wgrad_moves_streams_only(tracer):
    def same_launches(tr):
        return [[re.sub(r"^s\d+$", "s", a) for a in t] for s in tr.steps for t in s if t[0] not in EVENT_CALLS]
    on, off = tracer("overlap_wgrad=1"), tracer("overlap_wgrad=0")
    assert same_launches(on) == same_launches(off)
    assert all(t[-1] == "s0" for s in off.steps for t in s if t[0].startswith("ian_"))
    for lines in on.steps:
        # the weight gradients that land in a group's gradient buffer: nothing reads them before the regularisers.  (The MinibatchLayer's
        # goes to a scratch matrix that ian_k_mb_weight_bwd reads next, on the compute stream.)
        wg = [k for k, t in enumerate(lines) if t[0] == "ian_layer_backward_weight"]
        side = [k for k in wg if on.grad_extents(lines[k])]
        assert len(side) >= 15 and len(wg) - len(side) <= 3
        assert all(lines[k][-1] == ("s1" if k in side else "s0") for k in wg)
        first_update = min(k for k, t in enumerate(lines) if t[0] in ("ian_k_ortho", "ian_k_adam"))
        joins = [k for k in range(side[-1], first_update - 1) if lines[k][0] == "hipEventRecord" and lines[k][2] == "s1"
                 and lines[k + 1] == ["hipStreamWaitEvent", "s0", lines[k][1], "0"]]
        assert joins, "the compute stream joins the weight-gradient stream before the regularisers"


def check_planned_sweep(tr, i, moved):
    lines, red, wr = tr.sweep(i)
    ranges = {g: [] for g in moved}
    for k in red:
        (g, _, _), = tr.grad_extents(lines[k])
        lo = int(lines[k][1].split("+")[1]) // 4
        hi = lo + int(lines[k][2])
        ranges[g].append((lo, hi))
        for j in range(k + 1, len(lines)):   # in flight until wait_all: nothing touches a parameter that overlaps the bucket
            touched = [] if lines[j][0] == "allreduce_sum" else tr.grad_extents(lines[j])   # (other buckets: the tiling below)
            assert not any(gg == g and a < hi and b > lo for gg, a, b in touched), (lines[k], lines[j])
    for g in moved:
        r = sorted(ranges[g])
        assert r[0][0] == 0 and r[-1][1] == tr.numel[g] and all(a[1] == b[0] for a, b in zip(r, r[1:])), (g, r[:3])
    assert min(red) < max(wr), "at least one bucket is handed over before the last gradient write"
    after = [t for t in tr.steps[i][len(lines):] if tr.grad_extents(t)]
    assert after[0][0] == "ian_k_axpy" and tr.grad_extents(after[0])[0][0] == 1    # the L2 penalty on Z_params comes first
    assert not any(t[0] in ("ian_k_ortho", "ian_k_adam") for t in lines)


@pytest.mark.parametrize("exact", [1, 0])
def test_bucket_plan_per_update_kind(tracer, exact):
    tr = tracer("exact=%d" % exact, *DP)
    for i in (0, 1):       # first sweep of a kind: record the write order, reduce everything at the end
        lines, red, wr = tr.sweep(i)
        assert red and min(red) > max(wr)
    check_planned_sweep(tr, 2, (2, 1))    # update_gen moves decoder_params and Z_params
    check_planned_sweep(tr, 3, (0, 1))    # update_discrim moves encoder_params and Z_params


def test_plan_key_sends_a_sweep_back_to_record_mode(tracer):
    tr = tracer("exact=1", "which=0000", "@2:head6=0", *DP)
    early = []
    for i in range(4):
        lines, red, wr = tr.sweep(i)
        early.append(min(red) < max(wr))
    assert early == [False, True, False, True]
    check_planned_sweep(tr, 3, (2, 1))


def test_exact_mode_gathers(tracer):
    tr = tracer("exact=1", *DP)
    gathers = [[int(t[3]) for t in s if t[0] == "allgather"] for s in tr.steps]
    assert gathers[0] == gathers[2] and gathers[1] == gathers[3] and gathers[0] and gathers[1]
    # the float64 sums of a C-channel normalisation travel as 4 C floats: mu and logsigma (C = 100) share one message per direction
    assert all(g.count(800) == 2 and g.count(400) == 0 for g in gathers)
    assert not any(t[0] == "allgather" for s in tracer("exact=0", *DP).steps for t in s)

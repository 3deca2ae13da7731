"""The brush, clone and stroke calls' shared plan on the host: csrc/ian_edit_plan.h -- the layout of the uploaded table, the rows[k]
prefix and, per pass, the sequence of (step, first row, act, keep) -- compiled into a stand-alone program under AddressSanitizer and
UBSan (tests/edit_plan_main.cpp), which checks every case against the brute-force model "for k: the items with more than k points,
split into passes of `pass`".  What the program asserts per case: the columns never overlap and end exactly at the word count, every
(item, step) runs exactly once and in order, an item is blended exactly once, at its last step, a forward follows a blend exactly when
items are kept, and the residency is armed exactly for one pass with all counts equal.
This holds the plan, not edit_passes: the launches that follow from (act, keep) -- the blend of the tail, the forward again at batch
keep -- are HIP host code the program cannot reach, and the program counts them with edit_passes' own condition against the model's
count.  That the runtime enqueues them is pinned on the GPU by tests/test_gpu_sessions_stroke.py, _clone.py and _passes.py."""
import os
import re
import subprocess

import pytest

from session_helpers import ROOT

CSRC = os.path.join(ROOT, "neural_photo_editor_amd", "csrc")
BATCH_MAX = int(re.search(r"constexpr int BATCH_MAX = (\d+);", open(os.path.join(CSRC, "ian_rt_edit.inc")).read()).group(1))
COUNTS = ([1], [1, 1, 1], [3, 3, 3], [5, 3, 3, 1], [64], [64, 1], [4, 4, 2, 2, 2, 1], [1] * BATCH_MAX)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("edit_plan") / "edit_plan"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "edit_plan_main.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def run(exe, pass_, save, tips, own, counts, uniform=False):
    tail = ["u", len(counts), counts[0]] if uniform else ["v"] + list(counts)
    r = subprocess.run([exe] + [str(int(a)) if not isinstance(a, str) else a for a in [pass_, save, tips, own] + tail], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), (pass_, save, tips, own, counts, r.stdout, r.stderr[-2000:])
    return {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split()[1:])}


def passes(counts):
    n = len(counts)
    return sorted({1, 2, n, n + 1})


def test_every_case_agrees_with_the_brute_force_model(program):
    for counts in COUNTS:
        flags = ((0, 0), (1, 1)) if len(counts) == BATCH_MAX else ((0, 0), (1, 0), (0, 1), (1, 1))   # the long one: fewer runs, same code
        for p in passes(counts):
            for save, tips in flags:
                own = run(program, p, save, tips, True, counts)
                assert own["middles"] == sum(max(counts[o:o + p]) for o in range(0, len(counts), p)), (counts, p)
                assert own["resident"] == (len(counts) <= p and len(set(counts)) == 1), (counts, p)
                if len(set(counts)) == 1:   # a brush or a clone: one row per item, one word for all the counts; the same steps
                    shared = run(program, p, save, tips, False, counts, uniform=True)
                    assert {k: shared[k] for k in ("middles", "blends", "reforwards", "resident")} == {k: own[k] for k in shared if k != "words"}
                    assert shared["blends"] == -(-len(counts) // p) and shared["reforwards"] == 0   # once per pass, after the last step


def test_figures_worked_out_by_hand(program):
    # [5,3,3,1] in one pass: step 0 ends item 3 (forward at 3), step 2 ends items 1 and 2 (forward at 1), step 4 ends item 0
    r = run(program, 4, False, False, True, [5, 3, 3, 1])
    assert r == {"words": 4 + 12 + 6 + 7 * (4 + 3 + 3 + 1 + 1), "middles": 5, "blends": 3, "reforwards": 2, "resident": 0}
    # in passes of 2: [5,3] then [3,1], each with one forward again
    r = run(program, 2, True, True, True, [5, 3, 3, 1])
    assert r == {"words": 4 + 4 + 12 + 6 + 7 * 12 + 4, "middles": 5 + 3, "blends": 4, "reforwards": 2, "resident": 0}
    # a brush of 3 events, a clone of 3 events and 3 steps, a 3-point stroke on 3 sessions: the words differ, nothing else does
    assert run(program, 4, False, True, False, [1, 1, 1], uniform=True) == {"words": 3 + 9 + 21 + 3, "middles": 1, "blends": 1, "reforwards": 0, "resident": 1}
    assert run(program, 4, False, False, False, [3, 3, 3], uniform=True) == {"words": 3 + 9 + 21, "middles": 3, "blends": 1, "reforwards": 0, "resident": 1}
    assert run(program, 4, False, False, True, [3, 3, 3]) == {"words": 3 + 9 + 4 + 63, "middles": 3, "blends": 1, "reforwards": 0, "resident": 1}
    # the largest call: BATCH_MAX events in one pass
    assert run(program, BATCH_MAX, False, False, False, [1] * BATCH_MAX, uniform=True) == {"words": 11 * BATCH_MAX, "middles": 1, "blends": 1, "reforwards": 0,
                                                                                          "resident": 1}


def test_the_header_is_part_of_the_library_build():
    from neural_photo_editor_amd import build
    assert "ian_edit_plan.h" in build.HEADERS
    includes = re.findall(r"#include\s+(\S+)", open(os.path.join(CSRC, "ian_edit_plan.h")).read())
    assert includes == ["<cstddef>", "<cstdint>"]   # plain C++: nothing of the runtime enters the stand-alone program

"""CPU tests of the tap-GEMM planner csrc/ian_tg_plan.h (tiles, per-tile tap lists, K ranges, slabs, item order, the launch model):
tests/tg_plan_main.cpp, a stand-alone program built under AddressSanitizer and UBSan, plans every geometry for every tile shape, batch,
Cin, split limit and row order and checks each plan by brute force over (valid row, tap) -- see its head comment for the list."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural_photo_editor_amd", "csrc")
NTILES, PLANS_PER_TILE = 8, 6 * 3 * 3 * 2          # tile shapes; batches x Cin x limits x row orders


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tg_plan") / "tg_plan"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "tg_plan_main.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def run_geometry(exe, name):
    """One process per tile shape, side by side -> the five counters summed over the shapes."""
    def one(cfg):
        r = subprocess.run([exe, name, str(cfg)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (name, cfg, r.stderr[-2000:])
        head, *nums = r.stdout.split()
        assert head == "ok" and int(nums[0]) == PLANS_PER_TILE, r.stdout
        return [int(v) for v in nums]
    with ThreadPoolExecutor(NTILES) as pool:
        return [sum(col) for col in zip(*pool.map(one, range(NTILES)))]


# 5x5 stride-2 convolutions 8 -> 4, 16 -> 8, 64 -> 32; transposed 5x5 stride-2 (four parity classes) 4 -> 8, 16 -> 32; the 3x3 list with
# dilations 1, 2, 4, 8 on a 4x4 and a 16x16 map
@pytest.mark.parametrize("name", ["conv8", "conv16", "conv64", "deconv4", "deconv16", "dil4", "dil16"])
def test_every_plan_holds_by_brute_force(plan_program, name):
    plans, skipped, one_pos, kept, border_unsplit = run_geometry(plan_program, name)
    assert plans == NTILES * PLANS_PER_TILE
    assert skipped > 0 and one_pos > 0, "the sweep must reach tiles that skip taps and tiles of one position"
    if name in ("deconv4", "deconv16", "dil4", "dil16"):
        assert border_unsplit > 0, "... and border tiles that stay whole under a limit that cuts the interior ones"


def test_a_tile_with_nothing_inside_the_image_keeps_one_tap(plan_program):
    """The eight taps of dilation 8 alone on a 4x4 map: no row reads inside the image, every position-major list would be empty."""
    plans, skipped, one_pos, kept, border_unsplit = run_geometry(plan_program, "ring4")
    assert plans == NTILES * PLANS_PER_TILE and kept > 0 and skipped > 0


def test_the_launch_model_on_the_batch_64_layers(plan_program):
    """Makespan with skipping / without, best limit each, per layer and tile: nothing gets longer, the 32- and 16-pixel layers gain
    nothing (one round of workgroups lasts as long as an interior tile), the three K-split layers gain 6 to 23 %."""
    r = subprocess.run([plan_program, "model"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    ratio = {}
    for line in r.stdout.splitlines():
        layer, tile, v = line.split()
        ratio[layer, tile] = float(v)
    assert len(ratio) == 18 and all(v <= 1.0 for v in ratio.values()), ratio
    for tile in ("64x64", "128x64", "128x128"):
        assert ratio["enc_conv2", tile] == 1.0 and ratio["dec_conv3", tile] == 1.0
        assert 0.75 < ratio["enc_conv4", tile] < 0.92 and 0.75 < ratio["dec_conv1", tile] < 0.90 and 0.90 < ratio["dec_conv2", tile] < 0.95, ratio

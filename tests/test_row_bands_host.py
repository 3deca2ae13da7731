"""CPU tests of the row-band rule csrc/ian_row_bands.h (how many bands of rows head6_kernel and deconv_small_kernel cut an image into):
tests/row_bands_main.cpp, a stand-alone program built under AddressSanitizer and UBSan -- see its head comment."""
import os
import subprocess

import pytest

import row_band_cases as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural_photo_editor_amd", "csrc")
HEAD = dict(gran=1, min_rows=8)      # the head walks single rows and re-reads a halo of 4 rows per side: half a band keeps 2 x 4 rows
DEC_OUT = dict(gran=2, min_rows=0)   # dec_out walks row pairs; one halo row per side whatever the band


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("row_bands") / "row_bands"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "row_bands_main.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (args, r.stderr[-2000:])
    return r.stdout


def bands(exe, kind, H, wgs, batches):
    return [int(v) for v in run(exe, "bands", kind["gran"], kind["min_rows"], H, wgs, *batches).split()]


def test_defaults_give_8_4_2_1_bands(program):
    """head_wgs = dec_out_wgs = 256: the head at 64 rows and dec_out at 32 input rows run 8, 4, 2 and 1 bands at 8, 64, 128 and 256
    images; 4 bands begin at 64 images (63 x 4 < 256), 2 at 128, 1 at 256."""
    for kind, H in ((HEAD, 64), (DEC_OUT, 32)):
        assert bands(program, kind, H, 256, [8, 64, 128, 256]) == [8, 4, 2, 1]
        assert bands(program, kind, H, 256, [1, 2, 5, 24, 32, 33, 63, 127, 255, 257]) == [8, 8, 8, 8, 8, 8, 8, 4, 2, 1]


def test_a_32_row_head_never_exceeds_4_bands(program):
    """Half of a band keeps 2 x halo = 8 rows: 32 rows stop at 4 bands whatever the batch and the target."""
    for wgs in (1, 8, 256, 100000):
        got = bands(program, HEAD, 32, wgs, range(1, 300))
        assert max(got) <= 4, (wgs, max(got))
    assert bands(program, HEAD, 32, 256, [1, 8, 64, 128, 256]) == [4, 4, 4, 2, 1]


@pytest.mark.parametrize("kind,H,batches,table", [(DEC_OUT, 32, RB.DEC_OUT_BATCHES, RB.DEC_OUT_WGS), (HEAD, 64, RB.HEAD_BATCHES, RB.HEAD_WGS),
                                                  (HEAD, 64, (RB.TRAIN_HEAD_BATCH,), RB.TRAIN_HEAD_WGS)], ids=["dec_out", "head", "train_head"])
def test_the_gpu_tests_pairs_reach_every_band_count(program, kind, H, batches, table):
    """What keeps the GPU sweeps from passing vacuously: each (batch, target) pair gives exactly the band count it is listed under."""
    assert sorted(table) == [1, 2, 4, 8]
    for want, wgs in table.items():
        assert bands(program, kind, H, wgs, batches) == [want] * len(batches), (want, wgs)


def test_rule_is_the_three_loops_it_replaced_and_bands_divide_the_rows(program):
    """Over a grid of (batch, target, rows, halo): the function is the loop of each call site, gives 1 / 2 / 4 / 8, divides the rows
    (H % bands == 0; whole row pairs for dec_out: H % (2 bands) == 0) and halves no further than the target asks."""
    head, *nums = run(program, "sweep").split()
    cases, b1, b2, b4, b8 = (int(v) for v in nums)
    assert head == "ok" and cases == 10 * 11 * 300 * 6 and b1 + b2 + b4 + b8 == cases
    assert min(b1, b2, b4, b8) > 1000, "the grid must reach every band count"


def test_band_walks_cover_every_output_row_once(program):
    """The row walk of both kernels replayed on the CPU for 1, 2, 4 and 8 bands (the program checks that every output row receives each
    of its input rows once, in ascending order, leaves once, and shares its ring slot with no other open row).  dec_out at 32 input rows:
    the row span r_end - r_begin before the parity adjustment is 6 / 10 / - / 32 for an inner band at 8 / 4 / 2 / 1 bands and
    5 / 9 / 17 / - for an edge band, so 8 and 4 bands mix the even path (inner) with --r_begin (last band) and ++r_end (first band),
    2 bands take only the two odd paths and 1 band only the even one."""
    rows = [line.split() for line in run(program, "walk").splitlines()]
    dec = {int(r[2]): [int(v) for v in r[3:]] for r in rows if r[0] == "dec_out"}
    #            inner span, edge span, bands on the even path, --r_begin, ++r_end
    assert dec == {8: [6, 5, 6, 1, 1], 4: [10, 9, 2, 1, 1], 2: [-1, 17, 0, 1, 1], 1: [32, -1, 1, 0, 0]}
    head = {(int(r[1]), int(r[2])): [int(v) for v in r[3:5]] for r in rows if r[0] == "head"}
    assert head == {(64, 1): [64, -1], (64, 2): [-1, 36], (64, 4): [24, 20], (64, 8): [16, 12],
                    (32, 1): [32, -1], (32, 2): [-1, 20], (32, 4): [16, 12]}

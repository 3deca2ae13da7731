"""The three kernels that produce the picture, each held to the float64 evaluation of its OWN stage at every way it partitions its work:
deconv_small_kernel<3, BAL> (IAN_simple's dec_out: 1 / 2 / 4 / 8 row bands x the 16 x 16 and the 32 x 32 MFMA tiling) with the two
kernels it replaced, and head6_kernel + head_tail_kernel (the RGB-Beta head of the full IAN: 1 / 2 / 4 / 8 row bands, fused vs per-layer,
both sides of the batch threshold).

The reference of a case is the stage alone, in float64 on the CPU (the oracle's layer functions with float64 parameters), applied to the
input the device itself holds for that stage -- the producing slot read back after the run --, so the error measured is this stage's and
nothing upstream can hide or mimic it.  Band counts are reached at a handful of images through the options dec_out_wgs / head_wgs;
tests/test_row_bands_host.py pins on the CPU that the (batch, value) pairs of tests/row_band_cases.py give exactly 1, 2, 4 and 8 bands.
Every comparison prints its figure (pytest -s)."""
import contextlib
import os

import numpy as np
import pytest

import row_band_cases as RB
from oracle import ian_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "neural_photo_editor_amd", "configs")
TOL_BLOCK = 2e-5   # a single building block's forward values (tests/README.md)
TOL_ACT = 1e-4     # float32 activations: the head's bar -- its beta division amplifies the error of the sigmoids it divides
TOL_SPLIT = 1e-5   # two float32 evaluations of one sum that associate it differently (tests/test_gpu_tap_skip.py)
DEFAULTS = {"dec_out_wgs": 256, "dec_out_bal": 1, "dec_out_mfma": 1, "dec_out_px": 1, "head_wgs": 256, "head_fused": 1, "head_fused_min_n": 8}
BANDS = (1, 2, 4, 8)

_models, _refs, _runs = {}, {}, {}


def model_for(arch):
    if arch not in _models:
        from neural_photo_editor_amd import IAN
        P = O.make_params(arch, 1)
        _models[arch] = (IAN(os.path.join(CFG, arch + ".py"), True, params=P), {k: np.asarray(v, np.float64) for k, v in P.items()})
    return _models[arch]


@contextlib.contextmanager
def options(m, **opts):
    assert set(opts) <= set(DEFAULTS)
    try:
        for k, v in opts.items():
            m.handle.set_option(k, v)
        yield
    finally:
        for k in opts:
            m.handle.set_option(k, DEFAULTS[k])


def stage_reference(key, x, fn):
    """float64 stage output for the device-read input x; computed once per input (every option setting of a batch reads the same bits back)."""
    if key not in _refs or not np.array_equal(_refs[key][0], x):
        _refs[key] = (x, fn(x.astype(np.float64)))
    return _refs[key][1]


def dec_out_reference(x):
    P64 = model_for("IAN_simple")[1]
    return np.tanh(O.deconv5s2(x, P64["dec_out.W"], None, True))          # IAN_simple.py:171-181: no bias, tanh


def head_reference(x):
    """IAN.py:183-207 from the 128-channel map to the NCHW image."""
    P64, sc = model_for("IAN")[1], [2, 3, 4]
    R = O.act_fn("sigmoid", O.mdcl(x, P64, "R", sc))
    G = O.act_fn("sigmoid", O.mdcl(x, P64, "G_a", sc) + O.mdcl(R, P64, "G_b", sc))
    B = O.act_fn("sigmoid", O.mdcl(x, P64, "B_a", sc) + O.mdcl(np.concatenate([R, G], 1), P64, "B_b", sc))
    return np.concatenate([O.beta_layer(R[:, 0:1], R[:, 1:2]), O.beta_layer(G[:, 0:1], G[:, 1:2]), O.beta_layer(B[:, 0:1], B[:, 1:2])], 1)


def run_stage(arch, n, **opts):
    """One decoder run under the options -> (the stage's input as the device holds it, the image, the stage's float64 reference)."""
    key = (arch, n) + tuple(sorted(opts.items()))
    if key not in _runs:
        m, _ = model_for(arch)
        z = O.make_latents(n, seed=70 + n)
        with options(m, **opts):
            img = m.sample_at(z)
            x = m.activation("dec_conv3" if arch == "IAN_simple" else "dec_conv4", n)
        assert x.shape == ((n, 128, 32, 32) if arch == "IAN_simple" else (n, 128, 64, 64)) and img.shape == (n, 3, 64, 64)
        if (arch, n) in _refs and np.array_equal(_refs[arch, n][0], x):
            x = _refs[arch, n][0]                                        # one copy of the input per batch
        _runs[key] = (x, img)
    x, img = _runs[key]
    return x, img, stage_reference((arch, n), x, dec_out_reference if arch == "IAN_simple" else head_reference)


def check_stage(what, img, ref, tol):
    """Max-norm error of the stage, with the worst output row named: a fault at a band edge shows as one row."""
    d = np.abs(img.astype(np.float64) - ref)
    per_row = d.max(axis=(0, 1, 3)) / np.abs(ref).max()
    err, row = float(per_row.max()), int(per_row.argmax())
    print("%s: max-norm error %.3g, worst output row %d" % (what, err, row))
    bad = [(int(r), float("%.3g" % per_row[r])) for r in np.nonzero(per_row >= tol)[0]]
    assert np.isfinite(img).all() and err < tol, "%s: max-norm error %.3g at output row %d, tolerance %g; rows over it: %s" % (what, err, row, tol, bad)
    return err


def gap(what, a, b, ref):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64)).max(axis=(0, 1, 3)) / np.abs(ref).max()
    print("%s: gap %.3g, worst output row %d" % (what, float(d.max()), int(d.argmax())))
    return float(d.max()), int(d.argmax())


# ---------------------------------------------------------------------------------------------------------------------------------------
# dec_out of IAN_simple
# ---------------------------------------------------------------------------------------------------------------------------------------
def dec_out_opts(bands, bal):
    return {"dec_out_wgs": RB.DEC_OUT_WGS[bands], "dec_out_bal": bal}


@pytest.mark.parametrize("bal", [1, 0])
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("n", RB.DEC_OUT_BATCHES)
def test_dec_out_every_band_count_and_tiling_vs_float64(n, bands, bal):
    """deconv_small_kernel<3, BAL> at n = 4 (the smallest batch on the matrix cores) and n = 5 (blockIdx.x / bands over an odd image count):
    with 32 input rows, 8 and 4 bands mix the even row-pair path (inner bands) with ++r_end (first band) and --r_begin (last band), 2 bands
    take only the two odd paths, 1 band only the even one."""
    x, img, ref = run_stage("IAN_simple", n, **dec_out_opts(bands, bal))
    check_stage("dec_out n=%d, %d bands, dec_out_bal=%d" % (n, bands, bal), img, ref, TOL_BLOCK)


@pytest.mark.parametrize("bal", [1, 0])
@pytest.mark.parametrize("n", RB.DEC_OUT_BATCHES)
def test_dec_out_band_counts_agree(n, bal):
    """Across band counts within one tiling.  Read in deconv_small_kernel: Y of an input row does not depend on the band, but the taps of
    a row PAIR (r, r + 1) are summed in registers first (s7[2 ql + ky] over ql) and the pair's sum is added to the ring, so an output row
    with input rows q - 1, q, q + 1 is (a + b) + c when a pair starts at q - 1 and a + (b + c) when one starts at q: where the pairs start
    decides the order.  They start on an even row in the first band (r_begin = 0), in the last band (r_begin = q0 - 2 after --r_begin) and
    with one band, on an odd row (q0 - 1) in every inner band.  So: the output rows of the first and of the last band of the 8-band split
    (8 rows each, inside the first / last band of every coarser split) are bitwise the same for 1, 2, 4 and 8 bands, and so is the whole
    picture with 2 bands (a first and a last band, no inner one); everything else is held to the re-association bar 1e-5."""
    runs = {b: run_stage("IAN_simple", n, **dec_out_opts(b, bal)) for b in BANDS}
    x1, img1, ref = runs[1]
    for b in BANDS[1:]:
        x, img, _ = runs[b]
        assert np.array_equal(x, x1), "the stage's input differs between two runs of the same latents"
        g, row = gap("dec_out n=%d dec_out_bal=%d: %d bands vs 1" % (n, bal, b), img, img1, ref)
        assert g < TOL_SPLIT, "%d bands vs 1: gap %.3g at output row %d" % (b, g, row)
        assert b != 2 or np.array_equal(img, img1), "2 bands walk even row pairs throughout and must be bitwise the picture of 1 band"
        assert np.array_equal(img[:, :, :8], img1[:, :, :8]) and np.array_equal(img[:, :, 56:], img1[:, :, 56:]), \
            "%d bands: the first / last 8 output rows walk the same even row pairs as one band and must be bitwise the same" % b


@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("n", RB.DEC_OUT_BATCHES)
def test_dec_out_tilings_agree(n, bands):
    """The 16 x 16 blocks (dec_out_bal = 1: K in steps of 4) and the 32 x 32 blocks (K in steps of 2) accumulate the 128 channels in
    different orders: 1e-5."""
    _, a, ref = run_stage("IAN_simple", n, **dec_out_opts(bands, 1))
    _, b, _ = run_stage("IAN_simple", n, **dec_out_opts(bands, 0))
    g, row = gap("dec_out n=%d, %d bands: dec_out_bal 1 vs 0" % (n, bands), a, b, ref)
    assert g < TOL_SPLIT, "gap %.3g at output row %d" % (g, row)


@pytest.mark.parametrize("n", RB.DEC_OUT_BATCHES)
def test_dec_out_tile_kernel_without_the_matrix_cores(n):
    """dec_out_mfma = 0 sends batches >= 4 to deconv_out_nchw_kernel (kernels_misc.hip: 8 x 8 input tiles, channels split over 8 waves)."""
    x, img, ref = run_stage("IAN_simple", n, dec_out_mfma=0)
    check_stage("dec_out n=%d, dec_out_mfma=0" % n, img, ref, TOL_BLOCK)
    g, row = gap("dec_out n=%d: dec_out_mfma 0 vs 1" % n, img, run_stage("IAN_simple", n, **dec_out_opts(8, 1))[1], ref)
    assert g < TOL_SPLIT, "gap %.3g at output row %d" % (g, row)


@pytest.mark.parametrize("px", [1, 0])
def test_dec_out_below_the_matrix_core_batch(px):
    """n = 3: deconv_out_px_kernel (8 lanes per output pixel, default) and deconv_out_nchw_kernel (dec_out_px = 0)."""
    x, img, ref = run_stage("IAN_simple", 3, dec_out_px=px)
    check_stage("dec_out n=3, dec_out_px=%d" % px, img, ref, TOL_BLOCK)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the RGB-Beta head of the full IAN
# ---------------------------------------------------------------------------------------------------------------------------------------
def head_opts(bands):
    return {"head_fused_min_n": 1, "head_wgs": RB.HEAD_WGS[bands]}


@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("n", RB.HEAD_BATCHES)
def test_head_every_band_count_vs_float64(n, bands):
    """head6_kernel + head_tail_kernel at 3 and 5 images (head_fused_min_n = 1 lets them take the fused launch) against float64 R, G_a, G_b,
    B_a, B_b, the sigmoids and the three beta layers.  1e-4, the bar on float32 activations (2e-5 is a building block's bar; the beta
    division amplifies the error of its operands and nothing in the project pins a tighter figure for it).  Measured on the MI355X: 3.6e-7
    at 3 images and 4.1e-7 at 5, the same for every band count."""
    x, img, ref = run_stage("IAN", n, **head_opts(bands))
    check_stage("head n=%d, %d bands" % (n, bands), img, ref, TOL_ACT)


@pytest.mark.parametrize("n", RB.HEAD_BATCHES)
def test_head_band_counts_are_bitwise_the_same(n):
    """Read in head6_kernel: Y of an input row (the MFMA contraction) and the nine per-dy sums sd[g] built from it depend on the row alone;
    an output row y adds sd of the input rows y - 4 .. y + 4 to a ring slot that starts at zero, one row per loop step, in ascending row
    order -- a band only decides where the walk starts (r_begin <= y - 4 or the image's first row) and which rows it owns.  head_tail_kernel
    runs one workgroup per image on the compact map.  No summation order depends on the band: the pictures are identical."""
    runs = {b: run_stage("IAN", n, **head_opts(b)) for b in BANDS}
    x1, img1, _ = runs[1]
    for b in BANDS[1:]:
        x, img, _ = runs[b]
        assert np.array_equal(x, x1), "the stage's input differs between two runs of the same latents"
        diff = np.nonzero((img != img1).any(axis=(0, 1, 3)))[0]
        assert diff.size == 0, "%d bands vs 1: output rows %s differ" % (b, diff.tolist())


@pytest.mark.parametrize("n", RB.HEAD_BATCHES)
def test_head_fused_equals_the_per_layer_path(n):
    """head_fused = 1 (two launches) against head_fused = 0 (R, G_a, G_b, B_a, B_b, concat and beta as separate launches), same latents:
    1e-5 on the image, and the per-layer path within 1e-4 of the float64 stage as well."""
    x0, per_layer, ref = run_stage("IAN", n, head_fused=0)
    check_stage("head n=%d, head_fused=0" % n, per_layer, ref, TOL_ACT)
    x1, fused, _ = run_stage("IAN", n, **head_opts(8))
    assert np.array_equal(x0, x1), "the stage's input differs between two runs of the same latents"
    g, row = gap("head n=%d: fused vs per-layer" % n, fused, per_layer, ref)
    assert g < TOL_SPLIT, "gap %.3g at output row %d" % (g, row)


@pytest.mark.parametrize("n", [7, 8])
def test_head_on_both_sides_of_the_batch_threshold(n):
    """head_fused_min_n at its default 8: 7 images take the per-layer path, 8 the fused one; each within 1e-4 of its own float64 stage.
    That each batch takes the path named is shown bit for bit: 7 images give the picture of head_fused = 0, 8 images the picture of
    head_fused_min_n = 1."""
    x, img, ref = run_stage("IAN", n)
    check_stage("head n=%d, defaults" % n, img, ref, TOL_ACT)
    x2, forced, _ = run_stage("IAN", n, **({"head_fused": 0} if n < 8 else {"head_fused_min_n": 1}))
    assert np.array_equal(x, x2) and np.array_equal(img, forced)

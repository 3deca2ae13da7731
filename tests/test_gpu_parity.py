"""GPU parity tests: the HIP path (through the C ABI, via the ctypes host class) against the CPU oracle
and the committed golden vectors.  Tolerance for float32 activations is the north star's 1e-4 relative
(max-abs-error / max-abs-reference); MADE masks are checked bit-exactly in test_host.py."""
import os

import numpy as np
import pytest

from oracle import ian_oracle as O
from oracle.torch_twin import TorchTwin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "neural_photo_editor_amd", "configs")
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-4        # north-star tolerance on float32 activations
TOL_GRAD = 1e-5   # brush gradients vs a float64 reference: measured maxima 6.3e-7 (IAN_simple) / 9.4e-7 (IAN) over six patches
                  # against the reference-executed T.grad (tests/test_gpu_reference_pinned.py, round 3); bar = ~10x that


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(np.asarray(b)).max() + 1e-30))


def red_rgb():
    rgb = np.full((1, 3, 64, 64), -1.0, np.float32)
    rgb[:, 0] = 1.0
    return rgb


_cache = {}


def model_for(arch):
    if arch not in _cache:
        from neural_photo_editor_amd import IAN
        P = O.make_params(arch, 1)
        _cache[arch] = (IAN(os.path.join(CFG, arch + ".py"), True, params=P), O.Oracle(arch, P), P)
    return _cache[arch]


def test_native_library_is_loaded():
    """The product path is libian.so; make the loaded-library evidence explicit."""
    model_for("IAN_simple")
    maps = open("/proc/self/maps").read()
    assert "libian.so" in maps


@pytest.mark.parametrize("arch", O.ARCHS)
def test_golden_encode_decode(arch):
    m, orc, _ = model_for(arch)
    g = np.load(os.path.join(GOLD, "%s_seed1.npz" % arch))
    x = O.make_images(2)
    assert rel(m.Zfn(x), g["zpre"]) < TOL
    assert rel(m.encode_images(x), g["z"]) < TOL
    assert rel(m.sample_at(g["z"]), g["xhat"]) < TOL
    assert rel(m.sample_at(g["z_sample"]), g["x_sample"]) < TOL
    assert rel(m.reconstruct(x), g["xhat"]) < TOL
    assert rel(m.Z_IAF_fn(g["zpre"]), g["z"]) < TOL
    assert rel(m.sample(g["zpre"]), g["xhat"]) < TOL
    assert m.get_zdim() == 100


@pytest.mark.parametrize("arch", O.ARCHS)
@pytest.mark.parametrize("n", [1, 3, 5, 33])
def test_ragged_batches_vs_oracle(arch, n):
    m, orc, _ = model_for(arch)
    x = O.make_images(n, seed=10 + n)
    z = m.encode_images(x)
    zr = orc.encode_images(x)
    assert z.shape == (n, 100) and rel(z, zr) < TOL
    xh = m.sample_at(zr)
    assert xh.shape == (n, 3, 64, 64) and rel(xh, orc.sample_at(zr)) < TOL


@pytest.mark.parametrize("arch", O.ARCHS)
def test_every_layer_activation(arch):
    m, orc, _ = model_for(arch)
    n = 3
    x = O.make_images(n, seed=5)
    z = m.encode_images(x)
    for i, f in enumerate(orc.encoder_features(x)):
        assert rel(m.activation("enc_conv%d" % (i + 1), n), f) < TOL, "enc_conv%d" % (i + 1)
    zr = orc.encode_images(x)
    m.sample_at(zr)
    # the fused op that ends an MDBLOCK / a colour head is named after its last MDCL
    rename = {"dec_fc2": "l_dec_fc2", "out": "l_out", "dec_conv2a": "dec_conv2a2", "dec_conv3a": "dec_conv3a2",
              "dec_conv4a": "dec_conv4a2", "G": "G_b", "B": "B_b"}
    checked = 0
    for name, a in orc.decoder_activations(zr):
        nm = rename.get(name, name)
        if nm in m.lowered.slot_names:
            assert rel(m.activation(nm, n), a) < TOL, name
            checked += 1
    assert checked == (5 if arch == "IAN_simple" else 12)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6, 7])
def test_every_tile_config_and_split_policy(cfg):
    """All tapgemm tile shapes, with and without split-K, give the same answer."""
    m, orc, _ = model_for("IAN_simple")
    x = O.make_images(3, seed=7)
    ref = orc.reconstruct(x)
    try:
        from neural_photo_editor_amd.lib import is_ablation_build
        outs = []
        # K-loop schedules: 1 / 2 / 4 / 6 / 7 are the product's (autotune candidates); 0 (compiler-scheduled), 3 (LDS-DMA staging,
        # measured slower) and 8 exist in libian_ablation.so only (tests/test_gpu_ablation.py runs this test against it).
        # Same arithmetic in the same order -> identical bits.
        for var in ((0, 1, 2, 3, 4, 6, 7, 8) if is_ablation_build() else (1, 2, 4, 6, 7)):
            m.handle.set_option("tg_variant", var)
            m.handle.set_option("tg_cfg", cfg)
            m.handle.set_option("tg_split", 1)
            outs.append(m.reconstruct(x))
            assert rel(outs[-1], ref) < TOL
        assert all(np.array_equal(outs[0], o) for o in outs[1:])
        m.handle.set_option("tg_variant", 2)
        for split in (1, 0):
            m.handle.set_option("tg_cfg", cfg)
            m.handle.set_option("tg_split", split)
            assert rel(m.reconstruct(x), ref) < TOL
        m.handle.set_option("tg_target_items", 4096)   # aggressive split-K
        m.handle.set_option("tg_min_steps", 1)
        m.handle.set_option("tg_split", 1)
        base = m.reconstruct(x)
        assert rel(base, ref) < TOL
        # ... combined inside the launch (tg_fuse 1: write-through slabs + last arriver, reproducible; 2: float atomics) wherever
        # the tile carries that epilogue (the small 4-wave tiles; the others silently keep the reduce launch): launches of
        # images*QH*QW <= 1024 rows -- at 3 images every layer but enc_conv1
        for mode in (1, 2):
            m.handle.set_option("tg_fuse", mode)
            a, b = m.reconstruct(x), m.reconstruct(x)
            assert rel(a, ref) < TOL and rel(a, base) < 1e-5, mode
            if mode == 1:
                assert np.array_equal(a, b)
    finally:
        for k, v in (("tg_cfg", -1), ("tg_split", 1), ("tg_target_items", 768), ("tg_min_steps", 16), ("tg_variant", 2), ("tg_fuse", 0)):
            m.handle.set_option(k, v)


@pytest.mark.parametrize("arch", O.ARCHS)
def test_brush_gradients_vs_golden(arch):
    m, _, P = model_for(arch)
    g = np.load(os.path.join(GOLD, "%s_seed1.npz" % arch))
    z = g["z_sample"][:1]
    got = m.imgradRGB(26, 26, 30, 30, red_rgb(), z)
    assert got.shape == (1, 100) and rel(got, g["grad_rgb"]) < TOL_GRAD
    assert rel(m.imgrad(26, 26, 30, 30, z), g["grad_light"]) < TOL_GRAD
    # float-valued ints from Tk (NPE.py:202) are accepted
    assert np.array_equal(m.imgrad(26.0, 26.0, 30.0, 30.0, z), m.imgrad(26, 26, 30, 30, z))


@pytest.mark.parametrize("arch", O.ARCHS)
@pytest.mark.parametrize("patch", [(0, 0, 64, 64), (0, 0, 1, 1), (63, 63, 64, 64), (10, 20, 30, 40), (60, 0, 64, 9)])
def test_brush_gradients_patches_vs_twin(arch, patch):
    m, _, P = model_for(arch)
    import torch
    tw = TorchTwin(arch, P, dtype=torch.float64)
    z = O.make_latents(1, seed=11)
    rgb = np.random.RandomState(4).uniform(-1, 1, (1, 3, 64, 64)).astype(np.float32)
    c1, r1, c2, r2 = patch
    assert rel(m.imgradRGB(c1, r1, c2, r2, rgb, z), tw.imgradRGB(c1, r1, c2, r2, rgb, z)) < TOL_GRAD
    assert rel(m.imgrad(c1, r1, c2, r2, z), tw.imgrad(c1, r1, c2, r2, z)) < TOL_GRAD


@pytest.mark.parametrize("arch", O.ARCHS)
def test_edit_loop_trajectory(arch):
    """NPE.paint's update (NPE.py:199-209): Z -= 0.05 * grad * (1 + (x2 - x1)), 10 steps, vs the twin."""
    m, _, P = model_for(arch)
    tw = TorchTwin(arch, P)
    z_gpu = O.make_latents(1, seed=2).copy()
    z_ref = z_gpu.copy()
    c1, r1, c2, r2 = 26, 26, 30, 30
    rgb = red_rgb()
    for _ in range(10):
        z_gpu = z_gpu - 0.05 * m.imgradRGB(c1, r1, c2, r2, rgb, z_gpu) * (1 + (c2 - c1))
        z_ref = z_ref - 0.05 * tw.imgradRGB(c1, r1, c2, r2, rgb, z_ref) * (1 + (c2 - c1))
    assert rel(z_gpu, z_ref) < TOL
    assert rel(m.sample_at(z_gpu), tw.np_decode(z_ref)) < TOL


def test_decoder_forward_cache_is_transparent():
    """imgradRGB(z) right after sample_at(z) (NPE.py:205,218) reuses the resident decoder activations: same bits as a
    cold call, and a different latent / an intervening call invalidates the cache."""
    m, _, _ = model_for("IAN_simple")
    z1, z2 = O.make_latents(1, seed=31), O.make_latents(1, seed=32)
    rgb = red_rgb()
    os.environ["IAN_NO_DEC_CACHE"] = "1"
    try:
        cold1, cold2 = m.imgradRGB(26, 26, 30, 30, rgb, z1), m.imgradRGB(26, 26, 30, 30, rgb, z2)
    finally:
        del os.environ["IAN_NO_DEC_CACHE"]
    m.sample_at(z1)
    assert np.array_equal(m.imgradRGB(26, 26, 30, 30, rgb, z1), cold1)      # hit
    assert np.array_equal(m.imgradRGB(26, 26, 30, 30, rgb, z2), cold2)      # miss: other latent
    m.sample_at(z1)
    m.reconstruct(O.make_images(1, seed=3))                                  # clobbers the decoder activations
    assert np.array_equal(m.imgradRGB(26, 26, 30, 30, rgb, z1), cold1)
    rgb2 = rgb.copy()
    rgb2[0, :, 26:30, 26:30] = 0.25                                          # another colour: the upload cache must notice
    os.environ["IAN_NO_DEC_CACHE"] = "1"
    try:
        a = m.imgradRGB(26, 26, 30, 30, rgb2, z1)
    finally:
        del os.environ["IAN_NO_DEC_CACHE"]
    assert not np.array_equal(a, cold1)
    assert np.array_equal(m.imgradRGB(26, 26, 30, 30, rgb, z1), cold1) and np.array_equal(m.imgradRGB(26, 26, 30, 30, rgb2, z1), a)
    m.sample_at(np.concatenate([z1, z2]))                                    # batch 2: not cacheable
    assert np.array_equal(m.imgrad(26, 26, 30, 30, z1), m.imgrad(26, 26, 30, 30, z1.copy()))


@pytest.mark.parametrize("arch", O.ARCHS)
def test_fast_epilogue_equals_the_general_form(arch):
    """tg_fast_epilogue = 1 (the default: 32-bit buffer-descriptor stores, scale / shift once per column) against the general
    tg_store form, bit for bit.  3 images: ragged M on enc_conv3 / enc_conv4 (192 and 48 rows), full tiles elsewhere, the
    stride-2 deconv classes; full IAN supplies `res`, the brush gradient the BWD mode with `yfwd`.  IAN_simple's dense layers
    (scale_period != 0) take the general path under both settings."""
    m, _, _ = model_for(arch)
    x = O.make_images(3, seed=7)
    z = O.make_latents(1, seed=31)
    out = {}
    os.environ["IAN_NO_DEC_CACHE"] = "1"
    try:
        for fast in (0, 1):
            m.handle.set_option("tg_fast_epilogue", fast)
            out[fast] = (m.reconstruct(x), m.imgradRGB(10, 20, 30, 40, red_rgb(), z))
    finally:
        del os.environ["IAN_NO_DEC_CACHE"]
        m.handle.set_option("tg_fast_epilogue", 1)
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])


def test_device_pointers_equal_host_pointers():
    import torch
    m, _, _ = model_for("IAN_simple")
    x = O.make_images(4, seed=3)
    host = m.reconstruct(x)
    xd = torch.from_numpy(x).cuda()
    out = torch.empty_like(xd)
    m.handle.call("ian_reconstruct", xd, 4, out, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host)
    zd = torch.empty((4, 100), device="cuda")
    m.handle.call("ian_encode", xd, 4, zd)
    torch.cuda.synchronize()
    assert np.array_equal(zd.cpu().numpy(), m.encode_images(x))


# ---- full-size (BASELINE.json configs 2 and 3) size-independent properties --------------------------------
@pytest.mark.parametrize("arch,B", [("IAN_simple", 64), ("IAN", 256)])
def test_full_size_properties(arch, B):
    m, orc, _ = model_for(arch)
    x = O.make_images(B, seed=21)
    xh = m.reconstruct(x)
    assert xh.shape == (B, 3, 64, 64) and np.isfinite(xh).all() and np.abs(xh).max() <= 1.0
    # (a) images are independent: permuting the batch permutes the output, bit for bit
    perm = np.random.RandomState(0).permutation(B)
    assert np.array_equal(m.reconstruct(x[perm]), xh[perm])
    # (b) a SAMPLE of the batch against the oracle: three images (first, middle, last), because the CPU oracle needs seconds per
    # image.  The sample stands for the whole batch only together with (a): every image's result is bitwise independent of its
    # position and of its neighbours, so an image that is right in one slot is right in all of them; (c) covers all B images again.
    idx = [0, B // 2, B - 1]
    assert rel(xh[idx], orc.reconstruct(x[idx])) < TOL
    # (c) encode followed by decode equals reconstruct
    assert rel(m.sample_at(m.encode_images(x)), xh) < 1e-6


# ---- error behaviour ------------------------------------------------------------------------------------------
def test_errors_surface_as_exceptions():
    from neural_photo_editor_amd.lib import IanError
    m, _, _ = model_for("IAN_simple")
    with pytest.raises(ValueError):
        m.encode_images(np.zeros((0, 3, 64, 64), np.float32))
    with pytest.raises(ValueError):
        m.encode_images(np.zeros((2, 3, 32, 32), np.float32))
    with pytest.raises(ValueError):
        m.sample_at(np.zeros((2, 99), np.float32))
    with pytest.raises(IanError):
        m.imgrad(0, 0, 65, 64, np.zeros((1, 100), np.float32))
    # empty patch: mean over nothing; the reference would give NaN, we return a zero gradient without crashing
    g = m.imgrad(5, 5, 5, 5, np.zeros((1, 100), np.float32))
    assert np.all(g == 0)
    # n > 1 latents: API.py:59,64 differentiate a loss on X_hat[0] with respect to the WHOLE Z -> Z's shape, rows 1.. exactly zero
    # (INTEGRATION.md section 1 lists the three deviations above and this agreement)
    z3 = O.make_latents(3, seed=4)
    rgb = np.full((1, 3, 64, 64), -1.0, np.float32)
    for g3, g1 in ((m.imgrad(10, 12, 20, 30, z3), m.imgrad(10, 12, 20, 30, z3[:1])),
                   (m.imgradRGB(10, 12, 20, 30, rgb, z3), m.imgradRGB(10, 12, 20, 30, rgb, z3[:1]))):
        assert g3.shape == (3, 100) and g1.shape == (1, 100)
        assert np.array_equal(g3[:1], g1) and np.all(g3[1:] == 0)


@pytest.mark.parametrize("arch", O.ARCHS)
def test_every_decoder_gradient_buffer(arch):
    """dL/d(pre-epilogue value) of every decoder slot after imgradRGB vs autograd on the float64 twin is covered
    indirectly by dz; here: the brush gradient is linear in the seed -> full-image light gradient equals the sum
    of the gradients of a 2x2 partition of the image weighted by area (size-independent property)."""
    m, _, _ = model_for(arch)
    z = O.make_latents(1, seed=5)
    full = m.imgrad(0, 0, 64, 64, z)
    parts = [m.imgrad(c1, r1, c1 + 32, r1 + 32, z) for c1 in (0, 32) for r1 in (0, 32)]
    assert rel(sum(parts) / 4.0, full) < 1e-4


def test_sample_cli_writes_the_grid(tmp_path):
    """python sample_IAN.py <config> equivalent: 27 samples + 3 x [endpoint, 7 interpolants, endpoint] -> 6x9 grid."""
    from neural_photo_editor_amd import sample_cli
    cfg = str(tmp_path / "IAN.py")
    open(cfg, "w").write(open(os.path.join(CFG, "IAN.py")).read())
    with pytest.warns(UserWarning):
        out = sample_cli.main([cfg, "--out", str(tmp_path / "g.ppm")])
    data = open(out, "rb").read()
    assert data.startswith(b"P6\n576 384\n255\n") and len(data) == len(b"P6\n576 384\n255\n") + 384 * 576 * 3
    imgs = np.load(str(tmp_path / "g.npy"))
    assert imgs.shape == (54, 3, 64, 64) and imgs.dtype == np.uint8 and imgs.std() > 0


@pytest.mark.parametrize("n", [1, 2, 3])
def test_small_batch_image_layer_both_kernels(n):
    """IAN_simple's dec_out (IAN_simple.py:171-181) below batch 4: the 8-lanes-per-output-pixel kernel (default) and the
    tile kernel it replaced (dec_out_px=0) against the oracle and against each other."""
    m, orc, P = model_for("IAN_simple")
    z = O.make_latents(n, seed=40 + n)
    want = orc.sample_at(z)
    try:
        got_px = m.sample_at(z)
        m.handle.set_option("dec_out_px", 0)
        got_tile = m.sample_at(z)
    finally:
        m.handle.set_option("dec_out_px", 1)
    assert rel(got_px, want) < TOL and rel(got_tile, want) < TOL
    assert rel(got_px, got_tile) < 1e-5


@pytest.mark.parametrize("arch", O.ARCHS)
def test_latent_layer_backward_both_kernels(arch):
    """The last step of the brush gradient (backward-data of l_dec_fc2 into the latent): the batch-1 GEMV launch (default) and
    the split-K tap GEMM it replaced (dense_gemv=0) give the same gradient, and both match the golden one."""
    m, orc, P = model_for(arch)
    z = O.make_latents(1, seed=77)
    try:
        g1 = m.imgradRGB(8, 12, 40, 44, red_rgb(), z)
        l1 = m.imgrad(8, 12, 40, 44, z)
        m.handle.set_option("dense_gemv", 0)
        g0 = m.imgradRGB(8, 12, 40, 44, red_rgb(), z)
        l0 = m.imgrad(8, 12, 40, 44, z)
    finally:
        m.handle.set_option("dense_gemv", 1)
    assert rel(g1, g0) < 1e-5 and rel(l1, l0) < 1e-5
    assert np.abs(g1).max() > 0 and np.abs(l1).max() > 0
    # forward of the same layer: GEMV launch vs tap GEMM
    try:
        x1 = m.sample_at(z)
        m.handle.set_option("dense_gemv", 0)
        x0 = m.sample_at(z)
    finally:
        m.handle.set_option("dense_gemv", 1)
    assert rel(x1, x0) < 1e-5 and rel(x1, orc.sample_at(z)) < TOL


def _needs_ablation_library():
    """Negative results (in-launch split-K combine, kernels_b1.hip) are compiled into libian_ablation.so only; the product
    library rejects their options.  tests/test_gpu_ablation.py runs these tests against that library."""
    from neural_photo_editor_amd.lib import is_ablation_build
    if not is_ablation_build():
        m, _, _ = model_for("IAN_simple")
        for key, val in (("b1_conv", 1), ("tg_variant", 0), ("tg_variant", 3)):
            with pytest.raises(Exception):
                m.handle.set_option(key, val)                 # the product library refuses them loudly
        pytest.skip("variant compiled into libian_ablation.so only (see tests/test_gpu_ablation.py)")


@pytest.mark.parametrize("arch", O.ARCHS)
def test_split_k_combine_fused_vs_reduce_pass(arch):
    """Round 5: split-K partial sums combined INSIDE the tapgemm launch for the small launches of the batch-1 chains
    (kernels_tapgemm.hip, tg_fuse): mode 1 = write-through (sc1) slabs summed by the tile's last-arriving workgroup in slice order
    -- reproducible run to run whoever arrives last, which is also the sharp test of the hand-off itself (a stale slab line would
    change bits between repetitions); mode 2 = float atomics into a zero-at-rest tile + epilogue by the last arriver -- within
    round-off of the others, not bitwise.  Both match the oracle and the separate reduce pass (mode 0), forward and latent-brush
    backward, under aggressive split-K (tens of slabs per tile) and repeated 25 times back to back (uneven arrival orders)."""
    m, orc, P = model_for(arch)
    x = O.make_images(1, seed=91)
    z = O.make_latents(1, seed=92)
    want = orc.reconstruct(x)
    os.environ["IAN_NO_DEC_CACHE"] = "1"
    out = {}
    try:
        m.handle.set_option("tg_target_items", 4096)   # aggressive split-K: tens of slabs per tile
        m.handle.set_option("tg_min_steps", 1)
        for mode in (1, 2, 0):
            m.handle.set_option("tg_fuse", mode)
            out[mode] = ([m.reconstruct(x) for _ in range(25)], [m.imgradRGB(10, 20, 30, 40, red_rgb(), z) for _ in range(25)])
    finally:
        del os.environ["IAN_NO_DEC_CACHE"]
        for k, v in (("tg_target_items", 768), ("tg_min_steps", 16), ("tg_fuse", 0)):
            m.handle.set_option(k, v)
    for mode in (0, 1):
        assert all(np.array_equal(out[mode][0][0], a) for a in out[mode][0]), "mode %d: reconstruction not reproducible" % mode
        assert all(np.array_equal(out[mode][1][0], g) for g in out[mode][1]), "mode %d: gradient not reproducible" % mode
    for mode in (0, 1, 2):
        assert max(rel(a, want) for a in out[mode][0]) < TOL, mode
        assert max(rel(a, out[0][0][0]) for a in out[mode][0]) < 1e-5, mode
        assert max(rel(g, out[0][1][0]) for g in out[mode][1]) < 1e-4, mode
    with pytest.raises(Exception):
        m.handle.set_option("tg_fuse", 3)


@pytest.mark.parametrize("arch", O.ARCHS)
def test_batch1_streaming_deconv_equals_the_tapgemm_form(arch):
    """kernels_b1.hip (whole contraction per workgroup, one image) against the batch-N tapgemm + split-K form of the same
    transposed convs and of their backward-data: same arithmetic in another summation order -> float32 round-off apart,
    every decoder activation, every decoder gradient buffer and the latent gradient; both forms sit within 1e-4 of the
    oracle.  The streaming form is an experiment that stays selectable (b1_conv=1) but is OFF by default: it measured slower
    (DESIGN.md section 4)."""
    _needs_ablation_library()
    m, orc, _ = model_for(arch)
    z = O.make_latents(1, seed=41)
    rgb = red_rgb()
    outs = {}
    os.environ["IAN_NO_DEC_CACHE"] = "1"
    try:
        for flag in (1, 0):
            m.handle.set_option("b1_conv", flag)
            x = m.sample_at(z)
            acts = {nm: m.activation(nm, 1) for nm in m.lowered.slot_names if nm.startswith("dec_conv")}
            g = m.imgradRGB(10, 20, 30, 40, rgb, z)
            gl = m.imgrad(0, 0, 64, 64, z)
            outs[flag] = (x, acts, g, gl)
    finally:
        del os.environ["IAN_NO_DEC_CACHE"]
        m.handle.set_option("b1_conv", 0)
    (x1, a1, g1, l1), (x0, a0, g0, l0) = outs[1], outs[0]
    assert rel(x1, x0) < 2e-6 and rel(g1, g0) < 2e-5 and rel(l1, l0) < 2e-5
    assert a1.keys() == a0.keys() and len(a1) >= 3
    for nm in a1:
        assert rel(a1[nm], a0[nm]) < 2e-6, nm
    assert rel(x1, orc.sample_at(z)) < TOL

"""Position-major tile rows with the out-of-image taps of a tile skipped (option tg_pos_major; csrc/ian_tg_plan.h, tg_row in
kernels_tapgemm.hip) against image-major rows, on the GPU.  A skipped tap contributed exact zeros, so with K not split the two row
orders must agree BITWISE; with split-K only the slice boundaries move.

Shapes: single-position tiles must exist below the benchmark's batch of 64 -- 32 images under the 32x128, 64x64, 128x64 and 128x128
tiles give 1, 2, 4 and 4 positions per tile; 24 images give Bp = 32 with eight padding rows per position; 5 images Bp = 8; the brush
gradient Bp = 1.  Mode 2 forces position-major rows for any batch (auto, mode 1, starts at 64 images)."""
import os

import numpy as np
import pytest

from neural_photo_editor_amd import lib as L
from oracle import ian_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "neural_photo_editor_amd", "configs")
TOL = 1e-4          # the suite's bar against the oracle
TOL_SPLIT = 1e-5    # two split-K plans of one layer stack: a float32 sum of <= 25 600 terms re-associated at slice boundaries (measured
                    # <= 2.7e-6 by test_gpu_parity.py's split policies, <= 2.5e-6 over the cases of this file, each of which prints its figures)
TILES = {"32x128": 3, "64x64": 2, "128x64": 1, "128x128": 0}       # enum TgConfig
SHAPES = [(32, "32x128"), (32, "64x64"), (32, "128x64"), (32, "128x128"), (24, "64x64")]
DEFAULTS = (("tg_pos_major", 1), ("tg_cfg", -1), ("tg_split", 1), ("tg_target_items", 768), ("tg_min_steps", 16), ("tg_no_split_items", 384),
            ("tg_variant", 2))


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(np.asarray(b)).max() + 1e-30))


_models, _refs = {}, {}


def model_for(arch):
    if arch not in _models:
        from neural_photo_editor_amd import IAN
        P = O.make_params(arch, 1)
        _models[arch] = (IAN(os.path.join(CFG, arch + ".py"), True, params=P), O.Oracle(arch, P))
    return _models[arch]


def images(n):
    return O.make_images(n, seed=40 + n)


def oracle_recon(arch, n):
    """Computed once per (arch, batch), shared, never written to."""
    if (arch, n) not in _refs:
        _refs[arch, n] = model_for(arch)[1].reconstruct(images(n))
        _refs[arch, n].setflags(write=False)
    return _refs[arch, n]


def set_options(m, **kw):
    for k, v in kw.items():
        m.handle.set_option(k, v)


def restore(m):
    for k, v in DEFAULTS:
        m.handle.set_option(k, v)


def everything(m, n):
    """The reconstruction and every layer activation of its two halves, read the way test_gpu_parity.py::test_every_layer_activation
    reads them (m.activation after encode_images / sample_at)."""
    x = images(n)
    out = {"xhat": m.reconstruct(x)}
    z = m.encode_images(x)
    names = sorted(m.lowered.slot_names)
    for nm in names:
        if nm.startswith("enc_"):
            out[nm] = m.activation(nm, n)
    out["z"] = z
    m.sample_at(z)
    for nm in names:
        if not nm.startswith("enc_"):
            try:
                out[nm] = m.activation(nm, n)
            except L.IanError:        # a slot this batch never fills (fused head): absent in both row orders
                pass
    return out


@pytest.mark.parametrize("arch", O.ARCHS)
@pytest.mark.parametrize("n,tile", SHAPES)
def test_unsplit_position_major_is_bitwise_image_major(arch, n, tile):
    m, _ = model_for(arch)
    try:
        set_options(m, tg_cfg=TILES[tile], tg_split=0, tg_pos_major=0)
        a = everything(m, n)
        set_options(m, tg_pos_major=2)
        b = everything(m, n)
        assert sorted(a) == sorted(b) and len(a) >= 8, sorted(a)
        assert sum(k.startswith("enc_conv") for k in a) >= 4 and sum(k.startswith("dec_conv") for k in a) >= 3, sorted(a)
        for k in sorted(a):
            assert np.array_equal(a[k], b[k]), (k, rel(b[k], a[k]))
    finally:
        restore(m)


# limit None: the heuristic's split; 8 / 50: no item longer than that many K-steps (tg_min_steps is the floor of the heuristic's limit, and a
# target of 2^30 items puts the limit on the floor)
@pytest.mark.parametrize("arch", O.ARCHS)
@pytest.mark.parametrize("limit", [None, 8, 50])
@pytest.mark.parametrize("n,tile", SHAPES)
def test_split_position_major_agrees_with_image_major_and_the_oracle(arch, n, tile, limit):
    m, _ = model_for(arch)
    ref = oracle_recon(arch, n)
    x = images(n)
    try:
        set_options(m, tg_cfg=TILES[tile], tg_split=1)
        if limit is not None:
            set_options(m, tg_target_items=1 << 30, tg_no_split_items=1 << 30, tg_min_steps=limit)
        set_options(m, tg_pos_major=0)
        a = m.reconstruct(x)
        set_options(m, tg_pos_major=2)
        b = m.reconstruct(x)
        ea, eb, gap = rel(a, ref), rel(b, ref), rel(b, a)
        print("%s n=%d %s limit %s: image-major %.2e, position-major %.2e vs oracle; gap %.2e" % (arch, n, tile, limit, ea, eb, gap))
        assert ea < TOL and eb < TOL
        assert gap < TOL_SPLIT
    finally:
        restore(m)


def test_every_k_loop_schedule_gives_the_same_bits_position_major():
    m, _ = model_for("IAN_simple")
    x = images(32)
    try:
        set_options(m, tg_cfg=TILES["64x64"], tg_pos_major=2)
        outs = []
        for var in (1, 2, 4, 6, 7):
            set_options(m, tg_variant=var)
            outs.append(m.reconstruct(x))
        assert rel(outs[0], oracle_recon("IAN_simple", 32)) < TOL
        assert all(np.array_equal(outs[0], o) for o in outs[1:])
    finally:
        restore(m)


def test_brush_gradient_and_ragged_batch_position_major():
    """Bp = 1 (the batch-1 brush gradient: the backward epilogue and the reduce pass decode rows through the same function) and
    Bp = 8 (5 images: three padding rows per position)."""
    m, _ = model_for("IAN_simple")
    z = O.make_latents(1, seed=11)
    rgb = np.random.RandomState(4).uniform(-1, 1, (1, 3, 64, 64)).astype(np.float32)
    x5 = images(5)
    try:
        got = {}
        for split in (0, 1):
            for pm in (0, 2):
                set_options(m, tg_split=split, tg_pos_major=pm)
                got[split, pm] = (m.imgradRGB(10, 20, 30, 40, rgb, z), m.reconstruct(x5))
        assert np.array_equal(got[0, 0][0], got[0, 2][0]) and np.array_equal(got[0, 0][1], got[0, 2][1])
        gaps = rel(got[1, 2][0], got[1, 0][0]), rel(got[1, 2][1], got[1, 0][1])
        print("split-K gaps: brush gradient %.2e, 5-image reconstruction %.2e" % gaps)
        assert gaps[0] < TOL_SPLIT and gaps[1] < TOL_SPLIT
        assert rel(got[1, 2][1], oracle_recon("IAN_simple", 5)) < TOL
    finally:
        restore(m)


def test_tune_cache_format(tmp_path, monkeypatch):
    """A format-2 cache file (no row-order field) is ignored as a whole; a format-3 line whose row-order field is out of range is
    skipped on its own, and the tuner fills that layer in again."""
    from neural_photo_editor_amd import IAN
    cache = tmp_path / "tune.txt"
    monkeypatch.setenv("IAN_TUNE_CACHE", str(cache))
    m = IAN(os.path.join(CFG, "IAN_simple.py"), True, params=O.make_params("IAN_simple", 1))
    x = images(5)
    ref = m.reconstruct(x)
    old = "ian-tune-cache 2\n5 fwd enc_conv2 2 0 2 0\n5 fwd enc_conv3 2 0 2 0\n"
    cache.write_text(old)
    m.handle.autotune(5, 1)
    lines = cache.read_text().splitlines()
    assert lines[0] == "ian-tune-cache 3" and len(lines) > 5, lines[:3]
    assert all(len(ln.split()) == 8 and ln.split()[7] in ("-1", "0", "1") for ln in lines[1:]), lines
    assert rel(m.reconstruct(x), ref) < TOL_SPLIT
    # one line out of range in the new field, one poisoned so that taking it would show: 64x64 tile, no split, schedule 2
    victim = next(i for i, ln in enumerate(lines) if " enc_conv3 " in ln)
    keep = next(i for i, ln in enumerate(lines) if " enc_conv2 " in ln)
    lines[victim] = "5 fwd enc_conv3 2 0 2 0 7"
    lines[keep] = "5 fwd enc_conv2 2 0 2 0 0"
    cache.write_text("\n".join(lines) + "\n")
    m.handle.autotune(5, 1)
    after = cache.read_text().splitlines()
    assert after[0] == "ian-tune-cache 3" and len(after) == len(lines)
    assert lines[keep] in after                                   # a valid line is replayed, not re-tuned
    new = next(ln for ln in after if " enc_conv3 " in ln)
    assert new != lines[victim] and new.split()[7] in ("-1", "0", "1"), new
    assert rel(m.reconstruct(x), ref) < TOL_SPLIT
    m.close()

"""GPU unit parity of the small kernels that close the training step (csrc/kernels_train.hip from mb_weight_kernel down,
beta / beta_bwd and the layout helpers of kernels_misc.hip), called through the ian_k_* C entries, against float64 torch /
numpy on the CPU -- at the shapes the step really runs (nk = 500 over 16 grid-y blocks, nfeat = 1524, sharded MinibatchLayer
rows, 10^6-element Adam groups), at ragged edges, with strides larger than the row, and at values that saturate.

Tolerances are the project's (tests/README.md): 2e-5 on forward values, 1e-4 on gradients, 1e-6 absolute on Adam state of
O(1), bitwise where a kernel only moves or selects data.  Every buffer whose "not written" part belongs to the contract
(padding columns, outputs of rejected calls) is pre-filled with a sentinel and compared bit for bit.

The saturated cross-entropy case (test_saturated_cross_entropy) is the one the -log(softmax) form of the head cannot pass:
emulated in float32 on the CPU (denormals kept) that form is exact up to a logit gap of 90, 1.7e-4 / 2.7e-3 off at gaps
100 / 103 and +inf from 104 on (from ~87.4 on if expf flushes denormals); log(e0 + e1 + e2) - (z_t - m) is exact to float32
round-off at every gap.  The figures of this file on the MI355X (worst error per kernel family, first failing gap of the old
form, wall time) have NOT been recorded yet: each test prints its worst error (run with -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL, GTOL = 2e-5, 1e-4
SENT = -777.25                       # exactly representable; never a value any kernel here produces
WORST = {}


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / (np.abs(np.asarray(b)).max() + 1e-30))


def cs(c):
    return (c + 31) // 32 * 32


def c(v):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()


def sent(*shape):
    return torch.full(shape, SENT, device="cuda")


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def untouched(t):
    return bool((t == SENT).all())


def close(family, got, ref, tol, what=""):
    """max-norm relative error of got against ref under tol; the worst figure per kernel family is kept and printed"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    ref = ref.detach().numpy() if torch.is_tensor(ref) else ref
    e = rel(got, ref)
    WORST[family] = max(WORST.get(family, 0.0), e)
    assert np.isfinite(np.asarray(got)).all() and e < tol, (family, what, e, tol)
    return e


@pytest.fixture(scope="module")
def env():
    from neural_photo_editor_amd.lib import load_train_library
    from neural_photo_editor_amd import trainer as T
    lib = load_train_library()
    yield lib, T, T.K(lib)
    for fam in sorted(WORST):
        print("\n[train-tail] worst relative error %-22s %.3e" % (fam, WORST[fam]), end="")
    print()


def tt(v):
    return torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True)


# ----------------------------------------------------------------------------------------------------------------------
# MinibatchLayer
# ----------------------------------------------------------------------------------------------------------------------
def mb_reference(act, b, df):
    """float64 f = sum_b' exp(-(sum_d |act_b - act_b'| + 1e6 [b == b'])) + bias (layers.py:507-520) and d(sum f * df)/d act"""
    n = act.shape[0]
    at = tt(act)
    ad = (at.unsqueeze(3) - at.permute(1, 2, 0).unsqueeze(0)).abs().sum(2) + 1e6 * torch.eye(n, dtype=torch.float64).unsqueeze(1)
    f = torch.exp(-ad).sum(2) + torch.tensor(b, dtype=torch.float64).unsqueeze(0)
    (g,) = torch.autograd.grad(f, [at], torch.tensor(df, dtype=torch.float64))
    return f.detach().numpy(), g.numpy()


def mb_run(k, act, b, df, feat, shards):
    """mb_forward / mb_backward over `shards` equal row ranges of one activation matrix (nall = all rows), stacked"""
    nall, nk, nd = act.shape
    nin, n = feat.shape[1], nall // shards
    sa, sm, fs, dfs = cs(nk * nd) + 32, cs(nin + nk) + 32, nin + 5, nk + 3
    pad = lambda v, s: np.pad(v, ((0, 0), (0, s - v.shape[1])), constant_values=1e9)     # padding that would wreck a sum if read
    actd, featd, dfd, bd = c(pad(act.reshape(nall, -1), sa)), c(pad(feat, fs)), c(pad(df, dfs)), c(b)
    mbs, dacts = [], []
    for r in range(shards):
        mbd, dactd = sent(n, sm), sent(n, sa)
        k.mb_forward(actd, nall, sa, r * n, n, nk, nd, bd, featd[r * n:], fs, nin, mbd, sm)
        k.mb_backward(actd, nall, sa, r * n, n, nk, nd, dfd, dfs, dactd, sa)
        mbs.append(mbd.cpu().numpy())
        dacts.append(dactd.cpu().numpy())
    mb, dact = np.concatenate(mbs), np.concatenate(dacts)
    assert (mb[:, nin + nk:] == SENT).all() and (dact[:, nk * nd:] == SENT).all()          # row padding is not written
    assert same(mb[:, :nin], feat)                                                         # layers.py:524: the features, copied
    return mb[:, nin:nin + nk], dact[:, :nk * nd].reshape(nall, nk, nd)


MB_GEOMETRY = [(128, 1024, 500, 5), (5, 64, 33, 1), (7, 96, 64, 8), (3, 64, 31, 5)]


@pytest.mark.parametrize("n,nin,nk,nd", MB_GEOMETRY)
def test_minibatch_weight_normalisation(env, n, nin, nk, nd):
    """mb_weight / mb_weight_bwd (W = theta * exp(lws) / |theta|_col, layers.py:494): ncol = nk * nd is ragged against the
    32-column blocks in three of the four cases; accumulate 0 and 1."""
    lib, T, k = env
    rs = np.random.RandomState(nin + nk)
    ncol = nk * nd
    theta, lws = f32(rs.randn(nin, ncol) * 0.05), f32(rs.randn(ncol) * 0.1)
    dW = f32(rs.randn(nin, ncol))
    th, lw = tt(theta), tt(lws)
    sc = torch.exp(lw) / torch.sqrt((th ** 2).sum(0))
    W = th * sc.unsqueeze(0)
    gth, glw = torch.autograd.grad(W, [th, lw], torch.tensor(dW, dtype=torch.float64))
    Wd, csd = sent(nin * ncol + 8), sent(ncol + 8)
    k.mb_weight(c(theta), c(lws), Wd, csd, nin, ncol)
    close("mb_weight", Wd[:nin * ncol].reshape(nin, ncol), W, TOL)
    close("mb_weight", csd[:ncol], sc, TOL, "colscale")
    assert untouched(Wd[nin * ncol:]) and untouched(csd[ncol:])
    base_t, base_l = f32(rs.randn(nin, ncol)), f32(rs.randn(ncol))
    for accumulate in (0, 1):
        dth, dlw = c(np.append(base_t.ravel(), [SENT] * 8)), c(np.append(base_l, [SENT] * 8))
        k.mb_weight_bwd(c(theta), csd, c(dW), dth, dlw, nin, ncol, accumulate)
        add = float(accumulate)
        close("mb_weight_bwd", dth[:nin * ncol].reshape(nin, ncol).cpu().numpy() - add * base_t, gth, GTOL, accumulate)
        close("mb_weight_bwd", dlw[:ncol].cpu().numpy() - add * base_l, glw, GTOL, accumulate)
        assert untouched(dth[nin * ncol:]) and untouched(dlw[ncol:])


@pytest.mark.parametrize("n,nin,nk,nd", MB_GEOMETRY)
def test_minibatch_forward_backward_geometry(env, n, nin, nk, nd):
    """mb_forward / mb_backward on float32 activations that the float64 reference reads too (no GEMM in between): the step's
    geometry (nk = 500: 16 blocks in grid-y, the last with 20 live lanes; 128 samples: 16 strides of the 8 sample lanes) and
    ragged ones (n not a multiple of 8, nk < 32, nd = 1 and nd = 8)."""
    lib, T, k = env
    rs = np.random.RandomState(n + nk)
    act, b, df, feat = f32(rs.randn(n, nk, nd)), f32(rs.randn(nk)), f32(rs.randn(n, nk)), f32(rs.randn(n, nin))
    f, g = mb_reference(act, b, df)
    gf, gg = mb_run(k, act, b, df, feat, 1)
    close("mb_forward", gf, f, TOL)
    close("mb_backward", gg, g, GTOL)


def test_minibatch_sharded_rows_equal_the_whole_batch(env):
    """Data parallelism: each rank owns n rows [row0, row0 + n) of the nall = 3n gathered activations.  Three calls with
    row0 = 0, n, 2n, stacked, are the whole 3n-row batch: f needs every other row (o < nall) and must leave out exactly its
    own (o == row0 + b); dact needs the other ranks' df (df_all) in the (df[b] + df[b']) factor (mb_backward_kernel)."""
    lib, T, k = env
    rs = np.random.RandomState(17)
    n, nin, nk, nd = 6, 64, 33, 5
    act, b, df, feat = f32(rs.randn(3 * n, nk, nd)), f32(rs.randn(nk)), f32(rs.randn(3 * n, nk)), f32(rs.randn(3 * n, nin))
    f, g = mb_reference(act, b, df)
    gf, gg = mb_run(k, act, b, df, feat, 3)
    close("mb_forward", gf, f, TOL, "sharded")
    close("mb_backward", gg, g, GTOL, "sharded")


def test_minibatch_duplicate_rows(env):
    """Two samples with identical activations: distance 0, exp(0) = 1 in f, and sign(0) = 0 in the backward (torch's abs
    backward gives 0 there as well)."""
    lib, T, k = env
    rs = np.random.RandomState(18)
    n, nin, nk, nd = 9, 64, 40, 5
    act, b, df, feat = f32(rs.randn(n, nk, nd)), f32(rs.randn(nk)), f32(rs.randn(n, nk)), f32(rs.randn(n, nin))
    act[7] = act[2]
    f, g = mb_reference(act, b, df)
    assert (f[2] - b > 1.0).all()                                       # the duplicate contributes exp(0)
    gf, gg = mb_run(k, act, b, df, feat, 1)
    close("mb_forward", gf, f, TOL, "duplicates")
    close("mb_backward", gg, g, GTOL, "duplicates")


def test_minibatch_rejects_more_than_eight_dimensions(env):
    lib, T, k = env
    n, nin, nk, nd = 4, 32, 8, 9
    act, mb, dact = torch.zeros(n, cs(nk * nd), device="cuda"), sent(n, cs(nin + nk)), sent(n, cs(nk * nd))
    feat, b, df = torch.zeros(n, nin, device="cuda"), torch.zeros(nk, device="cuda"), torch.zeros(n, nk, device="cuda")
    with pytest.raises(T.IanTrainError):
        k.mb_forward(act, n, cs(nk * nd), 0, n, nk, nd, b, feat, nin, nin, mb, cs(nin + nk))
    with pytest.raises(T.IanTrainError):
        k.mb_backward(act, n, cs(nk * nd), 0, n, nk, nd, df, nk, dact, cs(nk * nd))
    torch.cuda.synchronize()
    assert untouched(mb) and untouched(dact)


# ----------------------------------------------------------------------------------------------------------------------
# discriminator head
# ----------------------------------------------------------------------------------------------------------------------
def head_reference(z, t0, t1, acc):
    """float64: p, the four loss slots (categorical cross-entropy as logsumexp(z) - z_t; 0 for target -1; first-maximum flag; 0)"""
    zt = torch.tensor(z, dtype=torch.float64)
    p = torch.softmax(zt, 1).numpy()
    lse = torch.logsumexp(zt, 1).numpy()
    loss = np.zeros((z.shape[0], 4))
    for s, t in enumerate((t0, t1)):
        if t >= 0:
            loss[:, s] = lse - z[:, t]
    loss[:, 2] = (np.argmax(z, 1) == acc)
    return p, loss


FWD_TARGETS = [(0, -1, 0), (0, 1, 1), (0, 2, 2), (-1, -1, 0)]           # enc_forward calls of ian_trainer.cpp + "no term at all"
BWD_TARGETS = [(0, -1), (1, -1), (2, -1), (0, 1), (-1, -1)]            # enc_backward calls + two terms + none


@pytest.mark.parametrize("nfeat", [84, 1524, 257])
@pytest.mark.parametrize("n", [1, 6, 128])
def test_discriminator_head(env, nfeat, n):
    """disc_head / disc_head_bwd / disc_head_wgrad: 1524 features = 6 strides of the 256 threads with a ragged tail, 257 = one
    thread with two features; all four loss slots and p; accumulate 0 and 1."""
    lib, T, k = env
    rs = np.random.RandomState(nfeat + n)
    ms = cs(nfeat) + 32
    mb, Wd = f32(rs.randn(n, nfeat)), f32(rs.randn(nfeat, 3) * 2.0 / np.sqrt(nfeat))
    z = mb.astype(np.float64) @ Wd.astype(np.float64)
    mbd, Wdd = c(np.pad(mb, ((0, 0), (0, ms - nfeat)), constant_values=1e9)), c(Wd)
    for t0, t1, acc in FWD_TARGETS:
        p, loss = head_reference(z, t0, t1, acc)
        pd, ld = sent(n, 3), sent(n, 4)
        k.disc_head(mbd, ms, nfeat, Wdd, n, t0, t1, acc, pd, ld)
        got = ld.cpu().numpy()
        close("disc_head", pd, p, TOL, "p")
        for s, t in enumerate((t0, t1)):
            if t >= 0:
                close("disc_head", got[:, s], loss[:, s], TOL, ("loss", s, t))
            else:
                assert same(got[:, s], np.zeros(n))
        assert same(got[:, 2], loss[:, 2]) and same(got[:, 2], np.argmax(pd.cpu().numpy(), 1) == acc)
        assert same(got[:, 3], np.zeros(n))
    p = torch.softmax(torch.tensor(z), 1).numpy()
    base = f32(rs.randn(nfeat, 3))
    for t0, t1 in BWD_TARGETS:
        w0, w1 = 0.7 / n, 0.2 / n
        dl = sum(w * (p - np.eye(3)[t]) for t, w in ((t0, w0), (t1, w1)) if t >= 0) + np.zeros_like(p)
        dlog, dmb = sent(n, 4), sent(n, ms)
        k.disc_head_bwd(pd, Wdd, nfeat, n, t0, w0, t1, w1, dlog, dmb, ms)
        assert untouched(dlog[:, 3]) and untouched(dmb[:, nfeat:])
        if t0 < 0 and t1 < 0:
            assert same(dlog[:, :3], np.zeros((n, 3))) and same(dmb[:, :nfeat], np.zeros((n, nfeat)))
            continue
        close("disc_head_bwd", dlog[:, :3], dl, GTOL, (t0, t1))
        close("disc_head_bwd", dmb[:, :nfeat], dl @ Wd.astype(np.float64).T, GTOL, (t0, t1))
        for accumulate in (0, 1):
            dWd = c(np.append(base.ravel(), [SENT] * 5))
            k.disc_head_wgrad(mbd, ms, nfeat, n, dlog, dWd, accumulate)
            ref = mb.astype(np.float64).T @ dlog[:, :3].cpu().numpy().astype(np.float64)
            close("disc_head_wgrad", dWd[:nfeat * 3].reshape(nfeat, 3).cpu().numpy() - accumulate * base, ref, GTOL, accumulate)
            assert untouched(dWd[nfeat * 3:])


@pytest.mark.parametrize("equal", [(0, 1), (1, 2), (0, 2), (0, 1, 2)])
def test_discriminator_accuracy_flag_on_ties(env, equal):
    """Equal columns of Wd give bit-equal logits: the accuracy flag follows the FIRST maximum, as T.argmax / numpy.argmax do."""
    lib, T, k = env
    rs = np.random.RandomState(5)
    n, nfeat = 64, 257
    mb, Wd = f32(rs.randn(n, nfeat)), f32(rs.randn(nfeat, 3) * 0.1)
    for j in equal[1:]:
        Wd[:, j] = Wd[:, equal[0]]
    z = np.stack([mb.astype(np.float64) @ np.ascontiguousarray(Wd[:, j], np.float64) for j in range(3)], 1)   # same routine per column
    assert all((z[:, j] == z[:, equal[0]]).all() for j in equal)
    assert (z.argmax(1) == equal[0]).sum() > 0                              # the tied classes do win somewhere
    for acc in (0, 1, 2):
        pd, ld = sent(n, 3), sent(n, 4)
        k.disc_head(c(mb), nfeat, nfeat, c(Wd), n, 0, -1, acc, pd, ld)
        assert same(ld[:, 2], np.argmax(z, 1) == acc), (equal, acc)


GAPS = [0, 1, 20, 60, 86, 89, 95, 100, 103, 104, 110, 200]


def test_saturated_cross_entropy(env):
    """Logit gaps to the target class from 0 to 200, exact in float32 (one feature column per class, identity rows of Wd):
    every loss finite, 2e-5 over the vector and per sample |got - ref| <= 2e-5 max(ref, 1) against float64
    logsumexp(z) - z_t, so that the large entries cannot mask the small ones; the gradient seeds against softmax - onehot."""
    lib, T, k = env
    n, nfeat = len(GAPS), 84
    z = np.array([[0.0, g, -3.0] for g in GAPS])
    mb, Wd = np.zeros((n, nfeat), np.float32), np.zeros((nfeat, 3), np.float32)
    mb[:, :3], Wd[:3] = z, np.eye(3)
    p, loss = head_reference(z, 0, 1, 1)                                     # slot 0: the losing class; slot 1: the winning one
    pd, ld = sent(n, 3), sent(n, 4)
    k.disc_head(c(mb), nfeat, nfeat, c(Wd), n, 0, 1, 1, pd, ld)
    got = ld.cpu().numpy().astype(np.float64)
    table = [(g, float(got[i, 0]), float(loss[i, 0])) for i, g in enumerate(GAPS)]
    print("\n[train-tail] saturated cross-entropy (gap, kernel, float64):", table)
    assert np.isfinite(got).all(), table
    for s in (0, 1):
        close("disc_head_saturated", got[:, s], loss[:, s], TOL, table)
        err = np.abs(got[:, s] - loss[:, s])
        assert (err <= TOL * np.maximum(loss[:, s], 1.0)).all(), (s, table)
    close("disc_head_saturated", pd, p, TOL, "p")
    dlog, dmb = sent(n, 4), sent(n, nfeat)
    k.disc_head_bwd(pd, c(Wd), nfeat, n, 0, 1.0, -1, 0.0, dlog, dmb, nfeat)
    close("disc_head_bwd", dlog[:, :3], p - np.eye(3)[0], GTOL, "saturated")


# ----------------------------------------------------------------------------------------------------------------------
# latent kernels
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["randn", "wide"])
@pytest.mark.parametrize("stride", [128, 160])
@pytest.mark.parametrize("n", [1, 5, 128])
@pytest.mark.parametrize("d", [1, 37, 100, 128])
def test_gaussian_sample_and_kl(env, d, n, stride, regime):
    """sample / sample_bwd (layers.py:419-433, train_IAN.py:172).  'wide': ls in [-8, 4], mu in [-6, 6] -- the KL term and dls are
    dominated by exp(2 ls) there (finite in float32).  eps has a row stride of its own; padding columns are not written."""
    lib, T, k = env
    rs = np.random.RandomState(d * 7 + n + stride)
    es = d + 3
    if regime == "randn":
        mu, ls = f32(rs.randn(n, d)), f32(rs.randn(n, d) * 0.3)
    else:
        mu, ls = f32(rs.uniform(-6, 6, (n, d))), f32(rs.uniform(-8, 4, (n, d)))
        ls.flat[0], ls.flat[-1] = 4.0, -8.0
    eps, dz0 = f32(rs.randn(n, d)), f32(rs.randn(n, d))
    klw = 1.0 / (n * d)
    mut, lst = tt(mu), tt(ls)
    z0 = mut + torch.exp(lst) * torch.tensor(eps, dtype=torch.float64)
    klt = 1 + 2 * lst - mut ** 2 - torch.exp(2 * lst)
    gmu, gls = torch.autograd.grad((z0 * torch.tensor(dz0, dtype=torch.float64)).sum() - 0.5 * klt.mean(), [mut, lst])
    pad = lambda v, s: c(np.pad(v, ((0, 0), (0, s - d)), constant_values=1e9))
    mud, lsd, epsd, dz0d = pad(mu, stride), pad(ls, stride), pad(eps, es), pad(dz0, stride)
    z0d, kld = sent(n, stride), sent(n * d + 4)
    k.sample(mud, lsd, epsd, z0d, kld, n, d, stride, es)
    close("sample", z0d[:, :d], z0, TOL, regime)
    close("sample", kld[:n * d].reshape(n, d), klt, TOL, regime + " kl term")
    assert untouched(z0d[:, d:]) and untouched(kld[n * d:])
    dmud, dlsd = sent(n, stride), sent(n, stride)
    k.sample_bwd(mud, lsd, epsd, dz0d, dmud, dlsd, n, d, stride, es, klw)
    close("sample_bwd", dmud[:, :d], gmu, GTOL, regime)
    close("sample_bwd", dlsd[:, :d], gls, GTOL, regime)
    assert untouched(dmud[:, d:]) and untouched(dlsd[:, d:])


def made_case(d, n, seed):
    """MADE weights + inputs whose 4 * n * d ReLU pre-activations (float64) all stay 1e-6 away from the kink, so that a float32
    evaluation takes the same branches (every hidden unit of these masks has ONE live input -- made.masks_once -- so its float32
    pre-activation is one fma of an input that is itself one fma: error < 1e-7); the seed is advanced until that holds."""
    from neural_photo_editor_amd import made
    masks = made.masks_once(d)
    for s in range(seed, seed + 50):
        rs = np.random.RandomState(s)
        Ws = [f32(rs.randn(d, d) * 0.1) * m for _ in range(2) for m in masks]
        bs = [f32(rs.randn(d) * 0.1) for _ in range(6)]
        z0, dz = f32(rs.randn(n, d)), f32(rs.randn(n, d))
        W, Bv = [torch.tensor(w, dtype=torch.float64) for w in Ws], [torch.tensor(b, dtype=torch.float64) for b in bs]
        zt = tt(z0)
        margin = []

        def pre(x, o):
            v = x @ W[o] + Bv[o]
            margin.append(float(v.detach().abs().min()))
            return torch.relu(v)
        # the reference graph runs each masked MLP on its own first hidden layer (made_iaf_kernel; layers.py:775)
        mlp = lambda h1, o: (pre(h1, o) @ W[o + 1] + Bv[o + 1]) + (h1 @ W[o + 2] + Bv[o + 2])
        z = (zt - mlp(pre(zt, 0), 0)) / torch.exp(mlp(pre(zt, 3), 3))
        if min(margin) > 1e-6:
            (g,) = torch.autograd.grad(z, [zt], torch.tensor(dz, dtype=torch.float64))
            return np.stack(Ws), np.stack(bs), z0, dz, z.detach().numpy(), g.numpy()
    raise AssertionError("no seed keeps the pre-activations off the ReLU kink")


@pytest.mark.parametrize("stride", [128, 160])
@pytest.mark.parametrize("n", [1, 5, 128])
@pytest.mark.parametrize("d", [1, 37, 100, 128])
def test_made_iaf_forward_backward(env, d, n, stride):
    """made_iaf / made_iaf_bwd for every d the launchers accept at its edges (1, 128 = all lanes live) and ragged in between."""
    lib, T, k = env
    Ws, bs, z0, dz, z, g = made_case(d, n, 1000 + d + n)
    pad = lambda v: c(np.pad(v, ((0, 0), (0, stride - d)), constant_values=1e9))
    wts, bias, z0d, dzd = c(Ws), c(bs), pad(z0), pad(dz)
    zd, dz0d = sent(n, stride), sent(n, stride)
    k.made_iaf(z0d, zd, wts, bias, n, d, stride)
    close("made_iaf", zd[:, :d], z, TOL)
    k.made_iaf_bwd(z0d, dzd, dz0d, wts, bias, n, d, stride)
    close("made_iaf_bwd", dz0d[:, :d], g, GTOL)
    assert untouched(zd[:, d:]) and untouched(dz0d[:, d:])


def test_made_iaf_rejects_more_than_128_latents(env):
    lib, T, k = env
    n, d = 2, 129
    z0, wts, bias = torch.zeros(n, 160, device="cuda"), torch.zeros(6 * d * d, device="cuda"), torch.zeros(6 * d, device="cuda")
    z, dz0 = sent(n, 160), sent(n, 160)
    with pytest.raises(T.IanTrainError):
        k.made_iaf(z0, z, wts, bias, n, d, 160)
    with pytest.raises(T.IanTrainError):
        k.made_iaf_bwd(z0, z0, dz0, wts, bias, n, d, 160)
    torch.cuda.synchronize()
    assert untouched(z) and untouched(dz0)


# ----------------------------------------------------------------------------------------------------------------------
# pair loss / row sums
# ----------------------------------------------------------------------------------------------------------------------
def pair_reference(a, b, mode, w):
    at, bt = tt(a), torch.tensor(b, dtype=torch.float64)
    v1 = (2 * (at - bt + 1e-8).abs()).sum() if mode == 0 else ((at - bt) ** 2).sum()    # train_IAN.py:169 / :244
    (ga,) = torch.autograd.grad(w * v1, [at])
    return float(v1), float(((at - bt) ** 2).sum()) if mode == 0 else 0.0, ga.numpy()


def pair_check(k, a, b, stride, mode, what):
    rows, C = a.shape
    rs = np.random.RandomState(rows + C)
    w, scale = 3.0 / a.size, 1.0 / a.size
    v1, v2, ga = pair_reference(a, b, mode, w)
    pad = lambda v: c(np.pad(v, ((0, 0), (0, stride - C)), constant_values=1e9))
    ad, bd = pad(a), pad(b)
    base = f32(rs.randn(rows, C) * w)                 # on the gradient's own scale: (base + g) - base keeps g's digits
    for nblocks in (1, 64, 1024):
        for accumulate in (0, 1):
            ws, out, da = sent(2 * nblocks + 2), sent(4), pad(base)
            da[:, C:] = SENT
            k.pair_loss(ad, bd, da, rows, C, stride, mode, w, accumulate, ws, nblocks, scale, out)
            o = out.cpu().numpy()
            close("pair_loss", o[:1], [scale * v1], TOL, (what, nblocks))
            if mode == 0:
                close("pair_loss", o[1:2], [scale * v2], TOL, (what, nblocks, "sum of squares"))
            else:
                assert o[1] == 0.0
            close("pair_loss", da[:, :C].cpu().numpy() - accumulate * base, ga, TOL, (what, nblocks, accumulate))
            assert untouched(da[:, C:]) and untouched(out[2:]) and untouched(ws[2 * nblocks:])
        ws, out = sent(2 * nblocks + 2), sent(4)
        k.pair_loss(ad, bd, None, rows, C, stride, mode, 0.0, 0, ws, nblocks, scale, out)   # da = NULL: the metrics pass
        close("pair_loss", out[:1], [scale * v1], TOL, (what, nblocks, "no gradient"))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("rows,C,stride", [(7, 33, 33), (1, 1, 1), (4096, 3, 3), (300, 100, 128), (257, 255, 256)])
def test_pair_loss_shapes(env, rows, C, stride, mode):
    """pair_loss + sum_finalize: one block (every thread strides the whole tensor), 64 and 1024 blocks (most of them empty on
    the small shapes), rows whose stride exceeds C (padding holds 1e9: a read of it wrecks the sum), accumulate, da = NULL."""
    lib, T, k = env
    rs = np.random.RandomState(rows * 3 + C + mode)
    a, b = f32(rs.uniform(-1, 1, (rows, C))), f32(rs.uniform(-1, 1, (rows, C)))
    pair_check(k, a, b, stride, mode, (rows, C, stride, mode))


def test_pixel_loss_sign_where_the_images_are_equal(env):
    """a == b exactly on a third of the elements: the reference's |a - b + 1e-8| (train_IAN.py:169) has derivative +1 there, in
    float32 and in float64 alike -- sign(a - b) would give 0."""
    lib, T, k = env
    rs = np.random.RandomState(9)
    a, b = f32(rs.uniform(-1, 1, (300, 100))), f32(rs.uniform(-1, 1, (300, 100)))
    b.flat[::3] = a.flat[::3]
    _, _, ga = pair_reference(a, b, 0, 3.0 / a.size)
    assert (ga.flat[::3] > 0).all()
    pair_check(k, a, b, 128, 0, "ties")


@pytest.mark.parametrize("width", [1, 2, 4, 63, 64])
def test_sum_rows(env, width):
    """sum_rows (sum_finalize_kernel on a caller's [n][width] array): width 4 over 128 samples is the per-sample loss slots;
    n around the 16-row stride of its four interleaved accumulators."""
    lib, T, k = env
    rs = np.random.RandomState(width)
    for n in (1, 3, 15, 16, 17, 128, 1000):
        x = f32(rs.uniform(-0.5, 1.5, (n, width)))
        out = sent(66)
        k.sum_rows(c(x), n, width, 0.37 / n, out)
        close("sum_rows", out[:width], x.astype(np.float64).sum(0) * (0.37 / n), TOL, (n, width))
        assert untouched(out[width:])


def test_sum_rows_rejects_more_than_64_columns(env):
    lib, T, k = env
    out = sent(80)
    with pytest.raises(T.IanTrainError):
        k.sum_rows(torch.ones(4 * 65, device="cuda"), 4, 65, 1.0, out)
    torch.cuda.synchronize()
    assert untouched(out)


# ----------------------------------------------------------------------------------------------------------------------
# Adam
# ----------------------------------------------------------------------------------------------------------------------
class AdamRef:
    """lasagne.updates.adam (App. B.7) in float64 on the float32 inputs"""

    def __init__(self, p):
        self.p, self.m, self.v, self.t = p.astype(np.float64), np.zeros(p.size), np.zeros(p.size), 0

    def step(self, g, lr=2e-4, b1=0.5, b2=0.999, eps=1e-8):
        self.t += 1
        a_t = lr * np.sqrt(1 - b2 ** self.t) / (1 - b1 ** self.t)
        self.m = b1 * self.m + (1 - b1) * g
        self.v = b2 * self.v + (1 - b2) * g.astype(np.float64) ** 2
        self.p = self.p - a_t * self.m / (np.sqrt(self.v) + eps)
        return float(a_t)


@pytest.mark.parametrize("n", [1, 255, 257, 5 * 10 ** 6])
def test_adam(env, n):
    """adam_kernel: three steps from a zero state, then a zero gradient (pure decay of m and v); a zero gradient on a zero state
    (0 / (0 + eps): the update is exactly 0); |g| = 1e-25 (g^2 underflows: v stays 0).  5e6 elements is past the grid cap
    (8192 blocks of 256): the grid-stride loop runs three times.  p, m and v against float64, 1e-6 absolute on values of O(1)."""
    lib, T, k = env
    rs = np.random.RandomState(n % 1000)
    p0 = f32(rs.randn(n))
    ref = AdamRef(p0)
    pd, md, vd = c(np.append(p0, SENT)), c(np.append(np.zeros(n), SENT)), c(np.append(np.zeros(n), SENT))

    def check(what):
        for name, got, want in (("p", pd, ref.p), ("m", md, ref.m), ("v", vd, ref.v)):
            e = float(np.abs(got[:n].cpu().numpy().astype(np.float64) - want).max())
            WORST["adam (absolute)"] = max(WORST.get("adam (absolute)", 0.0), e)
            assert e < 1e-6, (what, name, e)
            if name != "p":                                                # m, v are not O(1): held relatively as well
                close("adam m, v", got[:n], want, TOL, (what, name))
        assert untouched(pd[n:]) and untouched(md[n:]) and untouched(vd[n:])
    for t in range(3):
        g = f32(rs.randn(n))
        k.adam(pd, c(g), md, vd, n, ref.step(g), 0.5, 0.999, 1e-8)
        check("step %d" % (t + 1))
    g = np.zeros(n, np.float32)
    k.adam(pd, c(g), md, vd, n, ref.step(g), 0.5, 0.999, 1e-8)
    check("zero gradient after three steps")
    # zero gradient on a zero state
    ref = AdamRef(p0)
    pd, md, vd = c(np.append(p0, SENT)), c(np.append(np.zeros(n), SENT)), c(np.append(np.zeros(n), SENT))
    k.adam(pd, c(g), md, vd, n, ref.step(g), 0.5, 0.999, 1e-8)
    assert same(pd[:n], p0) and same(md[:n], np.zeros(n)) and same(vd[:n], np.zeros(n))
    # gradients whose square underflows
    g = f32(1e-25 * np.sign(rs.randn(n) + 1e-3))
    k.adam(pd, c(g), md, vd, n, ref.step(g), 0.5, 0.999, 1e-8)
    check("|g| = 1e-25")
    assert same(vd[:n], np.zeros(n))
    assert rel(md[:n].cpu().numpy(), ref.m) < 1e-6


# ----------------------------------------------------------------------------------------------------------------------
# entries no unit test reached: beta / beta_bwd, concat2, gather, layout transposes, globalpool, bn_running
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 5])
@pytest.mark.parametrize("rs_", [2, 32])
@pytest.mark.parametrize("hw", [64 * 64, 7])
@pytest.mark.parametrize("n", [1, 3])
def test_beta_layer(env, n, hw, rs_, act):
    """beta / beta_bwd (layers.py:397-408 x 3 + concat): out_c = 2 a / (a + b + 1e-8) - 1 on the two channels of three NHWC maps
    of pixel stride rs -> NCHW [n, 3, hw].  ian_k_beta_bwd takes ONE act for the three maps (the step passes sigmoid = 5; 0 = the
    bare layer) and plain gradient outputs.  Pixel 0 of every map is a = b = 0 (output exactly -1, finite gradient), pixel 1 is
    a = 0 < b; they are compared apart from the rest so that their 2e8 does not set the norm."""
    lib, T, k = env
    rs = np.random.RandomState(n * 100 + hw % 97 + rs_ + act)
    npix = n * hw
    maps = [f32(np.abs(rs.randn(npix, 2)) + 1e-3) if act == 0 else f32(1 / (1 + np.exp(-2 * rs.randn(npix, 2)))) for _ in range(3)]
    for m in maps:
        m[0], m[1, 0] = 0.0, 0.0
    gout = f32(rs.randn(n, 3, hw))
    vt = [tt(m) for m in maps]
    y = torch.stack([2 * (v[:, 0] / (v[:, 0] + v[:, 1] + 1e-8)) - 1 for v in vt], 0).reshape(3, n, hw).permute(1, 0, 2)
    gv = torch.autograd.grad(y, vt, torch.tensor(gout, dtype=torch.float64))
    dact = (lambda m: 1.0) if act == 0 else (lambda m: m.astype(np.float64) * (1 - m.astype(np.float64)))
    gref = [g.numpy() * dact(m) for g, m in zip(gv, maps)]
    pad = lambda m: c(np.pad(m, ((0, 0), (0, rs_ - 2)), constant_values=1e9))
    md = [pad(m) for m in maps]
    yd = sent(n * 3 * hw + 4)
    k.beta(md[0], md[1], md[2], yd, n, hw, rs_)
    got = yd[:n * 3 * hw].reshape(n, 3, hw)
    close("beta", got, y, TOL)
    assert same(got[0, :, :2], -np.ones((3, 2))) and untouched(yd[n * 3 * hw:])
    gd = [sent(npix, rs_) for _ in range(3)]
    k.beta_bwd(c(gout), md[0], md[1], md[2], gd[0], gd[1], gd[2], n, hw, rs_, act)
    for g, ref in zip(gd, gref):
        g = g.cpu().numpy()
        assert np.isfinite(g[:, :2]).all() and (g[:, 2:] == SENT).all()
        close("beta_bwd", g[2:, :2], ref[2:], GTOL, "regular pixels")
        close("beta_bwd", g[:1, :2], ref[:1], GTOL, "a = b = 0")
        close("beta_bwd", g[1:2, :2], ref[1:2], GTOL, "a = 0 < b")


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("ca,cb", [(3, 33), (33, 160), (160, 3), (2, 2)])
def test_concat2_is_a_copy(env, ca, cb, n):
    lib, T, k = env
    rs = np.random.RandomState(ca + cb + n)
    npix, sa, sb, sy = n * 37, cs(ca) + 32, cs(cb), cs(ca + cb) + 32
    a, b = f32(rs.randn(npix, sa)), f32(rs.randn(npix, sb))
    y = sent(npix, sy)
    k.concat2(c(a), ca, sa, c(b), cb, sb, y, sy, npix)
    assert same(y[:, :ca + cb], np.concatenate([a[:, :ca], b[:, :cb]], 1)) and untouched(y[:, ca + cb:])


@pytest.mark.parametrize("count", [1, 1000, 3 * 10 ** 6])
def test_gather_is_a_copy_with_holes(env, count):
    """dst[i] = map[i] >= 0 ? src[map[i]] : 0 -- 3e6 entries is past the grid cap (grid-stride loop)."""
    lib, T, k = env
    rs = np.random.RandomState(count % 999)
    src = f32(rs.randn(4097))
    m = rs.randint(-1, src.size, count).astype(np.int32)
    m[0] = -1
    dst = sent(count + 3)
    k.gather(c(src), torch.from_numpy(m).cuda(), dst, count)
    assert same(dst[:count], np.where(m >= 0, src[np.maximum(m, 0)], np.float32(0))) and untouched(dst[count:])


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("ch,stride", [(3, 3), (3, 32), (33, 64), (160, 160), (160, 192)])
def test_layout_transposes_are_copies(env, ch, stride, n):
    lib, T, k = env
    rs = np.random.RandomState(ch + stride + n)
    hw = 7 * 9
    x = f32(rs.randn(n, ch, hw))
    nhwc = sent(n, hw, stride)
    k.nchw_to_nhwc(c(x), nhwc, n, hw, ch, stride)
    assert same(nhwc[..., :ch], x.transpose(0, 2, 1)) and untouched(nhwc[..., ch:])
    back = sent(n * ch * hw + 2)
    k.nhwc_to_nchw(nhwc, stride, back, n, hw, ch)
    assert same(back[:n * ch * hw], x.ravel()) and untouched(back[n * ch * hw:])


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("C,xs,ys", [(3, 32, 3), (33, 64, 40), (160, 160, 192), (1024, 1024, 1024)])
def test_globalpool(env, C, xs, ys, n):
    """GlobalPoolLayer: forward against the float64 mean; the backward only scales (dy / hw, one IEEE division) and spreads:
    bit for bit, overwrite and accumulate."""
    lib, T, k = env
    rs = np.random.RandomState(C + n)
    hw = 16
    x, dy, base = f32(rs.randn(n, hw, C)), f32(rs.randn(n, C)), f32(rs.randn(n, hw, C))
    pad = lambda v, s: c(np.pad(v, [(0, 0)] * (v.ndim - 1) + [(0, s - C)], constant_values=1e9))
    y = sent(n, ys)
    k.globalpool(pad(x, xs), y, n, hw, C, xs, ys)
    close("globalpool", y[:, :C], x.astype(np.float64).mean(1), TOL)
    assert untouched(y[:, C:])
    g = (dy / np.float32(hw))[:, None, :]
    for accumulate in (0, 1):
        dx = pad(base, xs)
        dx[..., C:] = SENT
        k.globalpool_bwd(pad(dy, ys), dx, n, hw, C, xs, ys, accumulate)
        assert same(dx[..., :C], base + g if accumulate else np.broadcast_to(g, base.shape)), accumulate
        assert untouched(dx[..., C:])


@pytest.mark.parametrize("C", [1, 100, 1000])
def test_bn_running_averages(env, C):
    """r <- keep * r + alpha * batch with the step's keep = 0.9, alpha = 0.1 (Lasagne BatchNormLayer alpha = 0.1)."""
    lib, T, k = env
    rs = np.random.RandomState(C)
    rm, ri, m, i = (f32(rs.randn(C)) for _ in range(4))
    rmd, rid = c(np.append(rm, SENT)), c(np.append(ri, SENT))
    k.bn_running(rmd, c(m), rid, c(i), C, 0.9, 0.1)
    close("bn_running", rmd[:C], (1 - 0.1) * rm.astype(np.float64) + 0.1 * m, TOL)
    close("bn_running", rid[:C], (1 - 0.1) * ri.astype(np.float64) + 0.1 * i, TOL)
    assert untouched(rmd[C:]) and untouched(rid[C:])


# ----------------------------------------------------------------------------------------------------------------------
# the whole step with a saturated head
# ----------------------------------------------------------------------------------------------------------------------
def test_train_step_metrics_are_finite_when_the_head_saturates():
    """ian_train_step at B = 4 with discrimi.W scaled by 1e3 (logit gaps of hundreds): every metric finite, the four
    cross-entropy metrics within 2e-5 of the float64 twin on the same parameters."""
    import os
    from oracle import ian_oracle as O
    from oracle.train_twin import TrainTwin, make_train_params
    from neural_photo_editor_amd.trainer import Trainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B = 4
    P = make_train_params(O.make_params("IAN", 1))
    P["discrimi.W"] = (P["discrimi.W"] * np.float32(1e3)).astype(np.float32)
    X, Z = O.make_images(B, seed=0), O.make_latents(B, seed=5)
    eps = np.random.RandomState(6).randn(B, 100).astype(np.float32)
    L = {key: float(v) for key, v in TrainTwin(P, dtype=torch.float64).losses(X, Z, eps).items()}
    ce = ("discrim_d_loss", "gen_recon_loss", "gen_sample_loss", "discrim_g_loss")
    assert all(np.isfinite(L[key]) for key in L) and max(L[key] for key in ce) > 100.0, L    # saturated, and the twin is finite
    tr = Trainer(os.path.join(root, "neural_photo_editor_amd", "configs", "IAN.py"), P, B)
    m = tr.step("gen", X, Z, eps)
    tr.close()
    print("\n[train-tail] saturated step:", {key: (m[key], L[key]) for key in ce})
    assert all(np.isfinite(v) for v in m.values()), m
    for key in ce:
        assert abs(m[key] - L[key]) <= TOL * max(1.0, abs(L[key])), (key, m[key], L[key])

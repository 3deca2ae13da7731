"""The categorical cross-entropy of the discriminator head in the CPU oracles (the evaluating Theano / Lasagne stand-in of
oracle/refexec, oracle/train_twin.py, oracle/staged_twin.py): log-sum-exp form, finite for any finite logits.  The plain
-log(softmax(z)_t) form is +inf (or 0 * -inf = NaN under the one-hot sum) from a logit gap of ~745 on in float64; up to there the
two forms agree to round-off, which is why the committed reference-executed fixtures did not change (tests/test_reference_pinned.py)."""
import numpy as np
import pytest
import torch

GAPS = [0.0, 50.0, 700.0, 800.0, 5000.0]


def logits_and_reference(target):
    """one row per gap: logits (0, gap, -3); float64 logsumexp(z) - z_target"""
    z = np.array([[0.0, g, -3.0] for g in GAPS])
    zt = torch.tensor(z)
    return z, (torch.logsumexp(zt, 1) - zt[:, target]).numpy()


def check(got, ref):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), got
    assert (np.abs(got - ref) <= 1e-12 * np.maximum(np.abs(ref), 1e-300)).all(), (got, ref)


@pytest.mark.parametrize("target", [0, 1, 2])
def test_stand_in_cross_entropy_of_a_softmax_is_log_sum_exp(target):
    from oracle.refexec import minilasagne as L, minitheano as MT
    z, ref = logits_and_reference(target)
    x = MT.matrix("x")
    onehot = np.tile(np.eye(3)[target], (len(GAPS), 1)).astype(np.float32)
    ce = L.categorical_crossentropy(L.nnet_softmax(x), MT.constant(onehot))
    check(MT.function([x], ce)(z), ref)
    # any other parent keeps the plain form: -sum(t * log(q))
    q = np.array([[0.2, 0.5, 0.3], [0.9, 0.05, 0.05]])
    y = MT.matrix("y")
    plain = MT.function([y], L.categorical_crossentropy(y * 1.0, MT.constant(np.eye(3)[[target, target]].astype(np.float32))))(q)
    assert np.allclose(plain, -np.log(q[:, target]), rtol=1e-14, atol=0)


@pytest.mark.parametrize("target", [0, 1, 2])
def test_twins_cross_entropy_is_log_sum_exp(target):
    from oracle.train_twin import cross_entropy, softmax_with_logits
    z, ref = logits_and_reference(target)
    for i in range(len(GAPS)):                              # the twins take the batch mean: one sample at a time
        p = softmax_with_logits(torch.tensor(z[i:i + 1]))
        check([float(cross_entropy(p, target))], ref[i:i + 1])
    zt = torch.tensor(z, requires_grad=True)
    (g,) = torch.autograd.grad(cross_entropy(softmax_with_logits(zt), target), [zt])
    want = (torch.softmax(torch.tensor(z), 1).numpy() - np.eye(3)[target]) / len(GAPS)
    assert np.isfinite(g.numpy()).all() and np.abs(g.numpy() - want).max() <= 1e-15
    # a probability vector that is not the output of a softmax keeps -log(p_k)
    q = torch.tensor([[0.2, 0.5, 0.3]], dtype=torch.float64)
    assert abs(float(cross_entropy(q, target)) + np.log(float(q[0, target]))) < 1e-15


@pytest.mark.parametrize("twin", ["train", "staged"])
def test_twin_losses_stay_finite_with_a_saturated_head(twin):
    """The twins' whole loss dictionary with discrimi.W scaled until the float64 softmax underflows (logit gaps > 745)."""
    from oracle import ian_oracle as O
    from oracle.train_twin import TrainTwin, make_train_params
    from oracle.staged_twin import StagedTwin
    B = 2
    P = make_train_params(O.make_params("IAN", 1))
    P["discrimi.W"] = (P["discrimi.W"] * np.float32(1e4)).astype(np.float32)
    X, Z = O.make_images(B, seed=0), O.make_latents(B, seed=5)
    eps = np.random.RandomState(6).randn(B, 100).astype(np.float32)
    if twin == "train":
        tw = TrainTwin(P, dtype=torch.float64)
        L = tw.losses(X, Z, eps)
        p = tw.tensors["p_X_hat"]
    else:
        tw = StagedTwin(P, dtype=torch.float64)
        L = tw.losses_staged(X, Z, eps)
        p = tw.rec[("EH", "p")]
    assert float(p.detach().min()) == 0.0                                               # the plain form would take log(0) here
    ce = ("discrim_d_loss", "gen_recon_loss", "gen_sample_loss", "discrim_g_loss")
    L = {k: float(v.detach()) for k, v in L.items()}
    assert all(np.isfinite(v) for v in L.values()), L
    assert max(L[k] for k in ce) > 745.0

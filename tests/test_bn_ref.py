"""The yardstick of the BatchNorm kernel tests (tests/bn_ref.py) against
torch.nn.functional.batch_norm in float64 with autograd, and its mask packing.  Runs without a
GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref

EPS, MOM = float(np.float32(1e-5)), float(np.float32(0.01))
SHAPES = [(1, 1, 2, 1), (2, 3, 5, 3), (2, 4, 7, 18), (1, 12, 17, 5)]
TOL = 1e-12


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    c = shape[3]
    x = torch.randn(shape, generator=g, dtype=torch.float64) * (0.25 + 1.75 * torch.rand(c, generator=g, dtype=torch.float64)) \
        + (8 * torch.rand(c, generator=g, dtype=torch.float64) - 4)
    return dict(
        x=x, dy=torch.randn(shape, generator=g, dtype=torch.float64),
        res=torch.randn(shape, generator=g, dtype=torch.float64),
        gamma=1 + 0.3 * torch.randn(c, generator=g, dtype=torch.float64),
        beta=0.3 * torch.randn(c, generator=g, dtype=torch.float64),
        rm=torch.randn(c, generator=g, dtype=torch.float64),
        rv=0.5 + torch.rand(c, generator=g, dtype=torch.float64))


def _close(what, got, want, scale=None):
    """Agreement to TOL relative to the largest |want| (dx: to the largest of the terms it is
    the difference of, since with two pixels dx is all cancellation)."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    err = float((got - want).abs().max())
    top = float(want.abs().max()) if scale is None else float(scale.max())
    print(f"{what}: max|want| = {top:.3e}, max err = {err:.3e}")
    assert got.shape == want.shape and err <= TOL * max(top, 1e-300), what


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_training_mode_is_torch_batch_norm(shape, use_res, relu):
    d = _inputs(shape, 3 + shape[3])
    c = shape[3]
    count = shape[0] * shape[1] * shape[2]
    x, res, gamma, beta = (d[k].clone().requires_grad_() for k in ("x", "res", "gamma", "beta"))
    rm, rv = d["rm"].clone(), d["rv"].clone()
    t = F.batch_norm(_nchw(x), rm, rv, gamma, beta, True, MOM, EPS).permute(0, 2, 3, 1)
    if use_res:
        t = t + res
    y = torch.relu(t) if relu else t
    (y * d["dy"]).sum().backward()

    sums, _ = bn_ref.stats_sums(d["x"])
    fin = bn_ref.finalize(sums, count, d["gamma"], d["beta"], EPS, MOM, d["rm"], d["rv"], 7)
    save = bn_ref.save_of(fin)
    got = bn_ref.apply(d["x"], save[2], save[3], d["res"] if use_res else None, relu_on=relu)
    _close("y", got, y.detach())
    _close("running_mean", fin["running_mean"], rm)
    _close("running_var", fin["running_var"], rv)
    assert fin["num_batches_tracked"] == 8
    m = bn_ref.mask_of(got) if relu else None
    g = bn_ref.masked(d["dy"], m)
    bs, _ = bn_ref.bwd_sums(g, d["x"], save[0], save[1])
    dx, terms = bn_ref.bwd_apply(g, d["x"], save[0], save[1], d["gamma"], bs, count)
    dgamma, dbeta = bn_ref.param_grads(bs)
    _close("dx", dx, x.grad, terms)
    _close("dgamma", dgamma, gamma.grad)
    _close("dbeta", dbeta, beta.grad)
    if use_res:
        _close("dres", g, res.grad)
    # SyncBN's call: twice the count with doubled sums is the same two-rank batch
    dx2, _ = bn_ref.bwd_apply(g, d["x"], save[0], save[1], d["gamma"], 2 * bs, 2 * count)
    _close("dx (count 2P, sums doubled)", dx2, x.grad, terms)
    # accumulation onto earlier parameter gradients
    dg2, db2 = bn_ref.param_grads(bs, d["rm"], d["rv"])
    _close("dgamma +=", dg2, gamma.grad + d["rm"])
    _close("dbeta +=", db2, beta.grad + d["rv"])
    assert c == dgamma.numel()


@pytest.mark.parametrize("shape", SHAPES)
def test_shifted_statistics_give_the_same_save(shape):
    d = _inputs(shape, 11)
    count = shape[0] * shape[1] * shape[2]
    shift = d["rm"] * 3
    plain = bn_ref.finalize(bn_ref.stats_sums(d["x"])[0], count, d["gamma"], d["beta"], EPS, MOM,
                            d["rm"], d["rv"], 0, dtype=np.longdouble)
    shifted = bn_ref.finalize(bn_ref.stats_sums(d["x"], shift)[0], count, d["gamma"], d["beta"],
                              EPS, MOM, d["rm"], d["rv"], 0, mean_shift=shift, dtype=np.longdouble)
    for k in ("mean", "invstd", "scale", "shift", "running_mean", "running_var"):
        a, b = np.asarray(plain[k], dtype=np.float64), np.asarray(shifted[k], dtype=np.float64)
        assert np.abs(a - b).max() <= 1e-11 * np.abs(a).max(), k  # (the sums are doubles)


def test_finalize_edges():
    # count 1: the unbiased variance is the biased one (0); var < 0 is clamped; NULL gamma / beta
    fin = bn_ref.finalize(torch.tensor([[3.0, 2.0], [9.0, 3.9]]), 1, None, None, EPS, MOM,
                          torch.zeros(2), torch.ones(2), 0)
    assert np.array_equal(fin["var"], [0.0, 0.0])
    assert np.allclose(fin["invstd"], 1 / np.sqrt(EPS)) and np.array_equal(fin["scale"], fin["invstd"])
    assert np.allclose(fin["running_var"], 1 - MOM) and np.allclose(fin["running_mean"], [3 * MOM, 2 * MOM])
    assert np.allclose(fin["shift"], -fin["mean"] * fin["invstd"])


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_eval_mode_is_torch_batch_norm(shape, relu):
    d = _inputs(shape, 5)
    res = d["res"].clone().requires_grad_()
    t = F.batch_norm(_nchw(d["x"]), d["rm"], d["rv"], d["gamma"], d["beta"], False, MOM, EPS)
    t = t.permute(0, 2, 3, 1) + res
    y = torch.relu(t) if relu else t
    (y * d["dy"]).sum().backward()
    save = bn_ref.eval_coeffs(d["gamma"], d["beta"], d["rm"], d["rv"], EPS)
    got = bn_ref.apply(d["x"], save[2], save[3], d["res"], relu_on=relu)
    _close("y (eval)", got, y.detach())
    _close("dres (eval)", bn_ref.masked(d["dy"], bn_ref.mask_of(got) if relu else None), res.grad)
    _close("mean, invstd", save[:2], torch.stack([d["rm"], 1 / torch.sqrt(d["rv"] + EPS)]))
    none = bn_ref.eval_coeffs(None, None, d["rm"], d["rv"], EPS)
    _close("NULL gamma / beta", none[2:], torch.stack([save[1], -d["rm"] * save[1]]))


def test_residual_bn_apply_and_backward_are_two_batch_norms():
    shape = (2, 3, 5, 6)
    d, e = _inputs(shape, 21), _inputs(shape, 22)
    count = 30
    x, rx = d["x"].clone().requires_grad_(), e["x"].clone().requires_grad_()
    t = F.batch_norm(_nchw(x), None, None, d["gamma"], d["beta"], True, MOM, EPS) + \
        F.batch_norm(_nchw(rx), None, None, e["gamma"], e["beta"], True, MOM, EPS)
    y = torch.relu(t).permute(0, 2, 3, 1)
    (y * d["dy"]).sum().backward()
    s = bn_ref.save_of(bn_ref.finalize(bn_ref.stats_sums(d["x"])[0], count, d["gamma"], d["beta"], EPS))
    r = bn_ref.save_of(bn_ref.finalize(bn_ref.stats_sums(e["x"])[0], count, e["gamma"], e["beta"], EPS))
    got = bn_ref.apply(d["x"], s[2], s[3], rx=e["x"], rscale=r[2], rshift=r[3], relu_on=True)
    _close("y", got, y.detach())
    g = bn_ref.masked(d["dy"], bn_ref.mask_of(got))
    for tag, inp, sv, gm, leaf in (("dx", d["x"], s, d["gamma"], x), ("rdx", e["x"], r, e["gamma"], rx)):
        bs, _ = bn_ref.bwd_sums(g, inp, sv[0], sv[1])
        _close(tag, bn_ref.bwd_apply(g, inp, sv[0], sv[1], gm, bs, count)[0], leaf.grad)


def test_mask_semantics_and_packing():
    tiny = float(np.finfo(np.float32).tiny)
    y = torch.tensor([0.0, -0.0, tiny, -tiny, float("nan"), float("inf"), 1.0, -1.0, 2.0, 0.0])
    m = bn_ref.mask_of(y)
    assert m.tolist() == [False, False, True, False, False, True, True, False, True, False]
    g = bn_ref.masked(torch.arange(1.0, 11.0), m)
    assert g.tolist() == [0, 0, 3, 0, 0, 6, 7, 0, 9, 0]
    assert bn_ref.relu(torch.tensor([float("nan")])).isnan().all()  # NaN propagates forward
    mm = m.view(1, 1, 2, 5)  # two pixels of 5 channels: two quads each, the second partial
    b0, b1 = bn_ref.pack_mask(mm, 0), bn_ref.pack_mask(mm, 1)
    assert b0.shape == (2, 2) and b0.dtype == torch.uint8
    assert b0.tolist() == [[0b0100, 0b0000], [0b1011, 0b0000]]  # bit k of [p][q] = channel 4q + k
    assert b1.tolist() == [[0b0100, 0b1110], [0b1011, 0b1110]]  # the padding bits alone differ
    for b in (b0, b1):
        assert torch.equal(bn_ref.unpack_mask(b, 5), mm.view(2, 5))

"""FullModel_encdec(ssim_lambda=...): off it is the model it was (same bits, no SSIM launch); on,
every L1 reconstruction term has its SSIM sibling in loss_all, the step captures into a
StepGraph, and frames below the window are refused.  Tiny arch, B = 2, 32 x 64."""
import ctypes

import pytest
import torch

from helpers import build, make_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, HW = 2, (32, 64)
LAMS = (1.0, 0.1, 0.7)  # X1 / X2 / X3RECON_LAMBDA


def _setup(ssim_lambda=None, hw=HW, seed=0, **cfg_kw):
    from vae2.model import FullModel_encdec
    from vae2.optim import FusedAdam
    ed, ez = build(make_cfg("tiny", hw=hw, **cfg_kw), seed=seed)
    kw = {} if ssim_lambda is None else dict(ssim_lambda=ssim_lambda)
    fm = FullModel_encdec(ez, ed, None, None, None, None, None, *LAMS, 0.0, **kw).to(DEV)
    fm.train()
    fm.defer_checks = True
    opt = FusedAdam([m for m in (fm.encz_model, fm.encdec_model) if m is not None], lr=1e-3)
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(B, 9, *hw, generator=g).to(DEV) for _ in range(3)]
    eps = torch.randn(B, ed.z_dim, 1, 1, generator=g).to(DEV)
    code = torch.randn(B, ed.z_dim, 1, 1, generator=g).to(DEV)
    baseline = dict(is_baseline=True, baseline_mode=cfg_kw["mode"]) if cfg_kw else {}

    def fwd():
        opt.zero_grad()
        fm.set_noise(eps, code)
        return fm(*xs, 1.0, **baseline)
    return fm, opt, fwd


def _logged(fn):
    """fn() and the names of the kernels it launched, forward and backward.  The library's
    launch log is per thread and autograd runs the backward on a thread of its own, so the log
    is read around every C-ABI call, on the thread that makes it (as vae2.prof does)."""
    from vae2 import _lib
    lib = _lib.load()
    names = []

    def hook(name, f, args):
        lib.vae2_kernel_log_read(None, 0)  # drop what this thread logged outside a call
        rc = f(*args)
        buf = ctypes.create_string_buffer(1 << 16)
        if lib.vae2_kernel_log_read(buf, len(buf)):
            names.extend(buf.value.decode().split(";"))
        return rc
    lib.vae2_kernel_log(1)
    _lib.CALL_HOOK = hook
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.CALL_HOOK = None
        lib.vae2_kernel_log(0)
    return out, names


def _step(fwd):
    def f():
        res = fwd()
        res[0][0].backward()
        return res
    return f


def _grads(opt):
    return torch.cat([f.grad.reshape(-1) for f in opt.flats])


def test_lambda_zero_is_the_model_without_the_argument():
    fa, oa, wa = _setup(None)
    fb, ob, wb = _setup(0.0)
    (la, *pa), names_a = _logged(_step(wa))
    (lb, *pb), names_b = _logged(_step(wb))
    assert fb.ssim_terms is None and fa.ssim_terms is None
    assert names_a == names_b and len(names_a) > 100
    assert not [n for n in names_b if "ssim_loss" in n]
    for x, y in zip(la, lb):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    assert torch.equal(_grads(oa), _grads(ob))


def test_lambda_adds_the_weighted_terms():
    lam = 0.5
    f0, o0, w0 = _setup(0.0)
    f1, o1, w1 = _setup(lam)
    (l0, *p0) = _step(w0)()
    (l1, *p1), names = _logged(_step(w1))
    assert [n for n in names if "ssim_loss" in n].count("ssim_loss_fwd_kernel") == 3
    assert names.count("ssim_loss_finish_kernel") == 3
    assert names.count("ssim_loss_bwd_kernel") == 3
    # the predictions and the seven reference-shaped entries but loss_all are unchanged
    for x, y in zip(p0, p1):
        assert torch.equal(x, y)
    assert len(l1) == 7
    for x, y in zip(l0[1:], l1[1:]):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))
    terms = f1.ssim_terms
    assert isinstance(terms, tuple) and len(terms) == 3
    assert all(t.is_cuda and t.shape == () for t in terms)
    vals = [float(t) for t in terms]
    top = 9 * (HW[0] - 10) * (HW[1] - 10) * 2.0  # 1 - ssim is in [0, 2]; sum over B / B
    assert all(0.0 < v <= top for v in vals), vals
    want = float(l0[0]) + sum(lam * k * v for k, v in zip(LAMS, vals))
    got = float(l1[0])
    # two nested fp32 weighted sums (3 and 5 terms: 8 products, 6 additions), every rounding
    # at most 2^-24 of the terms' total magnitude
    mag = abs(float(l0[0])) + sum(abs(lam * k * v) for k, v in zip(LAMS, vals))
    print(f"loss_all {got!r} want {want!r} ssim terms {vals}")
    assert abs(got - want) <= 16 * 2.0 ** -24 * mag
    g0, g1 = _grads(o0), _grads(o1)
    assert bool(torch.isfinite(g1).all()) and not torch.equal(g0, g1)
    # the terms are live scalars of this forward: None again once the switch is off
    f1.ssim_lambda = 0.0
    w1()
    assert f1.ssim_terms is None


def test_baseline_mode_has_one_term():
    fm, opt, fwd = _setup(0.5, baseline=True, mode="DETERMINISTIC")
    (losses, *_), names = _logged(_step(fwd))
    assert names.count("ssim_loss_fwd_kernel") == 1
    assert names.count("ssim_loss_bwd_kernel") == 1
    assert len(fm.ssim_terms) == 1 and float(fm.ssim_terms[0]) > 0
    assert bool(torch.isfinite(_grads(opt)).all())
    want = LAMS[1] * float(losses[2]) + 0.5 * LAMS[1] * float(fm.ssim_terms[0])
    assert abs(float(losses[0]) - want) <= 8 * 2.0 ** -24 * abs(want)


def test_graph_replay_matches_eager():
    from vae2.graph import StepGraph

    def full(opt, fwd):
        def f():
            loss = fwd()[0][0]
            loss.backward()
            opt.step()
            return loss
        return f
    fa, oa, wa = _setup(0.5)
    fb, ob, wb = _setup(0.5)
    step_a, step_b = full(oa, wa), full(ob, wb)
    losses_a = [float(step_a()) for _ in range(5)]
    g = StepGraph(step_b, warmup=2)  # executes 2 eager steps, captures the 3rd
    losses_b = [float(g.replay()) for _ in range(3)]
    torch.cuda.synchronize()
    assert losses_a[2:] == losses_b, (losses_a, losses_b)
    assert len(set(losses_a)) == 5  # the steps do change the loss
    for x, y in zip(oa.flats, ob.flats):
        assert torch.equal(x.data, y.data)
    assert oa.step_count == ob.step_count == 5


def test_small_frames_are_refused():
    fm, opt, fwd = _setup(0.5, hw=(8, 8))
    with pytest.raises(ValueError, match="MI355X.SSIM_LAMBDA"):
        fwd()

"""vae2_sgd_coeffs / vae2_sgd_step_dev / vae2_sgd_step and vae2.optim.FusedSGD against
torch.optim.SGD.

Truth is torch.optim.SGD on the CPU in fp64 from the same fp32 inputs; the yardstick is
torch.optim.SGD on the CPU in fp32.  With err(x) = max|x - x64| a result x passes when

    err(gpu) <= 2 * err(cpu_fp32) + 2^-23 * max|x64|

for the parameters and for the momentum buffers: the factor 2 allows for a different
contraction and ordering of the multiply-adds between two fp32 evaluations, the floor is one
fp32 rounding of the largest value."""
import functools

import pytest
import torch

from helpers import build, make_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR = 0.05
STEPS = 5

# the last size takes a second grid-stride pass of the 16-byte body plus a ragged tail
SIZES = [1, 3, 4, 5, 1023, 4 * 256 * 4096 + 7]
CONFIGS = {
    "plain": dict(),
    "wd": dict(weight_decay=1e-2),
    "mom": dict(momentum=0.9),
    "mom_damp": dict(momentum=0.9, dampening=0.1),
    "nesterov": dict(momentum=0.9, nesterov=True),
    "nesterov_wd": dict(momentum=0.9, weight_decay=1e-2, nesterov=True),
}


@functools.lru_cache(maxsize=None)
def _inputs(n):
    g = torch.Generator().manual_seed(1000 + n % 997)
    return torch.randn(n, generator=g), tuple(torch.randn(n, generator=g) for _ in range(STEPS))


def _torch_sgd(p0, grads, dtype, buf0=None, lr=LR, **kw):
    """(p, momentum buffer or None) after torch.optim.SGD steps on the CPU in dtype."""
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.SGD([p], lr=lr, **kw)
    if buf0 is not None:
        opt.state[p]["momentum_buffer"] = buf0.to(dtype).clone()
    for g in grads:
        p.grad = g.to(dtype)
        opt.step()
    return p.detach(), opt.state[p].get("momentum_buffer")


@functools.lru_cache(maxsize=None)
def _reference(n, cfg):
    p0, grads = _inputs(n)
    return _torch_sgd(p0, grads, torch.float64, **CONFIGS[cfg]), \
        _torch_sgd(p0, grads, torch.float32, **CONFIGS[cfg])


def _check(what, got, x32, x64):
    e_gpu = float((got.double().cpu() - x64).abs().max())
    e_cpu = float((x32.double() - x64).abs().max())
    bound = 2.0 * e_cpu + 2.0 ** -23 * float(x64.abs().max())
    print(f"{what}: err(gpu)={e_gpu:.3e} err(cpu_fp32)={e_cpu:.3e} bound={bound:.3e}")
    assert e_gpu <= bound, (what, e_gpu, e_cpu, bound)


GUARD = 8  # sentinel floats around every device buffer: nothing outside [0, n) is written


def _dev_buf(src, offset, fill=None):
    n = src.numel()
    raw = torch.full((offset + n + GUARD,), 777.0, device=DEV)
    view = raw[offset:offset + n]
    if fill is None:
        view.copy_(src)
    else:
        view.fill_(fill)
    return raw, view


def _guards_ok(raw, offset, n):
    return bool((raw[:offset] == 777.0).all()) and bool((raw[offset + n:] == 777.0).all())


def _run_kernel(n, cfg, offset=0, host_scalar=False):
    """STEPS steps through the C ABI; the momentum buffer starts as NaN (the first step must
    not read it)."""
    from vae2 import ops
    from vae2._lib import call
    kw = CONFIGS[cfg]
    mom, damp = kw.get("momentum", 0.0), kw.get("dampening", 0.0)
    wd, nes = kw.get("weight_decay", 0.0), int(kw.get("nesterov", False))
    p0, grads = _inputs(n)
    praw, p = _dev_buf(p0, offset)
    graw, g = _dev_buf(grads[0], offset)
    braw, b = _dev_buf(p0, offset, fill=float("nan")) if mom else (None, None)
    state = torch.tensor([0.0, LR], dtype=torch.float64, device=DEV)
    coeffs = torch.zeros(4, device=DEV)
    s = ops.stream_ptr()
    for k, gk in enumerate(grads):
        g.copy_(gk)
        if host_scalar:
            call("vae2_sgd_step", ops.ptr(p), ops.ptr(g), ops.ptr(b), n, LR, mom, damp, wd, nes,
                 int(k == 0), s)
        else:
            call("vae2_sgd_coeffs", ops.ptr(state), mom, damp, nes, ops.ptr(coeffs), s)
            call("vae2_sgd_step_dev", ops.ptr(p), ops.ptr(g), ops.ptr(b), n, ops.ptr(coeffs),
                 mom, wd, nes, s)
    torch.cuda.synchronize()
    assert _guards_ok(praw, offset, n) and _guards_ok(graw, offset, n)
    assert braw is None or _guards_ok(braw, offset, n)
    assert torch.equal(g.cpu(), grads[-1])  # the gradient is read only
    if not host_scalar:
        assert float(state[0]) == STEPS and float(state[1]) == LR
    return p.cpu(), (b.cpu() if b is not None else None)


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("n", SIZES)
def test_sgd_kernel_matches_torch(n, cfg):
    (p64, b64), (p32, b32) = _reference(n, cfg)
    p, b = _run_kernel(n, cfg)
    _check(f"p n={n} {cfg}", p, p32, p64)
    assert (b is None) == (b64 is None)
    if b is not None:
        _check(f"buf n={n} {cfg}", b, b32, b64)


def test_sgd_kernel_misaligned_pointers():
    """p, g and buf one float into their allocations: the scalar path, same numbers."""
    n, cfg = 1023, "mom_damp"
    (p64, b64), (p32, b32) = _reference(n, cfg)
    p, b = _run_kernel(n, cfg, offset=1)
    _check("p misaligned", p, p32, p64)
    _check("buf misaligned", b, b32, b64)
    pa, ba = _run_kernel(n, cfg)  # the 16-byte path evaluates the same expression
    assert torch.equal(p, pa) and torch.equal(b, ba)


def test_sgd_host_scalar_form_same_bits():
    n, cfg = 1023, "mom_damp"
    p, b = _run_kernel(n, cfg)
    ph, bh = _run_kernel(n, cfg, host_scalar=True)
    assert torch.equal(p, ph) and torch.equal(b, bh)


# ------------------------------------------------------------------ FusedSGD ----

def _tiny_sgd(seed=0, grad_seed=3, **kw):
    from vae2.optim import FusedSGD
    ed, ez = build(make_cfg("tiny"), seed=seed)
    ed.to(DEV), ez.to(DEV)
    opt = FusedSGD([ez, ed], **kw)
    _fill_grads(opt, grad_seed)
    return opt


def _fill_grads(opt, seed):
    g = torch.Generator().manual_seed(seed)
    for f in opt.flats:
        f.grad.copy_(torch.randn(f.numel, generator=g))
    return [f.grad.cpu().clone() for f in opt.flats]


def test_first_step_semantics_under_replay():
    """A graph captured before the first step: replay 1 takes buf = g, replays 2 and 3 apply
    the dampening (the device step counter decides, not the capture)."""
    from vae2.graph import StepGraph
    kw = dict(lr=LR, momentum=0.9, dampening=0.1)
    a, b = _tiny_sgd(**kw), _tiny_sgd(**kw)
    p0 = [f.data.cpu().clone() for f in a.flats]
    g0 = [f.grad.cpu().clone() for f in a.flats]
    assert a.state_dict()["state"] == {}  # no momentum_buffer before a step, as torch
    for _ in range(3):
        a.step()
    graph = StepGraph(b.step, warmup=0)
    assert b.step_count == 0  # the capture itself ran nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert a.step_count == b.step_count == 3
    for fa, fb, ma, mb in zip(a.flats, b.flats, a.momentum_buffer, b.momentum_buffer):
        assert torch.equal(fa.data, fb.data)
        assert torch.equal(ma, mb)
    for k, (x0, g) in enumerate(zip(p0, g0)):
        tkw = dict(momentum=0.9, dampening=0.1)
        p64, b64 = _torch_sgd(x0, [g] * 3, torch.float64, **tkw)
        p32, b32 = _torch_sgd(x0, [g] * 3, torch.float32, **tkw)
        _check(f"replayed p[{k}]", b.flats[k].data, p32, p64)
        _check(f"replayed buf[{k}]", b.momentum_buffer[k], b32, b64)


def _setup(arch, B, hw, seed=0):
    from vae2.model import FullModel_encdec
    from vae2.optim import FusedSGD
    ed, ez = build(make_cfg(arch, hw=hw), seed=seed)
    fm = FullModel_encdec(ez, ed, None, None, None, None, None, 1.0, 0.1, 1.0, 0.0).to(DEV)
    fm.train()
    fm.defer_checks = True
    opt = FusedSGD([fm.encz_model, fm.encdec_model], lr=1e-2, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(B, 9, *hw, generator=g).to(DEV) for _ in range(3)]
    eps = torch.randn(B, ez.z_dim, 1, 1, generator=g).to(DEV)
    code = torch.randn(B, ez.z_dim, 1, 1, generator=g).to(DEV)

    def step():
        opt.zero_grad()
        fm.set_noise(eps, code)
        loss = fm(*xs, 1.0)[0][0]
        loss.backward()
        opt.step()
        return loss
    return fm, opt, step


def test_whole_sgd_step_graph_replay_matches_eager():
    from vae2.graph import StepGraph
    fa, oa, step_a = _setup("tiny", 2, (32, 64))
    fb, ob, step_b = _setup("tiny", 2, (32, 64))
    losses_a = [float(step_a()) for _ in range(5)]
    g = StepGraph(step_b, warmup=2)  # executes 2 eager steps, captures the 3rd
    losses_b = [float(g.replay()) for _ in range(3)]
    torch.cuda.synchronize()
    assert losses_a[2:] == losses_b, (losses_a, losses_b)
    # the pack refresh ran and the updated weights were used: every step sees a new loss
    assert len(set(losses_a)) == 5, losses_a
    for fa_, fb_ in zip(oa.flats, ob.flats):
        assert torch.equal(fa_.data, fb_.data)
    for ma, mb in zip(oa.momentum_buffer, ob.momentum_buffer):
        assert torch.equal(ma, mb) and float(ma.abs().max()) > 0
    assert oa.step_count == ob.step_count == 5
    ba = dict(fa.named_buffers())
    for name, buf in fb.named_buffers():
        assert torch.equal(buf, ba[name]), name
    # the device learning rate is honoured without a recapture
    before = [f.data.clone() for f in ob.flats]
    ob.set_lr(0.0)
    g.replay()
    torch.cuda.synchronize()
    assert ob.step_count == 6
    for f, x in zip(ob.flats, before):
        assert torch.equal(f.data, x)


def test_checkpoint_loads_into_torch_sgd():
    kw = dict(lr=LR, momentum=0.9, weight_decay=1e-4)
    opt = _tiny_sgd(**kw)
    opt.step()
    _fill_grads(opt, 4)
    opt.step()
    sd = opt.state_dict()
    params = opt.param_groups[0]["params"]
    assert sorted(sd["state"]) == list(range(len(params)))
    assert sd["param_groups"][0]["params"] == list(range(len(params)))
    topt = torch.optim.SGD(params, **kw)
    topt.load_state_dict(sd)
    for i, p in enumerate(params):
        tb = topt.state[p]["momentum_buffer"]
        assert tb.shape == p.shape
        assert torch.equal(tb, sd["state"][i]["momentum_buffer"].to(tb.device))
    grp = topt.param_groups[0]
    assert (grp["lr"], grp["momentum"], grp["weight_decay"], grp["nesterov"]) == \
        (LR, 0.9, 1e-4, False)


def test_torch_sgd_checkpoint_loads_into_fused_sgd():
    kw = dict(momentum=0.9, dampening=0.1, weight_decay=1e-4)
    opt = _tiny_sgd(lr=123.0)  # every hyper-parameter comes from the checkpoint
    params = opt.param_groups[0]["params"]
    gen = torch.Generator().manual_seed(11)
    # a torch-written state: two fp32 CPU steps from the same initial parameters
    tp = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    topt = torch.optim.SGD(tp, lr=LR, **kw)
    for _ in range(2):
        for p in tp:
            p.grad = torch.randn(p.shape, generator=gen)
        topt.step()
    sd = topt.state_dict()
    with torch.no_grad():
        for p, q in zip(params, tp):
            p.copy_(q)
    opt.load_state_dict(sd)
    assert opt.step_count >= 1  # the next step is not a first step
    ours = opt.state_dict()["state"]  # every buffer landed in its parameter's slice
    for i in range(len(params)):
        assert torch.equal(ours[i]["momentum_buffer"].cpu(), sd["state"][i]["momentum_buffer"])
    assert (opt.lr, opt.momentum, opt.dampening, opt.weight_decay, opt.nesterov) == \
        (LR, 0.9, 0.1, 1e-4, False)
    # the third step of both on the same gradients
    g3 = _fill_grads(opt, 12)
    x0 = [f.data.cpu().clone() for f in opt.flats]
    b0 = [m.cpu().clone() for m in opt.momentum_buffer]
    opt.step()
    torch.cuda.synchronize()
    for k, f in enumerate(opt.flats):
        p64, b64 = _torch_sgd(x0[k], [g3[k]], torch.float64, buf0=b0[k], **kw)
        p32, b32 = _torch_sgd(x0[k], [g3[k]], torch.float32, buf0=b0[k], **kw)
        _check(f"resumed p[{k}]", f.data, p32, p64)
        _check(f"resumed buf[{k}]", opt.momentum_buffer[k], b32, b64)


def test_optimizer_kind_mismatch_is_a_clear_error():
    from vae2.optim import FusedAdam, FusedSGD
    ed, ez = build(make_cfg("tiny"), seed=0)
    ed.to(DEV), ez.to(DEV)
    adam = FusedAdam([ez, ed], lr=1e-3)
    sgd = FusedSGD([ez, ed], lr=LR, momentum=0.9)
    with pytest.raises(ValueError, match="exp_avg"):
        sgd.load_state_dict(adam.state_dict())
    _fill_grads(sgd, 5)
    sgd.step()
    with pytest.raises(ValueError, match="momentum_buffer"):
        adam.load_state_dict(sgd.state_dict())

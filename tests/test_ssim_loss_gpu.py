"""vae2_ssim_loss_fwd / _bwd (csrc/ssim_loss.hip) against the fp64 restatement of
tests/ssim_ref.py, through the C ABI on sentinel-padded buffers, and the autograd op and
criterion on top of them.

Tolerance (set by the yardstick, not by the kernel): the kernel and the fp32 restatement are two
fp32 evaluations of one expression that differ in summation order and FMA use, so the kernel's
error against fp64 may be up to 4 x the fp32 restatement's own error on the same inputs,
floored at 2^-22 of the reference (the loss) or of the gradient's maximum.  Every case prints
its ratio err(kernel) / err(fp32 restatement).

Shapes: one output pixel per plane; partial tiles and an odd width; several forward (16 x 32
of the valid map) and backward (16 x 16) tiles in both directions; the two degenerate axes.
Each runs dense (ps = c) and as channels [1, 1 + c) of a 12-channel buffer that starts one
float into its allocation.

Measured on an MI355X (ratio err(kernel) / err(fp32 restatement), the bound being 4): the largest
is 1.83 in the backward ((1, 11, 140, 2), p near t, no coefficients) and 1.55 in the forward
((1, 140, 11, 2), the same kind of inputs); the forward's ratio is exactly 1.000 in 7 of the 30
distinct cases (the kernel returns the restatement's fp32 value) and at most 0.014 for constant
images.  The yardstick's own errors are 9e-9 to 3e-6 relative on the loss for noisy images and
7e-6 to 2e-4 for constant ones; 1e-7 to 4e-6 of the gradient's maximum for noisy images and up
to 2e-3 for constant ones.  A first version of
the kernels with the textbook arithmetic (e11 - mu1^2 unshifted, 1 - l cs) passed the backward
everywhere (largest ratio 2.9) but missed the forward bound in 5 of the 30 cases, constant
images at 4.2 - 6.8 and (1, 140, 11, 2) near-with-coefficients at 35; csrc/ssim_loss.hip and
DESIGN.md say what was changed and why.
"""
import functools

import pytest
import torch

import kparity as kp
import ssim_ref

pytestmark = pytest.mark.gpu

SHAPES = [(2, 11, 11, 3), (1, 12, 37, 9), (2, 45, 77, 9), (1, 11, 140, 2), (1, 140, 11, 2)]
LAYOUTS = ["dense", "slice"]
KINDS = ["near", "indep", "const"]
C1, C2 = ssim_ref.C1, ssim_ref.C2
SCALE = 0.5
GOUT = 1.25


def _slice(x, layout, sent=kp.SENT):
    if layout == "dense":
        return kp.Slice(x, sent=sent)
    return kp.Slice(x, ps=12, c0=1, offset=1, sent=sent)


@functools.lru_cache(maxsize=None)
def _case(shape, kind, affine):
    """Inputs and references of one case, computed once on the host and shared (read only)."""
    p, t = ssim_ref.make_inputs(shape, kind, seed=1 + SHAPES.index(shape))
    a, b = ssim_ref.coeffs(shape[3]) if affine else (None, None)
    l64 = float(ssim_ref.loss(p, t, SCALE, a, b))
    l32 = float(ssim_ref.loss(p, t, SCALE, a, b, dtype=torch.float32))
    g64 = ssim_ref.grad_autograd(p, t, SCALE, a, b, gout=GOUT)
    g32 = ssim_ref.grad_autograd(p, t, SCALE, a, b, dtype=torch.float32, gout=GOUT).double()
    return p, t, a, b, l64, l32, g64, g32


def _dev(x):
    return None if x is None else x.to(kp.DEV)


def _fwd(ps, ts, a, b, scale=SCALE, c1=C1, c2=C2):
    call, lib, ptr, st = kp.abi()
    ws = torch.empty(lib.vae2_ssim_loss_ws_size(ps.ref), dtype=torch.float64, device=kp.DEV)
    out = kp.scalar()
    call("vae2_ssim_loss_fwd", ps.ptr, ps.ref, ts.ptr, ts.ref, ptr(a), ptr(b), c1, c2, scale,
         ptr(ws), out.ptr, st)
    assert out.intact()
    return out.read().reshape(())


def _bwd(ps, ts, a, b, dps, gout=GOUT, scale=SCALE, beta=0.0, c1=C1, c2=C2):
    call, lib, ptr, st = kp.abi()
    g = kp.scalar(gout)
    call("vae2_ssim_loss_bwd", ps.ptr, ps.ref, ts.ptr, ts.ref, ptr(a), ptr(b), c1, c2, g.ptr,
         scale, dps.ptr, dps.ref, beta, st)
    assert g.intact() and float(g.read()) == gout
    return dps.read()


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_and_backward_against_fp64(shape, layout, kind, affine):
    p, t, a, b, l64, l32, g64, g32 = _case(shape, kind, affine)
    ps, ts = _slice(p, layout), _slice(t, layout)
    da, db = _dev(a), _dev(b)
    out = float(_fwd(ps, ts, da, db))
    e_k, e_y = abs(out - l64), abs(l32 - l64)
    bound = max(4 * e_y, 2.0 ** -22 * abs(l64))
    print(f"fwd {shape} {layout} {kind} affine={affine}: out={out!r} fp64={l64!r} "
          f"err={e_k:.3e} err(fp32 restatement)={e_y:.3e} ratio={e_k / max(e_y, 1e-300):.3f} "
          f"bound={bound:.3e}")
    dps = _slice(torch.full(shape, float("nan")), layout)
    dp = _bwd(ps, ts, da, db, dps).double()
    top = float(g64.abs().max())
    ge_k, ge_y = float((dp - g64).abs().max()), float((g32 - g64).abs().max())
    gbound = max(4 * ge_y, 2.0 ** -22 * top)
    print(f"bwd {shape} {layout} {kind} affine={affine}: max|grad|={top:.3e} err={ge_k:.3e} "
          f"err(fp32 restatement)={ge_y:.3e} ratio={ge_k / max(ge_y, 1e-300):.3f} "
          f"bound={gbound:.3e}")
    # nothing outside the views is written, and the operands are not written at all
    assert ps.intact() and ts.intact() and dps.intact()
    assert kp.same_bits(ps.read(), p) and kp.same_bits(ts.read(), t)
    assert e_k <= bound, ("forward", out, l64, e_k, bound)
    assert bool(torch.isfinite(dp).all()) and ge_k <= gbound, ("backward", ge_k, gbound)


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_identical_inputs_give_exact_zero(shape, layout, affine):
    p, _, a, b = _case(shape, "near", affine)[:4]
    ps, ts = _slice(p, layout), _slice(p.clone(), layout)
    da, db = _dev(a), _dev(b)
    out = _fwd(ps, ts, da, db)
    assert float(out) == 0.0
    dp = _bwd(ps, ts, da, db, _slice(torch.full(shape, float("nan")), layout))
    amax = float(a.abs().max()) if affine else 1.0
    print(f"p == t {shape} {layout} affine={affine}: max|dp| = {float(dp.abs().max()):.3e}")
    assert float(dp.abs().max()) <= 2.0 ** -20 * SCALE * amax


@pytest.mark.parametrize("layout", LAYOUTS)
def test_beta_one_accumulates(layout):
    shape = (2, 45, 77, 9)
    p, t, a, b = _case(shape, "near", True)[:4]
    ps, ts, da, db = _slice(p, layout), _slice(t, layout), _dev(a), _dev(b)
    dp0 = _bwd(ps, ts, da, db, _slice(torch.zeros(shape), layout))
    prev = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    dps = _slice(prev, layout)
    dp1 = _bwd(ps, ts, da, db, dps, beta=1.0)
    kp.check_bits("beta = 1", dp1, dp0 + prev)  # one fp32 add on each side
    assert dps.intact()
    kp.check_bits("beta = 0 overwrites", _bwd(ps, ts, da, db, _slice(prev, layout)), dp0)


def test_gout_and_scale_are_linear():
    shape = (1, 12, 37, 9)
    p, t, a, b = _case(shape, "indep", True)[:4]
    ps, ts, da, db = _slice(p, "dense"), _slice(t, "dense"), _dev(a), _dev(b)

    def grad(gout, scale):
        return _bwd(ps, ts, da, db, _slice(torch.zeros(shape), "dense"), gout=gout, scale=scale)
    base = grad(1.0, 0.5)
    # powers of two commute with every rounding
    kp.check_bits("gout x 2", grad(2.0, 0.5), 2 * base)
    kp.check_bits("scale x 4", grad(1.0, 2.0), 4 * base)
    kp.check_bits("scale x 4 (forward)", _fwd(ps, ts, da, db, scale=2.0),
                  4 * _fwd(ps, ts, da, db, scale=0.5))
    # any other factor: the product scale * gout * a_c is rounded once more
    g3 = grad(3.0, 0.5).double()
    err = (g3 - 3 * base.double()).abs()
    assert bool((err <= 4 * kp.U * (3 * base.double()).abs()).all()), float(err.max())
    l1, l3 = float(_fwd(ps, ts, da, db, scale=0.5)), float(_fwd(ps, ts, da, db, scale=1.5))
    assert abs(l3 - 3 * l1) <= 2 * kp.U * abs(l3)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_runs_are_bit_identical(layout):
    shape = (2, 45, 77, 9)
    p, t, a, b = _case(shape, "indep", True)[:4]
    ps, ts, da, db = _slice(p, layout), _slice(t, layout), _dev(a), _dev(b)
    outs = [_fwd(ps, ts, da, db) for _ in range(2)]
    kp.check_bits("forward twice", outs[1], outs[0])
    dps = [_bwd(ps, ts, da, db, _slice(torch.zeros(shape), layout)) for _ in range(2)]
    kp.check_bits("backward twice", dps[1], dps[0])
    # and a differently placed copy of the same data gives the same bits
    other = "slice" if layout == "dense" else "dense"
    kp.check_bits("forward, other layout", _fwd(_slice(p, other), _slice(t, other), da, db),
                  outs[0])


@pytest.mark.parametrize("view", ["dense", "padded"])
def test_autograd_op_is_the_abi_calls(view):
    """ops.ssim_loss == the direct calls, bit for bit; 'padded': an NHWC view with ps > c (what
    ops.new_act hands out for 9 channels)."""
    from vae2 import ops
    shape = (2, 45, 77, 9)
    p, t, a, b = _case(shape, "near", True)[:4]
    da, db = _dev(a), _dev(b)
    if view == "dense":
        pv, tv = p.to(kp.DEV), t.to(kp.DEV)
    else:
        pv, tv = ops.new_act(shape, da), ops.new_act(shape, da)
        assert pv.stride(2) == 12
        pv.copy_(p)
        tv.copy_(t)
    pv.requires_grad_(True)
    loss = ops.ssim_loss(pv, tv, SCALE, da, db)
    assert loss.shape == () and loss.is_cuda
    (GOUT * loss).backward()
    assert tv.grad is None
    ps, ts = _slice(p, "dense"), _slice(t, "dense")
    kp.check_bits("loss", loss.detach().cpu(), _fwd(ps, ts, da, db))
    want = _bwd(ps, ts, da, db, _slice(torch.zeros(shape), "dense"))
    kp.check_bits("grad", pv.grad.cpu().contiguous(), want)
    # the cached coefficients are the ones the model passes
    ca, cb = ops.ssim_coeffs(pv.device, 9)
    assert ops.ssim_coeffs(pv.device, 9)[0] is ca
    assert torch.equal(ca.cpu(), a) and torch.equal(cb.cpu(), b)
    # defaults: a = 1, b = 0
    plain = ops.ssim_loss(pv.detach(), tv, SCALE)
    kp.check_bits("no coefficients", plain.cpu(), _fwd(ps, ts, None, None))


def test_criterion_on_nchw_input_is_the_op():
    from vae2 import ops
    from vae2.criterion import SSIMLoss
    shape = (2, 45, 77, 9)
    p, t, a, b = _case(shape, "near", True)[:4]
    pn = p.permute(0, 3, 1, 2).contiguous().to(kp.DEV).requires_grad_(True)
    tn = t.permute(0, 3, 1, 2).contiguous().to(kp.DEV)
    loss = SSIMLoss()(pn, tn)
    loss.backward()
    ps, ts, da, db = _slice(p, "dense"), _slice(t, "dense"), _dev(a), _dev(b)
    kp.check_bits("criterion loss", loss.detach().cpu(), _fwd(ps, ts, da, db, scale=1.0 / 2))
    want = _bwd(ps, ts, da, db, _slice(torch.zeros(shape), "dense"), gout=1.0, scale=1.0 / 2)
    kp.check_bits("criterion grad", pn.grad.permute(0, 2, 3, 1).cpu().contiguous(), want)


def test_op_rejects_small_frames_and_mismatched_coefficients():
    from vae2 import ops
    from vae2._lib import HipError
    x = torch.zeros((1, 8, 8, 3), device=kp.DEV)
    with pytest.raises(HipError, match="vae2_ssim_loss_fwd"):
        ops.ssim_loss(x, x, 1.0)
    y = torch.zeros((1, 11, 11, 3), device=kp.DEV)
    with pytest.raises(ValueError, match="together"):
        ops.ssim_loss(y, y, 1.0, a=torch.ones(3, device=kp.DEV))
    with pytest.raises(ValueError, match="channels"):
        ops.ssim_loss(y, y, 1.0, a=torch.ones(2, device=kp.DEV), b=torch.ones(2, device=kp.DEV))

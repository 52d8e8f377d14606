"""Global gradient-norm clipping (ABI 14): vae2_grad_sumsq / vae2_clip_coeffs / the *_clip
steps / vae2_scale_dev, and max_grad_norm of vae2.optim.FusedSGD / FusedAdam.

The norm: the kernel squares and sums in fp64, so its summation error (< n * 2^-53 relative)
is far below half an fp32 ulp and only the final rounding to fp32 can differ from
want = float32(sqrt(sum g^2)) computed in fp64 on the CPU: |got - want| <= 2^-23 * want.

The coefficient is compared bit for bit with torch's fp32 expression evaluated by numpy on
the read-back norm; the fused steps are compared bit for bit with the existing steps run on a
gradient pre-scaled by a torch fp32 multiply.

Against torch (clip_grad_norm_ + torch.optim on the CPU) the convention is that of
test_sgd_gpu.py: truth is the CPU in fp64 from the same fp32 inputs, the yardstick the CPU in
fp32, and with err(x) = max|x - x64| a result passes when

    err(gpu) <= 2 * err(cpu_fp32) + 2^-23 * max|x64|.

"The same fp32 inputs" includes Adam's hyper-parameters: the C ABI takes lr (through the
device state), beta1, beta2, eps and weight_decay as fp32, so torch is given those fp32
values (float32(0.999) = 0.99900001287..., not 0.999).  The existing Adam kernel forms
1 - beta in fp32 from the rounded beta, which is exact for that value; given the decimal
0.999 instead, torch's 1 - beta2 differs from the kernel's by 1.3e-5 relative and exp_avg_sq
with it (measured on the MI355X at n = 1023: err 2.2e-7 against a bound of 2.0e-8) -- a
property of how the unclipped step takes its betas, not of clipping."""
import functools
import math

import numpy as np
import pytest
import torch

from helpers import build, make_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
ULP = 2.0 ** -23
GUARD = 8  # sentinel elements around every device buffer: nothing outside is written

# the last size takes a second grid-stride pass of the 16-byte body plus a ragged tail
SIZES = [1, 3, 4, 5, 1023, 4 * 256 * 4096 + 7]
SGD_CONFIGS = {
    "plain": dict(),
    "wd": dict(weight_decay=1e-2),
    "mom": dict(momentum=0.9),
    "mom_damp": dict(momentum=0.9, dampening=0.1),
    "nesterov": dict(momentum=0.9, nesterov=True),
    "nesterov_wd": dict(momentum=0.9, weight_decay=1e-2, nesterov=True),
}


def _f32(x):
    """The value an fp32 argument of the C ABI takes."""
    return float(np.float32(x))


ADAM_CONFIGS = {"adam": dict(), "adam_wd": dict(weight_decay=_f32(1e-2))}
LR = 0.05
ADAM_LR, BETAS, EPS = _f32(1e-3), (_f32(0.9), _f32(0.999)), _f32(1e-8)  # torch's defaults
STEP_SCALES = [0.5, 2.0, 0.75, 4.0, 0.25]  # clipping at max_norm = sqrt(n) is active in 2 and 4


def _abi():
    from vae2 import ops
    from vae2._lib import call, load
    return call, load(), ops.ptr, ops.stream_ptr()


def _dev_buf(src, offset=0, dtype=torch.float32):
    """A device copy of src `offset` elements into an allocation with sentinels around it."""
    n = src.numel()
    raw = torch.full((GUARD + offset + n + GUARD,), 777.0, device=DEV, dtype=dtype)
    view = raw[GUARD + offset:GUARD + offset + n]
    view.copy_(src)
    return raw, view


def _guards_ok(raw, view):
    n = view.numel()
    lo = (view.data_ptr() - raw.data_ptr()) // raw.element_size()
    return bool((raw[:lo] == 777.0).all()) and bool((raw[lo + n:] == 777.0).all())


def _want_norm(*gs):
    """(float32(sqrt(sum g^2)), the fp64 value) from fp32 inputs, in fp64 on the CPU."""
    tot = sum(float((g.double() ** 2).sum()) for g in gs)
    return np.float32(math.sqrt(tot)), math.sqrt(tot)


def _coef_numpy(t, max_norm):
    """torch's clip coefficient in fp32 from the fp32 norm t."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(t) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else c


def _norm_pass(views, max_norm, fill=float("nan")):
    """vae2_grad_sumsq of every view end to end into one workspace, then vae2_clip_coeffs.
    Returns (clip raw, clip view, ws raw, ws view); the workspace starts filled with `fill`."""
    call, lib, ptr, s = _abi()
    sizes = [int(lib.vae2_grad_norm_ws_size(v.numel())) for v in views]
    wraw, ws = _dev_buf(torch.full((sum(sizes),), fill, dtype=torch.float64), dtype=torch.float64)
    craw, clip = _dev_buf(torch.full((4,), -5.0))
    off = 0
    for v, k in zip(views, sizes):
        call("vae2_grad_sumsq", ptr(v), v.numel(), ptr(ws[off:]), s)
        off += k
    call("vae2_clip_coeffs", ptr(ws), sum(sizes), max_norm, ptr(clip), s)
    torch.cuda.synchronize()
    return craw, clip, wraw, ws


def _same_bits(a, b):
    return torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                       b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))


def _check_norm(host_gs, offset=0, max_norm=INF):
    """The norm of the concatenation of host_gs: one ulp, sentinels, g untouched, reproducible
    partials, every workspace slot written."""
    bufs = [_dev_buf(g, offset) for g in host_gs]
    views = [v for _, v in bufs]
    craw, clip, wraw, ws = _norm_pass(views, max_norm)
    want, _ = _want_norm(*host_gs)
    got = np.float32(clip[0].item())
    print(f"n={[g.numel() for g in host_gs]} offset={offset}: norm got={got!r} want={want!r} "
          f"diff={abs(float(got) - float(want)):.3e} ulp={ULP * float(want):.3e}")
    assert abs(float(got) - float(want)) <= ULP * float(want)
    assert not torch.isnan(ws).any()  # every slot of a NaN-filled workspace was written
    assert _guards_ok(craw, clip) and _guards_ok(wraw, ws)
    for (raw, v), g in zip(bufs, host_gs):
        assert _guards_ok(raw, v)
        assert torch.equal(v.cpu(), g)  # g is read only
    # a second launch, into a differently filled workspace: the same bits
    _, clip2, _, ws2 = _norm_pass(views, max_norm, fill=3.0)
    assert _same_bits(ws, ws2) and _same_bits(clip[:2], clip2[:2])
    return clip


# ---------------------------------------------------------------------- norm ----

@functools.lru_cache(maxsize=None)
def _randn(n, seed=0):
    return torch.randn(n, generator=torch.Generator().manual_seed(2000 + seed + n % 997))


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("n", SIZES)
def test_norm_matches_fp64(n, scale):
    _check_norm([_randn(n) * scale])


@pytest.mark.parametrize("n", [5, 1023])
def test_norm_of_values_whose_squares_overflow_fp32(n):
    clip = _check_norm([torch.full((n,), 1e20)])
    assert math.isfinite(clip[0].item())


def test_norm_two_buffers_of_unequal_size_in_one_workspace():
    _check_norm([_randn(1023), _randn(4 * 1024 + 3, seed=1) * 3.0])


@pytest.mark.parametrize("n", [1, 5, 1023])
def test_norm_pointer_offset_by_one_float(n):
    g = _randn(n)
    a = _check_norm([g], offset=1)  # the scalar path
    b = _check_norm([g], offset=0)
    assert abs(a[0].item() - b[0].item()) <= ULP * b[0].item()


# --------------------------------------------------------------- coefficient ----

def test_coefficient_below_at_and_above_max_norm():
    g = _randn(1023)
    _, view = _dev_buf(g)
    t = np.float32(_norm_pass([view], INF)[1][0].item())
    cases = [float(t) * 0.5, float(np.float32(t * np.float32(0.999))), float(t),
             float(np.nextafter(t, np.float32(INF))), float(t) * 2.0, 1e-30, 3e38]
    for max_norm in cases:
        max_norm = float(np.float32(max_norm))
        _, clip, _, _ = _norm_pass([view], max_norm)
        got_t, got_c = np.float32(clip[0].item()), np.float32(clip[1].item())
        want_c = _coef_numpy(got_t, max_norm)
        print(f"max_norm={max_norm!r} t={got_t!r} coef got={got_c!r} want={want_c!r}")
        assert got_t == t
        assert got_c.tobytes() == want_c.tobytes()
        assert (got_c < 1) == (max_norm < float(t))
    _, clip, _, _ = _norm_pass([view], INF)
    assert clip[1].item() == 1.0


def test_coefficient_of_zero_gradient_is_one():
    _, view = _dev_buf(torch.zeros(1023))
    _, clip, _, _ = _norm_pass([view], 0.5)
    assert clip[0].item() == 0.0 and clip[1].item() == 1.0


@pytest.mark.parametrize("bad,want_t,want_c", [(float("nan"), "nan", "nan"), (INF, "inf", 0.0),
                                               (-INF, "inf", 0.0)])
def test_nonfinite_gradient(bad, want_t, want_c):
    for n, at in ((1023, 517), (1023, 1022), (4 * 256 * 4096 + 7, 4 * 256 * 4096 + 6)):
        g = _randn(n).clone()
        g[at] = bad
        _, view = _dev_buf(g)
        _, clip, _, _ = _norm_pass([view], 2.0)
        t, c = clip[0].item(), clip[1].item()
        if want_t == "nan":
            assert math.isnan(t) and math.isnan(c)
        else:
            assert t == INF and c == want_c


# ------------------------------------------- fused step == pre-scaled step ----

def _prescaled(g, clip, offset):
    """g * clip[1] by a torch fp32 multiply on the device, at g's alignment."""
    return _dev_buf(g * clip[1], offset)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("cfg", list(SGD_CONFIGS))
def test_sgd_clip_step_equals_step_on_prescaled_gradient(cfg, offset):
    call, lib, ptr, s = _abi()
    n, kw = 1023, SGD_CONFIGS[cfg]
    mom, damp = kw.get("momentum", 0.0), kw.get("dampening", 0.0)
    wd, nes = kw.get("weight_decay", 0.0), int(kw.get("nesterov", False))
    p0 = _randn(n, seed=5)
    (pa_raw, pa), (pb_raw, pb) = _dev_buf(p0, offset), _dev_buf(p0, offset)
    nanbuf = torch.full((n,), float("nan"))
    (ba_raw, ba), (bb_raw, bb) = (_dev_buf(nanbuf, offset), _dev_buf(nanbuf, offset)) if mom \
        else ((None, None), (None, None))
    state = torch.tensor([0.0, LR], dtype=torch.float64, device=DEV)
    coeffs = torch.zeros(4, device=DEV)
    for k, scale in enumerate(STEP_SCALES[:3]):
        gh = _randn(n, seed=10 + k) * scale
        graw, g = _dev_buf(gh, offset)
        craw, clip, _, _ = _norm_pass([g], 0.4 * math.sqrt(n))
        assert 0 < clip[1].item() < 1  # clipping is active in every step
        _, gs = _prescaled(g, clip, offset)
        call("vae2_sgd_coeffs", ptr(state), mom, damp, nes, ptr(coeffs), s)
        call("vae2_sgd_step_dev_clip", ptr(pa), ptr(g), ptr(ba), n, ptr(coeffs), ptr(clip), mom,
             wd, nes, s)
        call("vae2_sgd_step_dev", ptr(pb), ptr(gs), ptr(bb), n, ptr(coeffs), mom, wd, nes, s)
        torch.cuda.synchronize()
        assert torch.equal(pa, pb), f"step {k}: {int((pa != pb).sum())} parameters differ"
        assert not torch.equal(pa.cpu(), p0)
        if mom:
            assert torch.equal(ba, bb), f"step {k}: momentum buffers differ"
            assert _guards_ok(ba_raw, ba)
        assert torch.equal(g.cpu(), gh)  # the gradient buffer is not modified
        assert _guards_ok(graw, g) and _guards_ok(pa_raw, pa) and _guards_ok(craw, clip)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("cfg", list(ADAM_CONFIGS))
def test_adam_clip_step_equals_step_on_prescaled_gradient(cfg, offset):
    call, lib, ptr, s = _abi()
    n, wd = 1023, ADAM_CONFIGS[cfg].get("weight_decay", 0.0)
    p0 = _randn(n, seed=5)
    zeros = torch.zeros(n)
    (pa_raw, pa), (_, pb) = _dev_buf(p0, offset), _dev_buf(p0, offset)
    (ma_raw, ma), (_, mb) = _dev_buf(zeros, offset), _dev_buf(zeros, offset)
    (va_raw, va), (_, vb) = _dev_buf(zeros, offset), _dev_buf(zeros, offset)
    state = torch.tensor([0.0, ADAM_LR], dtype=torch.float64, device=DEV)
    coeffs = torch.zeros(2, device=DEV)
    for k, scale in enumerate(STEP_SCALES[:3]):
        gh = _randn(n, seed=10 + k) * scale
        graw, g = _dev_buf(gh, offset)
        craw, clip, _, _ = _norm_pass([g], 0.4 * math.sqrt(n))
        assert 0 < clip[1].item() < 1
        _, gs = _prescaled(g, clip, offset)
        call("vae2_adam_coeffs", ptr(state), BETAS[0], BETAS[1], ptr(coeffs), s)
        call("vae2_adam_step_dev_clip", ptr(pa), ptr(g), ptr(ma), ptr(va), n, ptr(coeffs),
             ptr(clip), BETAS[0], BETAS[1], EPS, wd, s)
        call("vae2_adam_step_dev", ptr(pb), ptr(gs), ptr(mb), ptr(vb), n, ptr(coeffs), BETAS[0],
             BETAS[1], EPS, wd, s)
        torch.cuda.synchronize()
        assert torch.equal(pa, pb), f"step {k}: {int((pa != pb).sum())} parameters differ"
        assert torch.equal(ma, mb) and torch.equal(va, vb), f"step {k}: moments differ"
        assert not torch.equal(pa.cpu(), p0)
        assert torch.equal(g.cpu(), gh)
        assert _guards_ok(graw, g) and _guards_ok(pa_raw, pa) and _guards_ok(ma_raw, ma)
        assert _guards_ok(va_raw, va) and _guards_ok(craw, clip)


def test_scale_dev_scales_in_place_on_both_paths():
    call, lib, ptr, s = _abi()
    for n, offset in ((1, 0), (5, 0), (1023, 0), (1023, 1), (4 * 256 * 4096 + 7, 0)):
        gh = _randn(n) * 3.0
        raw, g = _dev_buf(gh, offset)
        _, clip, _, _ = _norm_pass([g], 0.4 * math.sqrt(n))
        want = g * clip[1]
        call("vae2_scale_dev", ptr(g), n, ptr(clip), s)
        torch.cuda.synchronize()
        assert torch.equal(g, want) and not torch.equal(g.cpu(), gh)
        assert _guards_ok(raw, g)


# ------------------------------------------------------------ against torch ----

@functools.lru_cache(maxsize=None)
def _inputs(n):
    g = torch.Generator().manual_seed(3000 + n % 997)
    return torch.randn(n, generator=g), tuple(torch.randn(n, generator=g) * sc
                                              for sc in STEP_SCALES)


def _torch_clipped(p0, grads, dtype, max_norm, adam, **kw):
    """Parameters and optimizer state after clip_grad_norm_ + torch.optim steps on the CPU."""
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.Adam([p], lr=ADAM_LR, betas=BETAS, eps=EPS, **kw) if adam \
        else torch.optim.SGD([p], lr=LR, **kw)
    for g in grads:
        p.grad = g.to(dtype).clone()
        torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
    st = opt.state[p]
    state = (st["exp_avg"], st["exp_avg_sq"]) if adam else (st.get("momentum_buffer"),)
    return (p.detach(),) + tuple(state)


@functools.lru_cache(maxsize=None)
def _reference(n, cfg):
    p0, grads = _inputs(n)
    adam = cfg in ADAM_CONFIGS
    kw = ADAM_CONFIGS[cfg] if adam else SGD_CONFIGS[cfg]
    return tuple(_torch_clipped(p0, grads, dt, math.sqrt(n), adam, **kw)
                 for dt in (torch.float64, torch.float32))


def _check(what, got, x32, x64):
    e_gpu = float((got.double().cpu() - x64).abs().max())
    e_cpu = float((x32.double() - x64).abs().max())
    bound = 2.0 * e_cpu + ULP * float(x64.abs().max())
    print(f"{what}: err(gpu)={e_gpu:.3e} err(cpu_fp32)={e_cpu:.3e} bound={bound:.3e}")
    assert e_gpu <= bound, (what, e_gpu, e_cpu, bound)


def _run_clipped(n, cfg):
    """Five clipped steps through the C ABI; returns (p, state..., coefficients)."""
    call, lib, ptr, s = _abi()
    adam = cfg in ADAM_CONFIGS
    kw = ADAM_CONFIGS[cfg] if adam else SGD_CONFIGS[cfg]
    mom, damp = kw.get("momentum", 0.0), kw.get("dampening", 0.0)
    wd, nes = kw.get("weight_decay", 0.0), int(kw.get("nesterov", False))
    p0, grads = _inputs(n)
    p = p0.to(DEV)
    g = torch.empty(n, device=DEV)
    a = torch.zeros(n, device=DEV) if adam else \
        (torch.full((n,), float("nan"), device=DEV) if mom else None)
    b = torch.zeros(n, device=DEV) if adam else None
    state = torch.tensor([0.0, ADAM_LR if adam else LR], dtype=torch.float64, device=DEV)
    coeffs = torch.zeros(4, device=DEV)
    ws = torch.empty(int(lib.vae2_grad_norm_ws_size(n)), dtype=torch.float64, device=DEV)
    clip = torch.zeros(4, device=DEV)
    coefs = []
    for gk in grads:
        g.copy_(gk)
        call("vae2_grad_sumsq", ptr(g), n, ptr(ws), s)
        call("vae2_clip_coeffs", ptr(ws), ws.numel(), math.sqrt(n), ptr(clip), s)
        if adam:
            call("vae2_adam_coeffs", ptr(state), BETAS[0], BETAS[1], ptr(coeffs), s)
            call("vae2_adam_step_dev_clip", ptr(p), ptr(g), ptr(a), ptr(b), n, ptr(coeffs),
                 ptr(clip), BETAS[0], BETAS[1], EPS, wd, s)
        else:
            call("vae2_sgd_coeffs", ptr(state), mom, damp, nes, ptr(coeffs), s)
            call("vae2_sgd_step_dev_clip", ptr(p), ptr(g), ptr(a), n, ptr(coeffs), ptr(clip),
                 mom, wd, nes, s)
        coefs.append(clip[1].item())
    torch.cuda.synchronize()
    out = (p, a, b) if adam else (p, a)
    return out, coefs


@pytest.mark.parametrize("cfg", list(SGD_CONFIGS) + list(ADAM_CONFIGS))
@pytest.mark.parametrize("n", SIZES)
def test_clipped_steps_match_torch(n, cfg):
    ref64, ref32 = _reference(n, cfg)
    got, coefs = _run_clipped(n, cfg)
    print(f"n={n} {cfg}: coefficients {coefs}")
    if n >= 1023:  # the norm of randn(n) * s is close to s * sqrt(n)
        assert [c < 1 for c in coefs] == [False, True, False, True, False]
    names = ("p", "exp_avg", "exp_avg_sq") if cfg in ADAM_CONFIGS else ("p", "buf")
    for name, x, x32, x64 in zip(names, got, ref32, ref64):
        assert (x is None) == (x64 is None)
        if x is not None:
            _check(f"{name} n={n} {cfg}", x, x32, x64)


# ----------------------------------------------- FusedSGD / FusedAdam, tiny ----

def _tiny(kind, seed=0, grad_seed=3, **kw):
    from vae2.optim import FusedAdam, FusedSGD
    ed, ez = build(make_cfg("tiny"), seed=seed)
    ed.to(DEV), ez.to(DEV)
    opt = FusedSGD([ez, ed], **kw) if kind == "sgd" else FusedAdam([ez, ed], **kw)
    return opt, _fill_grads(opt, grad_seed)


def _fill_grads(opt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    for f in opt.flats:
        f.grad.copy_(torch.randn(f.numel, generator=g) * scale)
    return [f.grad.cpu().clone() for f in opt.flats]


KINDS = {"sgd": dict(lr=LR, momentum=0.9, weight_decay=1e-4), "adam": dict(lr=ADAM_LR)}


@pytest.mark.parametrize("kind", list(KINDS))
def test_grad_norm_is_the_norm_of_all_flat_gradients(kind):
    opt, grads = _tiny(kind, max_grad_norm=INF, **KINDS[kind])
    assert len(opt.flats) == 2 and opt.flats[0].numel != opt.flats[1].numel
    opt.step()
    t = opt.grad_norm()
    assert t.is_cuda and t.dim() == 0
    want, _ = _want_norm(*grads)
    print(f"{kind}: grad_norm {t.item()!r} want {want!r}")
    assert abs(t.item() - float(want)) <= ULP * float(want)
    grads = _fill_grads(opt, 4, scale=7.0)  # the value is that of the last step()
    opt.step()
    want, _ = _want_norm(*grads)
    assert abs(opt.grad_norm().item() - float(want)) <= ULP * float(want)
    for f, g in zip(opt.flats, grads):
        assert torch.equal(f.grad.cpu(), g)  # step() leaves the flat gradients as they were


@pytest.mark.parametrize("kind", list(KINDS))
def test_infinite_threshold_equals_no_clipping(kind):
    a, _ = _tiny(kind, max_grad_norm=None, **KINDS[kind])
    b, _ = _tiny(kind, max_grad_norm=INF, **KINDS[kind])
    for k in range(3):
        _fill_grads(a, 20 + k), _fill_grads(b, 20 + k)
        a.step(), b.step()
    torch.cuda.synchronize()
    for fa, fb in zip(a.flats, b.flats):
        assert torch.equal(fa.data, fb.data)
    assert a.step_count == b.step_count == 3
    # state_dict() has exactly the keys it has without clipping
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb) and sorted(sa["state"]) == sorted(sb["state"])
    assert sa["param_groups"][0].keys() == sb["param_groups"][0].keys()
    for i in sa["state"]:
        assert sa["state"][i].keys() == sb["state"][i].keys()
        for key in sa["state"][i]:
            assert torch.equal(sa["state"][i][key], sb["state"][i][key])


def test_finite_threshold_scales_the_first_plain_sgd_update():
    """Plain SGD, threshold below the norm t: the update is -lr * g * c with
    ||g * c|| = max_norm * t / (t + 1e-6) up to a few fp32 roundings (c and each product:
    2^-20 covers them), and every stored parameter adds at most half an ulp of its own, so
    | ||dp|| - lr * max_norm | <= lr * max_norm * (2^-20 + 1e-6 / t) + 2^-23 * ||p||."""
    lr, max_norm = 0.1, 1.0
    opt, grads = _tiny("sgd", lr=lr, max_grad_norm=max_norm)
    before = torch.cat([f.data for f in opt.flats]).double().cpu()
    opt.step()
    after = torch.cat([f.data for f in opt.flats]).double().cpu()
    t = opt.grad_norm().item()
    assert t > max_norm
    dp = float((after - before).norm())
    tol = lr * max_norm * (2.0 ** -20 + 1e-6 / t) + ULP * float(before.norm())
    print(f"||dp||={dp!r} lr*max_norm={lr * max_norm} tol={tol:.3e} t={t}")
    assert abs(dp - lr * max_norm) <= tol
    # and it points along the gradient
    g = torch.cat(grads).double()
    cos = float(((before - after) * g).sum() / ((after - before).norm() * g.norm()))
    assert cos > 1 - 1e-6


@pytest.mark.parametrize("max_norm", [5.0, 1e6])
def test_clip_grad_norm_function(max_norm):
    from vae2.optim import clip_grad_norm_
    opt, grads = _tiny("sgd", lr=LR, max_grad_norm=max_norm)
    opt.step()
    t_step = opt.grad_norm().item()
    g_dev = [f.grad.clone() for f in opt.flats]
    t = clip_grad_norm_(opt, max_norm)
    assert t.is_cuda and t.dim() == 0 and t.item() == t_step  # the same norm
    coef = _coef_numpy(np.float32(t.item()), max_norm)
    assert (coef < 1) == (max_norm < t_step)
    for f, g in zip(opt.flats, g_dev):
        assert torch.equal(f.grad, g * float(coef))
    # a list of FlatParams is accepted as well
    for f, g in zip(opt.flats, g_dev):
        f.grad.copy_(g)
    t2 = clip_grad_norm_(list(opt.flats), max_norm)
    assert t2.item() == t_step
    for f, g in zip(opt.flats, g_dev):
        assert torch.equal(f.grad, g * float(coef))


# ------------------------------------------------------------- graph replay ----

@pytest.mark.parametrize("kind", list(KINDS))
def test_norm_and_coefficient_are_recomputed_under_replay(kind):
    """A graph captured before the first step over "refill the flat gradients from a static
    tensor, step": every replay's grad_norm() follows the rescaled static tensor, and the
    parameters equal an eager twin's bit for bit."""
    from vae2.graph import StepGraph
    a, grads = _tiny(kind, max_grad_norm=1.0, **KINDS[kind])
    _, base = _want_norm(*grads)
    kw = dict(max_grad_norm=1.5 * base, **KINDS[kind])
    a, _ = _tiny(kind, **kw)
    b, _ = _tiny(kind, **kw)
    static = [g.to(DEV) for g in grads]

    def step():
        for f, src in zip(b.flats, static):
            f.grad.copy_(src)
        b.step()

    graph = StepGraph(step, warmup=0)
    assert b.step_count == 0  # the capture itself ran nothing
    total = 1.0
    for scale, clipped in ((1.0, False), (2.0, True), (0.125, False)):
        total *= scale
        for src in static:
            src.mul_(scale)
        graph.replay()
        for f, src in zip(a.flats, static):
            f.grad.copy_(src)
        a.step()
        torch.cuda.synchronize()
        want, _ = _want_norm(*[s.cpu() for s in static])
        got = b.grad_norm().item()
        print(f"{kind} replay at scale {total}: grad_norm {got!r} want {want!r}")
        assert abs(got - float(want)) <= ULP * float(want)
        assert (b._norm.clip[1].item() < 1) == clipped
        assert got == a.grad_norm().item()
        for fa, fb in zip(a.flats, b.flats):
            assert torch.equal(fa.data, fb.data)
    assert a.step_count == b.step_count == 3

"""Kernel-level parity of the training objective: vae2_l1_fwd/_bwd, vae2_lsgan_fwd/_bwd,
vae2_reparam_kl_fwd/_bwd, vae2_weighted_sum and vae2_nonfinite_check, called through the C
ABI on sentinel-padded device buffers.  Truth is computed on the CPU in fp64 from the same
fp32 inputs (and the fp32 values the scalar arguments take in the ABI).

Tolerance rules (kparity.py), none tuned from the kernels' output:

* Bit-exact ops are compared bit for bit with torch fp32 evaluating the same expression:
  pure moves (prior=1: z == eps) and single-rounding products with beta 0 (l1_bwd:
  sign * (gout * scale), each factor pair rounded once).
* Sums (L1, LSGAN, KL):  |got - want64| <= K * 2^-24 * sum|terms_i| + 2^-24 * |want64|, K the
  length of the kernel's longest fp32 add chain: a thread adds its `it` grid-stride terms,
  wave_sum adds 6 times, thread 0 adds the 4 wave totals with 3 adds: K = it + 6 + 3.  The
  blocks' partials are then summed in fp64 (error ~2^-53, nothing), cast to fp32 (the
  2^-24 * |want64| term) and multiplied by scale, a power of two in every case here (exact).
  With nb = min(1024, ceil(n / 1024)) blocks of 256 threads, it = ceil(n / (256 * nb)); each
  case's table entry carries it and K, and the test checks nb against vae2_reduce_ws_size.
  For KL, terms_i = 0.5 * (mu^2 + e^lv + |lv| + 1) (every intermediate of the kernel's
  expression is below twice that), and two ulp of each expf are added: 2^-23 * e^lv * 0.5 * 2.
  K counts the adds of the chain.  An L1 term's own rounding (p - t) takes the place of the
  thread's first add, which is onto 0.f and exact; the roundings inside an LSGAN term (x - 1)
  and a KL term (its four operations) are not counted, so for those two the bound is the
  chain's first-order worst case, not the expression's.  It is kept as it is: the first run
  on the MI355X left a factor of 7 or more in every case (the lines each test prints).
* Other element-wise fp32 results (lsgan_bwd, z, reparam_kl_bwd, weighted_sum, anything with
  beta != 0, where the compiler may contract to an fma, and where expf differs from the
  CPU's by an ulp):  err(gpu) <= 2 * err(cpu_fp32) + 2^-23 * max|x64|, err(x) = max|x - x64|.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from kparity import DEV, Slice, abi, check_bits, check_ew, check_sum, flat, same_bits, scalar

pytestmark = pytest.mark.gpu
INF = float("inf")
NAN = float("nan")


def _f32(x):
    """The value an fp32 argument of the C ABI takes."""
    return float(np.float32(x))


def _loss_it(n):
    """(blocks, per-thread iterations) of the loss kernels' first stage at n elements."""
    nb = min(1024, max(1, -(-n // 1024)))
    return nb, -(-n // (256 * nb))


# name -> (shape, (ps, c0) of the first operand, of the second, of the gradient, it, K)
#   K = it + 6 (wave_sum) + 3 (the 4 wave totals);  it = ceil(n / (256 * nb))
FWD_CASES = {
    # (a) flat (1, 1, n, 1): block and wave edges
    "flat1": ((1, 1, 1, 1), (1, 0), (1, 0), (1, 0), 1, 10),       # nb 1, it 1: K = 1 + 9
    "flat255": ((1, 1, 255, 1), (1, 0), (1, 0), (1, 0), 1, 10),   # nb 1, it 1: K = 1 + 9
    "flat256": ((1, 1, 256, 1), (1, 0), (1, 0), (1, 0), 1, 10),   # nb 1, it 1: K = 1 + 9
    "flat257": ((1, 1, 257, 1), (1, 0), (1, 0), (1, 0), 2, 11),   # nb 1, thread 0 twice: 2 + 9
    "flat1025": ((1, 1, 1025, 1), (1, 0), (1, 0), (1, 0), 3, 12),  # nb 2, 512 threads: 3 + 9
    # (b) channel slices of wider buffers, starting at a non-zero channel: 210 elements
    "nhwc": ((2, 5, 7, 3), (27, 6), (9, 3), (12, 5), 1, 10),      # nb 1, it 1: K = 1 + 9
    # (c) 1,054,800 elements: ceil(n / 1024) = 1031 > 1024 blocks, so 262,144 threads loop
    #     ceil(4.02) = 5 times: K = 5 + 9
    "capped": ((2, 200, 293, 9), (9, 0), (10, 1), (12, 2), 5, 14),
}
# (d) backward only: ew_blocks caps at 65,536 blocks, 257 elements take a second pass
BIG_N = 65536 * 256 + 257
SCALE = 0.25  # 1 / B at B = 4: a power of two, so the final product is exact
GOUT = 1.7


@functools.lru_cache(maxsize=None)
def _pt(name):
    """(p, t) of a case, fp32 on the host; some elements equal, one pair +0 against -0."""
    shape = FWD_CASES[name][0] if name != "big" else (1, 1, BIG_N, 1)
    g = torch.Generator().manual_seed(4000 + sum(shape))
    p = torch.randn(shape, generator=g)
    t = torch.randn(shape, generator=g)
    n = p.numel()
    pf, tf = p.view(-1), t.view(-1)
    if n > 8:
        eq = torch.arange(3, n, 7)[:64]
        tf[eq] = pf[eq]  # p == t exactly: gradient 0
        pf[5], tf[5] = 0.0, -0.0
        pf[6], tf[6] = -0.0, 0.0  # (the last element stays random: a dropped pass must show)
    return p, t


def _l1_truth(p, t):
    d = (p.double() - t.double()).abs()
    return float(d.sum()) * SCALE, float(d.sum()) * SCALE


def _run_l1_fwd(p, t, pl, tl):
    call, lib, ptr, s = abi()
    n = p.numel()
    P, T = Slice(p, *pl), Slice(t, *tl)
    nb = int(lib.vae2_reduce_ws_size(n))
    ws = flat(torch.full((nb,), NAN))
    out = scalar()
    call("vae2_l1_fwd", P.ptr, P.ref, T.ptr, T.ref, SCALE, ws.ptr, out.ptr, s)
    torch.cuda.synchronize()
    assert P.intact() and T.intact() and ws.intact() and out.intact()
    assert same_bits(P.read(), p) and same_bits(T.read(), t)  # inputs are read only
    return out.read().item(), ws.read().view(-1), nb


@pytest.mark.parametrize("name", list(FWD_CASES))
def test_l1_fwd(name):
    shape, pl, tl, _, it, k = FWD_CASES[name]
    p, t = _pt(name)
    got, ws, nb = _run_l1_fwd(p, t, pl, tl)
    assert (nb, it) == _loss_it(p.numel()) and k == it + 6 + 3
    assert not torch.isnan(ws).any()  # every slot of the NaN-filled workspace was written
    want, terms = _l1_truth(p, t)
    check_sum(f"l1_fwd {name}", got, want, terms, k)


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_l1_fwd_nonfinite_input_gives_nonfinite_loss(bad):
    for name in ("flat257", "nhwc", "capped"):
        p, t = _pt(name)
        for at in (0, p.numel() - 1):
            q = p.clone()
            q.view(-1)[at] = bad
            got, _, _ = _run_l1_fwd(q, t, *FWD_CASES[name][1:3])
            print(f"l1_fwd {name} p[{at}]={bad}: loss {got}")
            assert not math.isfinite(got)


def _l1_bwd_want(p, t, prev, beta):
    """fp32 expression of the kernel, and fp64 truth (beta 1)."""
    g = np.float32(GOUT) * np.float32(SCALE)  # gout[0] * scale, rounded once
    d = p - t
    sg = torch.where(d > 0, 1.0, torch.where(d < 0, -1.0, 0.0)).float()
    v = sg * float(g)  # exact: sg is 0 or +-1
    if beta == 0:
        return v, None
    return v + prev, sg.double() * float(g) + prev.double()


def _run_l1_bwd(name, beta):
    call, lib, ptr, s = abi()
    if name == "big":
        pl = tl = dl = (1, 0)
    else:
        _, pl, tl, dl, _, _ = FWD_CASES[name]
    p, t = _pt(name)
    prev = torch.randn(p.shape, generator=torch.Generator().manual_seed(17)) if beta else \
        torch.full(p.shape, NAN)  # beta 0 overwrites, whatever was there
    P, T, D = Slice(p, *pl), Slice(t, *tl), Slice(prev, *dl)
    gout = scalar(GOUT)
    call("vae2_l1_bwd", P.ptr, P.ref, T.ptr, T.ref, gout.ptr, SCALE, D.ptr, D.ref, float(beta), s)
    torch.cuda.synchronize()
    assert P.intact() and T.intact() and D.intact() and gout.intact()
    got = D.read()
    v32, v64 = _l1_bwd_want(p, t, prev, beta)
    if beta == 0:
        check_bits(f"l1_bwd {name} beta=0", got, v32)
        zero = (p == t)
        assert bool((got[zero] == 0).all()) and int(zero.sum()) >= min(2, p.numel() - 1)
    else:
        check_ew(f"l1_bwd {name} beta=1", got, v32, v64)


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("name", list(FWD_CASES) + ["big"])
def test_l1_bwd(name, beta):
    _run_l1_bwd(name, beta)


# ------------------------------------------------------------------- LSGAN ----

def _run_lsgan_fwd(x, xl, target):
    call, lib, ptr, s = abi()
    X = Slice(x, *xl)
    nb = int(lib.vae2_reduce_ws_size(x.numel()))
    ws, out = flat(torch.full((nb,), NAN)), scalar()
    call("vae2_lsgan_fwd", X.ptr, X.ref, float(target), SCALE, ws.ptr, out.ptr, s)
    torch.cuda.synchronize()
    assert X.intact() and ws.intact() and out.intact() and same_bits(X.read(), x)
    assert not torch.isnan(ws.read()).any()
    return out.read().item(), nb


@pytest.mark.parametrize("target", [0, 1])
@pytest.mark.parametrize("name", list(FWD_CASES))
def test_lsgan_fwd(name, target):
    shape, xl, _, _, it, k = FWD_CASES[name]
    x, _ = _pt(name)
    got, nb = _run_lsgan_fwd(x, xl, target)
    assert (nb, it) == _loss_it(x.numel()) and k == it + 6 + 3
    sq = (x.double() - target) ** 2  # every term is non-negative: sum|terms| = the sum
    want = float(sq.sum()) * SCALE
    check_sum(f"lsgan_fwd {name} target={target}", got, want, want, k)


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("target", [0, 1])
@pytest.mark.parametrize("name", list(FWD_CASES) + ["big"])
def test_lsgan_bwd(name, target, beta):
    call, lib, ptr, s = abi()
    xl, dl = ((1, 0), (1, 0)) if name == "big" else (FWD_CASES[name][1], FWD_CASES[name][3])
    x, _ = _pt(name)
    prev = torch.randn(x.shape, generator=torch.Generator().manual_seed(18)) if beta else \
        torch.full(x.shape, NAN)
    X, D, gout = Slice(x, *xl), Slice(prev, *dl), scalar(GOUT)
    call("vae2_lsgan_bwd", X.ptr, X.ref, float(target), gout.ptr, SCALE, D.ptr, D.ref,
         float(beta), s)
    torch.cuda.synchronize()
    assert X.intact() and D.intact() and gout.intact() and same_bits(X.read(), x)
    # the kernel's expression in fp32, and in fp64 from the same fp32 scalars
    g32 = np.float32(2.0) * np.float32(GOUT) * np.float32(SCALE)
    v32 = float(g32) * (x - float(target))
    v64 = 2.0 * _f32(GOUT) * SCALE * (x.double() - target)
    if beta:
        v32, v64 = v32 + prev, v64 + prev.double()
    check_ew(f"lsgan_bwd {name} target={target} beta={beta}", D.read(), v32, v64)


def test_lsgan_flat_on_a_noncontiguous_input_equals_dense():
    from vae2 import ops
    g = torch.Generator().manual_seed(19)
    base = torch.randn(2, 3, 5, 7, generator=g).to(DEV)
    outs = []
    for real in (True, False):
        a = base.permute(0, 2, 3, 1).requires_grad_(True)  # NCHW storage seen as NHWC
        b = base.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
        assert not a.is_contiguous() and b.is_contiguous()
        la, lb = ops.lsgan(a, real, 0.5, flat=True), ops.lsgan(b, real, 0.5, flat=True)
        (la * 1.5).backward()
        (lb * 1.5).backward()
        torch.cuda.synchronize()
        print(f"lsgan flat real={real}: strided {la.item()!r} dense {lb.item()!r}")
        assert same_bits(la.reshape(1), lb.reshape(1))
        assert a.grad.shape == b.grad.shape and torch.equal(a.grad, b.grad)
        want = float(((base.double().cpu() - float(real)) ** 2).sum()) * 0.5
        check_sum(f"lsgan flat real={real}", la.item(), want, want, 10)  # 210 elements: 1 + 9
        outs.append(la.item())
    assert outs[0] != outs[1]


# --------------------------------------------------------- reparam + KL ----

# name -> (z shape, (ps, c0) of muvar, of eps, of z, of dmuvar, of dz, scale, it, K)
KL_CASES = {
    # the workload's (B, 1, 1, zc): 80 elements, nb 1, it 1: K = 1 + 9
    "vec": ((8, 1, 1, 10), (20, 0), (10, 0), (12, 0), (20, 0), (10, 0), 0.125, 1, 10),
    # an HD-z map, muvar a slice at ps 12: 1024 elements, nb 1, 256 threads x 4: K = 4 + 9
    "map": ((2, 8, 16, 4), (12, 2), (4, 0), (8, 3), (12, 4), (6, 1), 0.5, 4, 13),
    # 1,050,624 elements: ceil(n / 1024) = 1026 > 1024 blocks, ceil(4.008) = 5 passes: 5 + 9
    "capped": ((1, 513, 512, 4), (8, 0), (4, 0), (4, 0), (8, 0), (4, 0), 1.0, 5, 14),
}


@functools.lru_cache(maxsize=None)
def _kl_inputs(name, edge):
    """(muvar, eps): randn, or with edge == True also lv = +-0, -30, +20 and mu = 0."""
    (n, h, w, zc) = KL_CASES[name][0]
    g = torch.Generator().manual_seed(5000 + n * h * w)
    mv = torch.randn(n, h, w, 2 * zc, generator=g)
    eps = torch.randn(n, h, w, zc, generator=g)
    if edge:
        m = mv.view(-1, 2 * zc)
        last = m.shape[0] - 1
        m[0, zc + 0], m[0, zc + 1], m[0, zc + 2], m[0, zc + 3] = 0.0, -0.0, -30.0, 20.0
        m[last, zc + 3], m[last, zc + 2], m[last, 0] = -30.0, 20.0, 0.0
        m[0, 0], m[0, 3] = 0.0, -0.0
    return mv, eps


def _kl_truth(mv, eps, scale):
    zc = eps.shape[3]
    mu, lv = mv[..., :zc].double(), mv[..., zc:].double()
    kl = scale * float((0.5 * (mu * mu + lv.exp() - lv - 1.0)).sum())
    terms = scale * float((0.5 * (mu * mu + lv.exp() + lv.abs() + 1.0)).sum())
    expf_slack = scale * float((0.5 * 2.0 * 2.0 ** -23 * lv.exp()).sum())  # 2 ulp of each expf
    z64 = mu + (0.5 * lv).exp() * eps.double()
    z32 = mv[..., :zc] + torch.exp(mv[..., zc:] * 0.5) * eps
    return kl, terms, expf_slack, z32, z64


def _run_kl_fwd(name, edge, prior, accumulate, preset):
    call, lib, ptr, s = abi()
    shape, ml, el, zl, _, _, scale, it, k = KL_CASES[name]
    mv, eps = _kl_inputs(name, edge)
    M, E = Slice(mv, *ml), Slice(eps, *el)
    Z = Slice(torch.full(shape, NAN), *zl)
    nb = int(lib.vae2_reduce_ws_size(eps.numel()))
    assert (nb, it) == _loss_it(eps.numel()) and k == it + 6 + 3
    ws, out = flat(torch.full((nb,), NAN)), scalar(preset)
    call("vae2_reparam_kl_fwd", M.ptr, M.ref, E.ptr, E.ref, Z.ptr, Z.ref, int(prior), scale,
         out.ptr, int(accumulate), ws.ptr, s)
    torch.cuda.synchronize()
    for b in (M, E, Z, ws, out):
        assert b.intact()
    assert same_bits(M.read(), mv) and same_bits(E.read(), eps)
    assert not torch.isnan(ws.read()).any()
    return Z.read(), out.read().view(1)


@pytest.mark.parametrize("edge", [False, True], ids=["randn", "edge"])
@pytest.mark.parametrize("name", list(KL_CASES))
def test_reparam_kl_fwd(name, edge):
    scale, k = KL_CASES[name][6], KL_CASES[name][8]
    mv, eps = _kl_inputs(name, edge)
    kl, terms, slack, z32, z64 = _kl_truth(mv, eps, scale)
    z, got = _run_kl_fwd(name, edge, prior=0, accumulate=0, preset=NAN)  # overwrites a NaN
    check_sum(f"kl {name} edge={edge}", got.item(), kl, terms, k, extra=slack)
    check_ew(f"z {name} edge={edge}", z, z32, z64)
    # prior sampling: z is eps bit for bit, the KL is the same bits
    zp, gotp = _run_kl_fwd(name, edge, prior=1, accumulate=0, preset=NAN)
    check_bits(f"z prior {name}", zp, eps)
    assert same_bits(gotp, got)
    # accumulate: one fp32 add onto the pre-set value
    pre = np.float32(-3.25)
    _, gota = _run_kl_fwd(name, edge, prior=0, accumulate=1, preset=float(pre))
    want = torch.tensor([float(pre + np.float32(got.item()))], dtype=torch.float32)
    print(f"kl accumulate {name}: got={gota.item()!r} want={want.item()!r}")
    assert same_bits(gota, want)


@pytest.mark.parametrize("with_gkl", [False, True], ids=["nogkl", "gkl"])
@pytest.mark.parametrize("with_dz", [False, True], ids=["nodz", "dz"])
@pytest.mark.parametrize("edge", [False, True], ids=["randn", "edge"])
@pytest.mark.parametrize("name", list(KL_CASES))
def test_reparam_kl_bwd(name, edge, with_dz, with_gkl):
    call, lib, ptr, s = abi()
    shape, ml, el, _, dml, dzl, scale, _, _ = KL_CASES[name]
    zc = shape[3]
    mv, eps = _kl_inputs(name, edge)
    dz = torch.randn(shape, generator=torch.Generator().manual_seed(21))
    M, E, DZ = Slice(mv, *ml), Slice(eps, *el), Slice(dz, *dzl)
    DM = Slice(torch.full(mv.shape, NAN), *dml)
    gkl = scalar(GOUT)
    call("vae2_reparam_kl_bwd", M.ptr, M.ref, E.ptr, E.ref, DZ.ptr if with_dz else None, DZ.ref,
         gkl.ptr if with_gkl else None, scale, DM.ptr, DM.ref, s)
    torch.cuda.synchronize()
    for b in (M, E, DZ, DM, gkl):
        assert b.intact()
    got = DM.read()
    # the kernel's expression in torch fp32 and in fp64
    gk32 = float(np.float32(GOUT) * np.float32(scale)) if with_gkl else 0.0
    g32 = dz if with_dz else torch.zeros(shape)
    mu, lv = mv[..., :zc], mv[..., zc:]
    dmu32 = g32 + gk32 * mu
    dlv32 = g32 * eps * 0.5 * torch.exp(lv * 0.5) + gk32 * 0.5 * (torch.exp(lv) - 1.0)
    gk64 = _f32(GOUT) * scale if with_gkl else 0.0
    g64, mu64, lv64 = g32.double(), mu.double(), lv.double()
    dmu64 = g64 + gk64 * mu64
    dlv64 = g64 * eps.double() * 0.5 * (0.5 * lv64).exp() + gk64 * 0.5 * (lv64.exp() - 1.0)
    tag = f"{name} edge={edge} dz={with_dz} gkl={with_gkl}"
    check_ew(f"dmu {tag}", got[..., :zc], dmu32, dmu64)
    check_ew(f"dlv {tag}", got[..., zc:], dlv32, dlv64)
    if not with_dz and not with_gkl:
        assert bool((got == 0).all())


# ------------------------------------------------------------ weighted sum ----

@pytest.mark.parametrize("n", [1, 2, 8])
def test_weighted_sum(n):
    call, lib, ptr, s = abi()
    g = torch.Generator().manual_seed(30 + n)
    vals = (torch.randn(n, generator=g) * 10).tolist()
    lams = torch.randn(n, generator=g).tolist()
    if n >= 2:
        lams[1] = 0.0
    if n >= 8:
        lams[3], lams[6] = -2.5, -0.0
    terms = [scalar(v) for v in vals]  # each term is its own device scalar
    ptrs = (ctypes.c_void_p * n)(*[t.ptr.value for t in terms])
    lamc = (ctypes.c_float * n)(*lams)
    out = scalar()
    call("vae2_weighted_sum", n, ptrs, lamc, out.ptr, s)
    torch.cuda.synchronize()
    assert out.intact() and all(t.intact() for t in terms)
    s32, s64 = np.float32(0.0), 0.0
    for v, lam in zip(vals, lams):  # the kernel's order
        s32 = np.float32(s32 + np.float32(lam) * np.float32(v))
        s64 += _f32(lam) * _f32(v)
    check_ew(f"weighted_sum n={n}", out.read().view(1), torch.tensor([float(s32)]),
             torch.tensor([s64], dtype=torch.float64))
    for t, v in zip(terms, vals):
        assert t.read().item() == _f32(v)


# --------------------------------------------------------- non-finite check ----

CHECK_BLOCK = 262144  # 1024 blocks of 256 threads: beyond it every thread loops
CHECK_SIZES = [1, 63, 64, 65, 256, 257, CHECK_BLOCK, CHECK_BLOCK + 1, 2 * CHECK_BLOCK + 3]
FLT_MAX = float(np.finfo(np.float32).max)
DENORM = float(np.float32(1e-45))


def _flag(value):
    raw = torch.full((17,), 777, dtype=torch.int32, device=DEV)
    raw[8] = value
    return raw, raw[8:9]


def _flag_guards_ok(raw):
    return bool((raw[:8] == 777).all()) and bool((raw[9:] == 777).all())


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", CHECK_SIZES)
def test_nonfinite_check(n, offset):
    call, lib, ptr, s = abi()
    x = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000))
    edge = [FLT_MAX, -FLT_MAX, DENORM, -DENORM, -0.0, 0.0]
    for i, v in enumerate(edge):  # all finite
        x[(i * 37) % n] = v
    X = flat(x, offset=offset)
    assert (X.ptr.value % 16 == 4) == bool(offset)
    view = X.view.view(-1)

    def run(start):
        raw, flag = _flag(start)
        call("vae2_nonfinite_check", X.ptr, n, ptr(flag), s)
        torch.cuda.synchronize()
        assert _flag_guards_ok(raw) and X.intact()
        return int(flag.item())

    assert run(0) == 0  # +-FLT_MAX, denormals and -0 are finite
    assert run(1) == 1  # a raised flag stays raised on clean data
    assert same_bits(X.read().view(-1), x)
    spots = sorted({0, n - 1} | ({CHECK_BLOCK} if n > CHECK_BLOCK else set()))
    for at in spots:
        keep = view[at].clone()
        for bad in (NAN, INF, -INF):
            view[at] = bad
            got = run(0)
            print(f"nonfinite n={n} offset={offset} x[{at}]={bad}: flag {got}")
            assert got == 1
        view[at] = keep
    assert run(0) == 0


def test_nonfinite_check_of_nothing_leaves_the_flag():
    call, lib, ptr, s = abi()
    X = flat(torch.full((4,), NAN))
    for start in (0, 1, 5):
        raw, flag = _flag(start)
        assert lib.vae2_nonfinite_check(X.ptr, 0, ptr(flag), s) == 0
        torch.cuda.synchronize()
        assert int(flag.item()) == start and _flag_guards_ok(raw)

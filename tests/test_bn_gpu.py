"""Kernel-level parity of the BatchNorm family (csrc/bn.hip): every vae2_bn_* entry point called
through the C ABI on sentinel-padded device buffers (kparity.Slice / kparity.Guarded), compared
element for element, channel for channel, with the fp64 reference of tests/bn_ref.py computed
from the same fp32 inputs.  vae2_kernel_log tells which kernel a case ran.

Tolerance rules, counted from the code, none tuned from the kernels' output
(U = 2^-24, E = 2^-53):

1. Partial sums (vae2_bn_stats, vae2_bn_relu_bwd_reduce, vae2_bn_multi_bwd_reduce and its
   rpartials): the kernel's fp32 partial rows are summed on the host in fp64 and
   |got - want64| <= K * U * sum|terms| + U * |want64| (kparity.check_sums), K the longest fp32
   add chain.  A block covers ppb = pass * max(1, ceil(P / (blocks * pass))) pixels, pass =
   4 * quad_rows(C), quad_rows(C) = 256 / ceil(C / 4) (1 above 256 quads), blocks = tune key 19.
   Quad kernels: a thread adds ceil(ppb / rows) terms and thread c the rows' sums, K =
   ceil(ppb / rows) + rows.  Scalar kernel: C <= 256: K = ceil(ppb / R) + R, R = 256 / C;
   C > 256: K = ppb.  The sum x^2 column takes K + 1 (the square), the sum g * xhat column K + 3
   ((x - mean), * invstd, * g).  ceil(P / ppb) is checked against vae2_bn_partial_rows.
2. Row reductions (vae2_bn_partials_reduce, the reduce half of vae2_bn_reduce_finalize*,
   vae2_bn_bwd_reduce_param_grads, vae2_bn_multi_reduce): double sums against the host's sum of
   the same partial rows (numpy longdouble): |got - want| <= rows * E * sum|partials|; with
   accumulate, + E * |want| for the add onto the previous value.
3. Finalize (double arithmetic rounded once to fp32), truth in numpy longdouble from the sums
   the kernel itself wrote or was given, fp32 values of momentum and eps:
   |got - want| <= U * (|want| + d) + d, d the first-order error of the double expression:
     m0 = s0 / n, q = s1 / n, var = q - m0^2:  dv = E * (q + 3 m0^2 + |var|)  (the quotient, the
       product, twice the error of m0, the subtraction; the clamp at 0 is 1-Lipschitz)
     mean = m0 + mean_shift:  dmean = E * (|m0| + |mean|)
     invstd = 1 / sqrt(var + eps):  dinv = invstd^3 / 2 * dv + 3 E * invstd  (add, sqrt, divide)
     scale = gamma * invstd:  dscale = |gamma| * dinv + E * |scale|
     shift = beta - mean * scale:  dshift = |scale| * dmean + |mean| * dscale +
       E * |mean * scale| + E * (|beta| + |mean * scale|)
     unbiased = var * n / (n - 1):  dunb = dv * n / (n - 1) + 2 E * unbiased
     running = (1 - mom) * old + mom * new:  mom * dnew + 3 E * (|(1 - mom) * old| + |mom * new|)
   Parameter gradients, dgamma += (float)s onto a previous value: U * (|s| + |new|).
   vae2_bn_eval_coeffs is fp32 arithmetic: kparity.check_ew.
4. Forward apply, per element, want64 = x * scale + shift (the product of two fp32 values is
   exact in fp64): a single fmaf, |got - want64| <= U * |want64|; with a residual the fmaf and
   the add round, U * (|x * scale + shift| + |want64|); with a residual BatchNorm its fmaf
   rounds too, + U * |rx * rscale + rshift|.  ReLU is 1-Lipschitz and is applied to the truth.
   NaN and Inf come out as in torch.  Mask bytes: the bits of the valid channels equal
   (y_gpu > 0) of the kernel's own output.
5. Backward apply, per element: |dx - want64| <= 8 * U * |gamma * invstd| * (|g| + |sum_g / n| +
   |xhat * sum_gx / n|).  Recount against bn_bwd_apply_q_kernel / bn_bwd_apply_body2:
   mg = fl(fl(sum) * fl(1 / n)) carries 3 roundings, mgx the same, xhat = fl(fl(x - mean) *
   invstd) 2, their product 1, the two subtractions 1 each, fl(gamma * invstd) 1 and the final
   product 1: to first order the coefficient is 4 on |g|, 7 on |sum_g / n| and 9 on the third
   term when nothing is contracted to an fma.  The bound asserted is the uniform 8 of the
   design: tighter than the recount on the third term, so no looser than the code allows
   anywhere it matters (|g| dominates unless g is masked).  rdx follows the same rule.  dres is
   bit-exact (masked dy); with dres_acc bit-exact against torch fp32 prev + g.  The ReLU mask is
   exact in every mode: y and the mask bytes are test inputs, and fmaf(x, scale, shift) > 0
   holds iff the exact x * scale + shift > 0, which fp64 decides (exact product, one rounding
   that keeps the sign); the inputs are asserted to have |x * scale + shift| = 0 or >= 2^-100.

Inputs: per-channel mean in [-4, 4] and std in [0.25, 2]; channel 1 is constant 3.0 (variance
exactly 0); gamma ~ N(1, 0.3), one negative; beta ~ N(0, 0.3); channel 0 has scale 0.5, shift
-1 and an x = 2 (x * scale + shift = +0), channel 2 scale 0.5, shift -0 and an x = -0 (-0);
stored y holds +0, -0 and the smallest positive normal; the element-wise kernels also get one
NaN and one +Inf.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import bn_ref
from kparity import SENT, U, Guarded, Slice, abi, check_bits, check_ew, check_sums, same_bits

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
E = 2.0 ** -53
EPS, MOM = float(np.float32(1e-5)), float(np.float32(0.01))
TINY = float(np.finfo(np.float32).tiny)
LD = np.longdouble


# ------------------------------------------------------------------ helpers ----

def r4(c):
    return (c + 3) // 4 * 4


def quad_rows(c):
    c4 = (c + 3) // 4
    return 256 // c4 if c4 <= 256 else 1


def quad_ok(c):
    return (c + 3) // 4 <= 256


def ppb_of(p, c, blocks):
    pas = 4 * quad_rows(c)
    return pas * max(1, -(-p // (blocks * pas)))


def chain_k(c, ppb, quad):
    """K of rule 1."""
    if quad:
        return -(-ppb // quad_rows(c)) + quad_rows(c)
    if c <= 256:
        return -(-ppb // (256 // c)) + 256 // c
    return ppb


# name -> (pixel stride, first channel) of a slice of C channels
LAYOUTS = {"dense": lambda c: (c, 0), "aligned": lambda c: (r4(c) + 8, 4),
           "c0=1": lambda c: (r4(c) + 8, 1), "odd": lambda c: (r4(c) + 9, 4)}


def S(x, kind, sent=SENT):
    ps, c0 = LAYOUTS[kind](x.shape[3])
    return Slice(x, ps, c0, sent=sent)


def v4(s):
    return s.ptr.value % 16 == 0 and s.ps % 4 == 0


@contextlib.contextmanager
def tune(lib, key, value):
    old = lib.vae2_conv2d_set_tune(key, value)
    assert old >= 0
    try:
        yield
    finally:
        lib.vae2_conv2d_set_tune(key, old)


@contextlib.contextmanager
def logged(lib, names):
    """Appends the kernels launched inside the block to `names` (template arguments without
    blanks)."""
    lib.vae2_kernel_log(1)
    try:
        yield
        buf = ctypes.create_string_buffer(8192)
        lib.vae2_kernel_log_read(buf, 8192)
        got = [k.replace(" ", "") for k in buf.value.decode().split(";") if k]
        print("KERNELS", " ".join(got))
        names += got
    finally:
        lib.vae2_kernel_log(0)


def ratio(rule, what, err, bound):
    """err <= bound element for element; prints the worst err / bound."""
    err, bound = torch.as_tensor(err).double().reshape(-1), torch.as_tensor(bound).double().reshape(-1)
    assert bool(torch.isfinite(err).all()) and bool(torch.isfinite(bound).all()), what
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                    torch.where(err > 0, torch.full_like(err, INF), torch.zeros_like(err)))
    top = float(r.max()) if r.numel() else 0.0
    print(f"RATIO rule{rule} {top:.4f} {what}: max err {float(err.max()) if r.numel() else 0.0:.3e}")
    assert bool((err <= bound).all()), (what, top)


def elementwise(rule, what, got, want64, bound):
    """Every element: non-finite values equal the truth's, finite ones within `bound`."""
    fin = torch.isfinite(want64)
    assert got.shape == want64.shape and torch.equal(torch.isfinite(got), fin), what
    assert torch.equal(got[~fin].double().nan_to_num(1e300, 2e300, -2e300),
                       want64[~fin].nan_to_num(1e300, 2e300, -2e300)), what
    exact = fin & ~torch.isfinite(bound)  # ReLU of -Inf: the bound is infinite, the value 0
    assert torch.equal(got[exact].double(), want64[exact]), what
    fin = fin & ~exact
    ratio(rule, what, (got.double() - want64)[fin].abs(), bound[fin])


def sums_rule(what, part, want, terms, k0, k1):
    """Rule 1 on partial rows [2][rows][C]: column sums in fp64 against want [2][C]."""
    assert bool(torch.isfinite(part).all()), what  # every slot written
    got = part.double().sum(1)
    for q, k in ((0, k0), (1, k1)):
        ratio(1, f"{what} [{q}] K={k}", (got[q] - want[q]).abs(),
              k * U * terms[q] + U * want[q].abs())
        check_sums(f"{what} [{q}]", got[q], want[q], terms[q], k)


def ld_sum(part):
    """Column sums of partial rows [2][rows][C] and of their absolute values, in longdouble."""
    a = part.numpy().astype(LD)
    return a.sum(1), np.abs(a).sum(1)


def f64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def rows_rule(what, got, part, prev=None):
    """Rule 2: double sums [2][C] against the longdouble sum of the partial rows."""
    want, mag = ld_sum(part)
    bound = part.shape[1] * E * mag
    if prev is not None:
        want = want + prev.numpy().astype(LD)
        bound = bound + E * np.abs(want)
    err = np.abs(got.numpy().astype(LD) - want)
    ratio(2, what, f64(err), f64(bound))


def finalize_rule(what, save, rm, rv, sums, n, gamma, beta, rm0, rv0, shift):
    """Rule 3 on save [4][C] and the running statistics, from the double sums [2][C]."""
    fin = bn_ref.finalize(sums, n, gamma, beta, EPS, MOM, rm0, rv0, None, shift, dtype=LD)
    s = sums.numpy().astype(LD).reshape(2, -1)
    m0, q = fin["m0"], s[1] / LD(n)
    g = np.abs(gamma.numpy().astype(LD)) if gamma is not None else LD(1)
    b = np.abs(beta.numpy().astype(LD)) if beta is not None else LD(0)
    mean, inv, sc, sh = (fin[k] for k in ("mean", "invstd", "scale", "shift"))
    dv = E * (q + 3 * m0 * m0 + np.abs(q - m0 * m0))
    dmean = E * (np.abs(m0) + np.abs(mean))
    dinv = inv ** 3 / 2 * dv + 3 * E * inv
    dscale = g * dinv + E * np.abs(sc)
    ms = np.abs(mean * sc)
    dshift = np.abs(sc) * dmean + np.abs(mean) * dscale + E * ms + E * (b + ms)
    for i, (tag, want, d) in enumerate((("mean", mean, dmean), ("invstd", inv, dinv),
                                        ("scale", sc, dscale), ("shift", sh, dshift))):
        err = np.abs(save[i].numpy().astype(LD) - want)
        ratio(3, f"{what} {tag}", f64(err), f64(U * (np.abs(want) + d) + d))
    if rm0 is None:
        return fin
    dunb = dv * n / (n - 1) + 2 * E * fin["unbiased"] if n > 1 else dv
    for tag, got, old, new, dnew in (("running_mean", rm, rm0, mean, dmean),
                                     ("running_var", rv, rv0, fin["unbiased"], dunb)):
        want = fin[tag]
        d = MOM * dnew + 3 * E * (np.abs((1 - LD(MOM)) * old.numpy().astype(LD)) + np.abs(LD(MOM) * new))
        err = np.abs(got.numpy().astype(LD) - want)
        ratio(3, f"{what} {tag}", f64(err), f64(U * (np.abs(want) + d) + d))
    return fin


def grads_rule(what, got, s, prev):
    """dgamma / dbeta += (float)s onto prev (None: the pointer was NULL and nothing is read)."""
    new = s.double() + prev.double()
    ratio(3, what, (got.double() - new).abs(), U * (s.double().abs() + new.abs()))


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def layer_data(c, shape, seed=0):
    """The fixed inputs of a (C, (n, h, w)) case; never modified by a test."""
    n, h, w = shape
    g = gen(1000 * c + n * h * w + seed)
    x = torch.randn((n, h, w, c), generator=g) * (0.25 + 1.75 * torch.rand(c, generator=g)) + \
        (8 * torch.rand(c, generator=g) - 4)
    if c >= 2:
        x[..., 1] = 3.0  # variance exactly 0
    x[0, 0, 0, 0] = 2.0
    if c >= 3:
        x[0, 0, 0, 2] = -0.0
    gamma = 1 + 0.3 * torch.randn(c, generator=g)
    gamma[3 if c > 3 else 0] = -gamma[3 if c > 3 else 0].abs() - 0.1
    beta = 0.3 * torch.randn(c, generator=g)
    p = n * h * w
    sums, _ = bn_ref.stats_sums(x)
    save = bn_ref.save_of(bn_ref.finalize(sums, p, gamma, beta, EPS)).float()
    save[2, 0], save[3, 0] = 0.5, -1.0  # x = 2: exactly +0
    if c >= 3:
        save[2, 2], save[3, 2] = 0.5, -0.0  # x = -0: exactly -0
    dy = torch.randn((n, h, w, c), generator=g)
    res = torch.randn((n, h, w, c), generator=g)
    rx = torch.randn((n, h, w, c), generator=g) * 1.5 + 0.5
    rgamma = 1 + 0.3 * torch.randn(c, generator=g)
    rsave = bn_ref.save_of(bn_ref.finalize(bn_ref.stats_sums(rx)[0], p, rgamma,
                                           0.3 * torch.randn(c, generator=g), EPS)).float()
    pre = bn_ref.pre_act(x, save[2], save[3])
    assert bool(((pre == 0) | (pre.abs() >= 2.0 ** -100)).all())  # no denormal decides a mask
    assert float(pre[0, 0, 0, 0]) == 0.0 and not bool((pre > 0)[0, 0, 0, 0])
    y = bn_ref.relu(pre + res.double()).float()  # a stored output: a test input of the backward
    yf = y.view(-1)
    for i, v in ((3, 0.0), (5, -0.0), (7, TINY)):
        yf[i % yf.numel()] = v
    prev = torch.randn((n, h, w, c), generator=g)
    return dict(x=x, gamma=gamma, beta=beta, save=save, dy=dy, res=res, rx=rx, rgamma=rgamma,
                rsave=rsave, y=y, prev=prev, p=p, c=c, shape=(n, h, w, c))


def with_nan_inf(t):
    """A copy with one NaN and one +Inf (the last two elements), for element-wise kernels."""
    t = t.clone()
    if t.numel() >= 5:
        t.view(-1)[-1], t.view(-1)[-2] = NAN, INF
    return t


# C = 18: rows = 51, pass = 204: one pixel, fewer than the rows, one pass, one pass + 11 (a
# one-pixel tail of the two-in-flight loop: 215 = 4 * 51 + 11), one pass + 58
SHAPES_18 = [(1, 1, 1), (1, 1, 7), (1, 12, 17), (1, 5, 43), (2, 1, 131)]
# one odd P for every other C; 1028 channels at P = 9 give 3 partial rows
OTHER_C = {1: (1, 3, 7), 3: (1, 3, 7), 36: (1, 7, 11), 72: (1, 5, 9), 270: (1, 5, 7),
           1024: (1, 1, 9), 1028: (1, 1, 9), 257: (1, 1, 7)}
BASE = [(18, s) for s in SHAPES_18] + list(OTHER_C.items())
# more than one pass per block with tune key 19 = 256: (C, shape) -> (ppb, rows)
MULTIPASS = {(72, (3, 64, 80)): (112, 138), (270, (1, 56, 56)): (24, 131)}


def case_id(v):
    if isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], tuple):
        return f"c{v[0]}-{'x'.join(map(str, v[1]))}"
    return None


# --------------------------------------------------- 1. statistics sums ----

STATS = [(cs, lay, 1024) for cs in BASE for lay in ("dense", "aligned", "c0=1")] + \
        [(cs, lay, 256) for cs in MULTIPASS for lay in ("aligned", "odd")]


@pytest.mark.parametrize("cs,layout,blocks", STATS, ids=lambda v: case_id(v) or str(v))
def test_stats_and_partials_reduce(cs, layout, blocks):
    call, lib, ptr, s = abi()
    c, shape = cs
    d = layer_data(c, shape)
    x, p = d["x"], d["p"]
    X = S(x, layout)
    quad = quad_ok(c) and v4(X)
    ppb = ppb_of(p, c, blocks)
    names = []
    with tune(lib, 19, blocks):
        rows = int(lib.vae2_bn_partial_rows(X.ref))
        assert rows == -(-p // ppb)
        if cs in MULTIPASS:
            assert (ppb, rows) == MULTIPASS[cs]
        part = Guarded(torch.full((2 * rows * c,), NAN))
        with logged(lib, names):
            call("vae2_bn_stats", X.ptr, X.ref, part.ptr, s)
    torch.cuda.synchronize()
    assert names == ["chan_partials_q_kernel<0>" if quad else "chan_partials_kernel<0>"], names
    assert X.intact() and part.intact() and same_bits(X.read(), x)
    rowsf = part.read().view(2, rows, c)
    want, terms = bn_ref.stats_sums(x)
    k = chain_k(c, ppb, quad)
    sums_rule(f"stats c={c} {shape} {layout} {names[0]}", rowsf, want, terms, k, k + 1)
    # the row reduction, then the same rows accumulated onto it
    sums = Guarded(torch.full((2 * c,), NAN, dtype=torch.float64))
    names = []
    with logged(lib, names):
        call("vae2_bn_partials_reduce", part.ptr, rows, c, sums.ptr, 0, s)
    torch.cuda.synchronize()
    first = sums.read().view(2, c)
    assert sums.intact() and part.intact() and names == ["partials_reduce_kernel"]
    rows_rule(f"partials_reduce c={c} rows={rows}", first, rowsf)
    call("vae2_bn_partials_reduce", part.ptr, rows, c, sums.ptr, 1, s)
    torch.cuda.synchronize()
    assert sums.intact() and same_bits(part.read().view(2, rows, c), rowsf)
    rows_rule(f"partials_reduce accumulate c={c} rows={rows}", sums.read().view(2, c), rowsf, first)


# ------------------------------------------------------------ 2. finalize ----

def synth(c, n, kind, shifted, seed):
    """Per-channel (mean, biased variance) and the double sums [2][C] that give them over n
    values, of x - 50 when shifted.  kind "clamp": s1 / n - m0^2 comes out slightly negative;
    n = 1: fp32-representable values, so x^2 is exact and the variance is exactly 0."""
    g = gen(seed)
    mean = (8 * torch.rand(c, generator=g, dtype=torch.float64) - 4) + (50.0 if shifted else 0.0)
    var = 0.06 + 4 * torch.rand(c, generator=g, dtype=torch.float64)
    var[c // 2] = 0.0
    m0 = mean - (50.0 if shifted else 0.0)
    if n == 1:
        m0 = m0.float().double()
        var = torch.zeros(c, dtype=torch.float64)
    s1 = n * (var + m0 * m0)
    if kind == "clamp":
        s1 = n * (m0 * m0) * (1 - 1e-12)
    return torch.stack([n * m0, s1])


def fin_args(c, variant, shifted, seed):
    """(gamma, beta, running_mean, running_var, num_batches_tracked, mean_shift) of a variant:
    "full" everything set, "null" every optional pointer NULL, "clamp" as full."""
    if variant == "null":
        return None, None, None, None, None, None
    g = gen(seed + 1)
    gamma = 1 + 0.3 * torch.randn(c, generator=g)
    gamma[0] = -gamma[0].abs()
    return (gamma, 0.3 * torch.randn(c, generator=g), torch.randn(c, generator=g),
            0.5 + torch.rand(c, generator=g), torch.tensor([41], dtype=torch.int64),
            torch.full((c,), 50.0) if shifted else None)


def G(t, **kw):
    return Guarded(t, **kw) if t is not None else None


def P(gd):
    return gd.ptr if gd is not None else None


@pytest.mark.parametrize("variant", ["full", "null", "clamp"])
@pytest.mark.parametrize("count", [1, 1000])
@pytest.mark.parametrize("c", [1, 18, 300])
@pytest.mark.parametrize("shifted", [False, True], ids=["plain", "shifted"])
def test_finalize_from_sums(shifted, c, count, variant):
    call, lib, ptr, s = abi()
    sums = synth(c, count, variant, shifted and variant != "null", 7 * c + count)
    gamma, beta, rm0, rv0, nbt0, shift = fin_args(c, variant, shifted, c)
    Sm, Ga, Be, Rm, Rv, Nb, Sh = (G(t) for t in (sums, gamma, beta, rm0, rv0, nbt0, shift))
    save = Guarded(torch.full((4 * c,), NAN))
    names = []
    for rep in (1, 2):
        with logged(lib, names):
            if shifted:
                call("vae2_bn_finalize_shifted", Sm.ptr, float(count), P(Sh), P(Ga), P(Be), P(Rm),
                     P(Rv), P(Nb), MOM, EPS, c, save.ptr, s)
            else:
                call("vae2_bn_finalize", Sm.ptr, float(count), P(Ga), P(Be), P(Rm), P(Rv), P(Nb),
                     MOM, EPS, c, save.ptr, s)
        torch.cuda.synchronize()
        assert all(b is None or b.intact() for b in (Sm, Ga, Be, Rm, Rv, Nb, Sh, save))
        assert torch.equal(Sm.read().view(2, c), sums)
        fin = finalize_rule(f"finalize{'_shifted' if shifted else ''} c={c} n={count} {variant} #{rep}",
                            save.read().view(4, c), Rm and Rm.read(), Rv and Rv.read(), sums, count,
                            gamma, beta, rm0, rv0, shift)
        if variant == "clamp" or count == 1:
            assert bool((f64(fin["var"]) == 0).all())  # the clamp / the exactly-zero variance
        if nbt0 is not None:
            assert int(Nb.read()[0]) == 41 + rep  # exactly 1 per call
            rm0, rv0 = Rm.read(), Rv.read()  # the second call starts from the first one's
    assert names == ["bn_finalize_kernel"] * 2, names


@pytest.mark.parametrize("variant", ["full", "null", "clamp"])
@pytest.mark.parametrize("count", [1, 1000])
@pytest.mark.parametrize("rows", [1, 255, 257, 2049, 5000])
@pytest.mark.parametrize("c", [1, 18, 300])
@pytest.mark.parametrize("shifted", [False, True], ids=["plain", "shifted"])
def test_reduce_finalize_from_partial_rows(shifted, c, rows, count, variant):
    call, lib, ptr, s = abi()
    g = gen(rows + c)
    target = synth(c, count, variant, shifted and variant != "null", 3 * c + rows)
    # fp32 partial rows that sum to about the target: positive weights, so no cancellation
    wgt = 0.5 + torch.rand(2, rows, c, generator=g, dtype=torch.float64)
    part = (target.view(2, 1, c) * wgt / wgt.sum(1, keepdim=True)).float()
    if variant == "clamp":  # the rounding of the rows must not lift the variance above 0
        part[1] = (part[1].double() * (1 - 1e-5)).float()
    gamma, beta, rm0, rv0, nbt0, shift = fin_args(c, variant, shifted, c + rows)
    Pt, Ga, Be, Rm, Rv, Nb, Sh = (G(t) for t in (part, gamma, beta, rm0, rv0, nbt0, shift))
    Sm = Guarded(torch.full((2 * c,), NAN, dtype=torch.float64))
    save = Guarded(torch.full((4 * c,), NAN))
    names = []
    with logged(lib, names):
        if shifted:
            call("vae2_bn_reduce_finalize_shifted", Pt.ptr, rows, c, Sm.ptr, float(count), P(Sh),
                 P(Ga), P(Be), P(Rm), P(Rv), P(Nb), MOM, EPS, save.ptr, s)
        else:
            call("vae2_bn_reduce_finalize", Pt.ptr, rows, c, Sm.ptr, float(count), P(Ga), P(Be),
                 P(Rm), P(Rv), P(Nb), MOM, EPS, save.ptr, s)
    torch.cuda.synchronize()
    assert names == ["reduce_then_kernel<0>"], names
    assert all(b is None or b.intact() for b in (Pt, Sm, Ga, Be, Rm, Rv, Nb, Sh, save))
    assert same_bits(Pt.read().view(2, rows, c), part)
    sums = Sm.read().view(2, c)
    what = f"reduce_finalize{'_shifted' if shifted else ''} c={c} rows={rows} n={count} {variant}"
    rows_rule(what + " sums", sums, part)
    fin = finalize_rule(what, save.read().view(4, c), Rm and Rm.read(), Rv and Rv.read(), sums,
                        count, gamma, beta, rm0, rv0, shift)
    if variant == "clamp":
        assert bool((f64(fin["var"]) == 0).all())
    if nbt0 is not None:
        assert int(Nb.read()[0]) == 42


# ------------------------------------------------ 3. the ill-conditioned chain ----

@pytest.mark.parametrize("m", [0.0, 4.0, 50.0])
def test_stats_to_finalize_chain(m):
    """vae2_bn_stats then vae2_bn_reduce_finalize on x ~ N(m, 0.5): the rule-1 bounds of the two
    sums propagated through mean = s0 / n (+ shift) and invstd = 1 / sqrt(s1 / n - m0^2 + eps).
    m = 50 goes through the shifted path (statistics of x - 50, exact in fp32) and gets the
    bound of the shifted sums: no cancellation of E[x^2] - E[x]^2 at |mean| = 100 std."""
    call, lib, ptr, s = abi()
    c, shape = 18, (4, 16, 16)
    p = 1024
    x = m + 0.5 * torch.randn(shape + (c,), generator=gen(int(m) + 1))
    shifted = m == 50.0
    xs = x - 50.0 if shifted else x
    assert torch.equal(xs.double(), x.double() - (50.0 if shifted else 0.0))  # exact
    X = S(xs, "aligned")
    with tune(lib, 19, 1024):
        rows = int(lib.vae2_bn_partial_rows(X.ref))
        ppb = ppb_of(p, c, 1024)
        assert rows == -(-p // ppb) == 6
        part = Guarded(torch.full((2 * rows * c,), NAN))
        call("vae2_bn_stats", X.ptr, X.ref, part.ptr, s)
    Sm = Guarded(torch.full((2 * c,), NAN, dtype=torch.float64))
    save = Guarded(torch.full((4 * c,), NAN))
    Sh = Guarded(torch.full((c,), 50.0))
    if shifted:
        call("vae2_bn_reduce_finalize_shifted", part.ptr, rows, c, Sm.ptr, float(p), Sh.ptr, None,
             None, None, None, None, MOM, EPS, save.ptr, s)
    else:
        call("vae2_bn_reduce_finalize", part.ptr, rows, c, Sm.ptr, float(p), None, None, None,
             None, None, MOM, EPS, save.ptr, s)
    torch.cuda.synchronize()
    assert X.intact() and part.intact() and Sm.intact() and save.intact() and Sh.intact()
    k = chain_k(c, ppb, True)
    want, terms = bn_ref.stats_sums(xs)
    # the sum over rows of K U sum|t| + U |row sum|, and the double reduction (rule 2)
    ds0 = ((k + 1) * U + rows * E) * terms[0]
    ds1 = ((k + 2) * U + rows * E) * terms[1]
    m0 = want[0] / p
    truth = bn_ref.finalize(bn_ref.stats_sums(x)[0], p, eps=EPS, dtype=LD)  # of x itself
    mean, inv = f64(truth["mean"]), f64(truth["invstd"])
    q = want[1] / p
    bmean = ds0 / p + U * mean.abs() + E * (m0.abs() + mean.abs())  # (+ dmean of rule 3)
    bvar = ds1 / p + 2 * m0.abs() * ds0 / p + E * (q + 3 * m0 * m0 + (q - m0 * m0).abs())
    binv = inv ** 3 / 2 * bvar + (U + 3 * E) * inv
    got = save.read().view(4, c).double()
    emean, einv = (got[0] - mean).abs(), (got[1] - inv).abs()
    print(f"CHAIN m={m:g} {'shifted' if shifted else 'plain'}: mean err {float(emean.max()):.3e} "
          f"(bound {float(bmean.max()):.3e}, rel {float((emean / mean.abs().clamp_min(1)).max()):.3e}), "
          f"invstd err {float(einv.max()):.3e} (bound {float(binv.max()):.3e}, "
          f"rel {float((einv / inv).max()):.3e})")
    ratio("3-chain", f"chain m={m:g} mean", emean, bmean)
    ratio("3-chain", f"chain m={m:g} invstd", einv, binv)


# -------------------------------------------------------- 4. eval coefficients ----

@pytest.mark.parametrize("affine", [True, False], ids=["gamma-beta", "null"])
@pytest.mark.parametrize("c", [1, 18, 300])
def test_eval_coeffs(c, affine):
    call, lib, ptr, s = abi()
    g = gen(c)
    gamma = 1 + 0.3 * torch.randn(c, generator=g) if affine else None
    beta = 0.3 * torch.randn(c, generator=g) if affine else None
    rm, rv = 4 * torch.randn(c, generator=g), 0.06 + 4 * torch.rand(c, generator=g)
    rv[c // 2] = 0.0
    Ga, Be, Rm, Rv = G(gamma), G(beta), G(rm), G(rv)
    save = Guarded(torch.full((4 * c,), NAN))
    names = []
    with logged(lib, names):
        call("vae2_bn_eval_coeffs", P(Ga), P(Be), Rm.ptr, Rv.ptr, EPS, c, save.ptr, s)
    torch.cuda.synchronize()
    assert names == ["bn_eval_kernel"]
    assert all(b is None or b.intact() for b in (Ga, Be, Rm, Rv, save))
    one, zero = torch.ones(c), torch.zeros(c)
    inv32 = 1.0 / torch.sqrt(rv + np.float32(EPS))
    g32, b32 = (gamma, beta) if affine else (one, zero)
    x32 = torch.stack([rm, inv32, g32 * inv32, b32 - rm * g32 * inv32])
    check_ew(f"eval_coeffs c={c} affine={affine}", save.read().view(4, c), x32,
             bn_ref.eval_coeffs(gamma, beta, rm, rv, EPS))
    assert same_bits(save.read().view(4, c)[0], rm)  # the mean is a copy


# ------------------------------------------------------------ 5. forward apply ----

def apply_truth(d, x, res, relu, rb=False):
    """(want64 after the ReLU, the bound of rule 4) of one layer."""
    pre = bn_ref.pre_act(x, d["save"][2], d["save"][3])
    if res is not None:
        want = pre + res.double()
        bound = U * (pre.abs() + want.abs())
    elif rb:
        rpre = bn_ref.pre_act(d["rx"], d["rsave"][2], d["rsave"][3])
        want = pre + rpre
        bound = U * (pre.abs() + want.abs() + rpre.abs())
    else:
        want, bound = pre, U * pre.abs()
    return (bn_ref.relu(want) if relu else want), bound


# layouts of (x, y, res): all the same, or one operand alone off the 16-byte grid
APPLY_LAYOUTS = {"dense": ("dense",) * 3, "aligned": ("aligned",) * 3, "c0=1": ("c0=1",) * 3,
                 "x-odd": ("odd", "aligned", "aligned"), "y-c0=1": ("aligned", "c0=1", "aligned"),
                 "res-odd": ("aligned", "aligned", "odd"), "res-aligned": ("c0=1", "c0=1", "aligned")}
APPLY = [(cs, lay) for cs in BASE for lay in ("dense", "aligned", "c0=1")] + \
        [(cs, lay) for cs in ((18, (1, 5, 43)), (36, (1, 7, 11)), (1028, (1, 1, 9)))
         for lay in ("x-odd", "y-c0=1", "res-odd", "res-aligned")]


@pytest.mark.parametrize("use_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("cs,layout", APPLY, ids=lambda v: case_id(v) or str(v))
def test_apply(cs, layout, relu, use_res):
    call, lib, ptr, s = abi()
    c, shape = cs
    d = layer_data(c, shape)
    lx, ly, lr = APPLY_LAYOUTS[layout]
    x = with_nan_inf(d["x"])
    res = d["res"] if use_res else None
    X, Y = S(x, lx), S(torch.full(d["shape"], NAN), ly)
    R = S(res, lr) if use_res else None
    save = Guarded(d["save"])
    names = []
    with logged(lib, names):
        call("vae2_bn_apply", X.ptr, X.ref, save.ptr, R.ptr if R else None, R.ref if R else Y.ref,
             Y.ptr, Y.ref, relu, s)
    torch.cuda.synchronize()
    ops_v4 = v4(X) and v4(Y) and (R is None or v4(R))
    want_kernel = "bn_apply_q_kernel" if quad_ok(c) and ops_v4 else \
        "bn_apply_kernel_v4" if c % 4 == 0 and ops_v4 else "bn_apply_kernel"
    assert names == [want_kernel], (names, want_kernel)
    assert X.intact() and Y.intact() and save.intact() and (R is None or R.intact())
    assert same_bits(X.read(), x)
    want, bound = apply_truth(d, x, res, relu)
    elementwise(4, f"apply c={c} {shape} {layout} relu={relu} res={use_res} {want_kernel}",
                Y.read(), want, bound)


# --------------------------------------------- 6. backward reduce, parameter gradients ----

def mask_truth(d, mode, y=None):
    """The exact ReLU mask of a mode: from the stored y (or mask bytes made of it), recomputed
    from x, or none."""
    if mode == "none":
        return None
    if mode == "recompute":
        return bn_ref.pre_act(d["x"], d["save"][2], d["save"][3]) > 0
    return bn_ref.mask_of(d["y"] if y is None else y)


# layouts of (x, y, dy, dx, dres)
BWD_LAYOUTS = {"dense": ("dense",) * 5, "aligned": ("aligned",) * 5, "c0=1": ("c0=1",) * 5,
               "odd": ("odd",) * 5,
               "x-odd": ("odd", "aligned", "aligned", "aligned", "aligned"),
               "y-odd": ("aligned", "odd", "aligned", "aligned", "aligned"),
               "dy-c0=1": ("aligned", "aligned", "c0=1", "aligned", "aligned"),
               "dx-odd": ("aligned", "aligned", "aligned", "odd", "aligned"),
               "dres-c0=1": ("aligned", "aligned", "aligned", "aligned", "c0=1")}
ONE_OFF = ((18, (1, 5, 43)), (36, (1, 7, 11)))
REDUCE = [(cs, lay, 1024) for cs in BASE for lay in ("dense", "aligned", "c0=1")] + \
         [(cs, lay, 1024) for cs in ONE_OFF for lay in ("x-odd", "y-odd", "dy-c0=1")] + \
         [(cs, lay, 256) for cs in MULTIPASS for lay in ("aligned", "odd")]


@pytest.mark.parametrize("mode", ["y", "recompute", "none"])
@pytest.mark.parametrize("cs,layout,blocks", REDUCE, ids=lambda v: case_id(v) or str(v))
def test_bwd_reduce_and_param_grads(cs, layout, blocks, mode):
    call, lib, ptr, s = abi()
    c, shape = cs
    d = layer_data(c, shape)
    x, dy, p = d["x"], d["dy"], d["p"]
    lx, ly, ldy = BWD_LAYOUTS[layout][:3]
    X, DY = S(x, lx), S(dy, ldy, sent=333.0)
    Y = S(d["y"], ly, sent=555.0) if mode == "y" else None
    save = Guarded(d["save"])
    quad = quad_ok(c) and v4(X) and v4(DY) and (Y is None or v4(Y))
    ppb = ppb_of(p, c, blocks)
    names = []
    with tune(lib, 19, blocks):
        rows = int(lib.vae2_bn_partial_rows(X.ref))
        assert rows == -(-p // ppb)
        part = Guarded(torch.full((2 * rows * c,), NAN))
        with logged(lib, names):
            call("vae2_bn_relu_bwd_reduce", DY.ptr, DY.ref, Y.ptr if Y else None,
                 Y.ref if Y else X.ref, X.ptr, X.ref, save.ptr, int(mode != "none"), part.ptr, s)
    torch.cuda.synchronize()
    assert names == ["chan_partials_q_kernel<1>" if quad else "chan_partials_kernel<1>"], names
    assert X.intact() and DY.intact() and part.intact() and save.intact() and (Y is None or Y.intact())
    m = mask_truth(d, mode)
    g = bn_ref.masked(dy, m)
    want, terms = bn_ref.bwd_sums(g, x, d["save"][0], d["save"][1])
    k = chain_k(c, ppb, quad)
    rowsf = part.read().view(2, rows, c)
    tag = f"c={c} {shape} {layout} {mode}"
    sums_rule(f"bwd_reduce {tag} {names[0]}", rowsf, want, terms, k, k + 3)
    # rows -> double sums (+ parameter gradients): NULL gradients, then onto earlier values
    sums = Guarded(torch.full((2 * c,), NAN, dtype=torch.float64))
    names = []
    with logged(lib, names):
        call("vae2_bn_bwd_reduce_param_grads", part.ptr, rows, c, sums.ptr, None, None, s)
    torch.cuda.synchronize()
    got = sums.read().view(2, c)
    assert names == ["reduce_then_kernel<1>"] and sums.intact() and part.intact()
    rows_rule(f"bwd_reduce_param_grads {tag} sums", got, rowsf)
    pg, pb = torch.randn(c, generator=gen(c)), torch.randn(c, generator=gen(c + 1))
    DG, DB = Guarded(pg), Guarded(pb)
    sums2 = Guarded(torch.full((2 * c,), NAN, dtype=torch.float64))
    call("vae2_bn_bwd_reduce_param_grads", part.ptr, rows, c, sums2.ptr, DG.ptr, DB.ptr, s)
    torch.cuda.synchronize()
    assert DG.intact() and DB.intact() and sums2.intact() and torch.equal(sums2.read().view(2, c), got)
    grads_rule(f"bwd_reduce_param_grads {tag} dgamma", DG.read(), got[1], pg)
    grads_rule(f"bwd_reduce_param_grads {tag} dbeta", DB.read(), got[0], pb)
    # the same from the double sums; with dgamma NULL only dbeta is touched
    DG, DB, DB2 = Guarded(pg), Guarded(pb), Guarded(pb)
    names = []
    with logged(lib, names):
        call("vae2_bn_bwd_param_grads", sums.ptr, c, DG.ptr, DB.ptr, s)
        call("vae2_bn_bwd_param_grads", sums.ptr, c, None, DB2.ptr, s)
    torch.cuda.synchronize()
    assert names == ["bn_param_grad_kernel"] * 2 and sums.intact()
    assert DG.intact() and DB.intact() and DB2.intact()
    grads_rule(f"bwd_param_grads {tag} dgamma", DG.read(), got[1], pg)
    grads_rule(f"bwd_param_grads {tag} dbeta", DB.read(), got[0], pb)
    assert same_bits(DB2.read(), DB.read())


# ----------------------------------------------------------- 7. backward apply ----

# (mask source, dres, gamma, count = 2 P with doubled sums)
BWD_VARIANTS = {"y-dres": ("y", True, True, False), "y": ("y", False, True, False),
                "recompute": ("recompute", False, True, False),
                "recompute-dres-nogamma-2P": ("recompute", True, False, True),
                "none-dres": ("none", True, True, False), "none-nogamma-2P": ("none", False, False, True)}
BWD_APPLY = [(cs, lay) for cs in BASE for lay in ("dense", "aligned", "c0=1")] + \
            [(cs, lay) for cs in ONE_OFF for lay in ("x-odd", "y-odd", "dy-c0=1", "dx-odd", "dres-c0=1")]


@pytest.mark.parametrize("variant", list(BWD_VARIANTS))
@pytest.mark.parametrize("cs,layout", BWD_APPLY, ids=lambda v: case_id(v) or str(v))
def test_bwd_apply(cs, layout, variant):
    call, lib, ptr, s = abi()
    c, shape = cs
    d = layer_data(c, shape)
    mode, use_dres, use_gamma, twice = BWD_VARIANTS[variant]
    x, dy, p = d["x"], d["dy"], d["p"]
    y = with_nan_inf(d["y"])  # a NaN y cuts the gradient, +Inf passes it
    lx, ly, ldy, ldx, ldr = BWD_LAYOUTS[layout]
    X, DY = S(x, lx), S(dy, ldy, sent=333.0)
    Y = S(y, ly, sent=555.0) if mode == "y" else None
    DX = S(torch.full(d["shape"], NAN), ldx)
    DR = S(torch.full(d["shape"], NAN), ldr) if use_dres else None
    m = mask_truth(d, mode, y)
    g = bn_ref.masked(dy, m)
    f = 2 if twice else 1
    sums64 = f * bn_ref.bwd_sums(g, x, d["save"][0], d["save"][1])[0]
    count = float(f * p)
    save, Sm, Ga = Guarded(d["save"]), Guarded(sums64), G(d["gamma"] if use_gamma else None)
    names = []
    with logged(lib, names):
        call("vae2_bn_relu_bwd_apply", DY.ptr, DY.ref, Y.ptr if Y else None, Y.ref if Y else X.ref,
             X.ptr, X.ref, save.ptr, P(Ga), Sm.ptr, count, int(mode != "none"), DX.ptr, DX.ref,
             DR.ptr if DR else None, DR.ref if DR else DX.ref, s)
    torch.cuda.synchronize()
    quad = quad_ok(c) and all(v4(t) for t in (X, DY, DX, Y, DR) if t is not None)
    want_kernel = "bn_bwd_apply_q_kernel" if quad else "bn_bwd_apply_kernel"
    assert names == [want_kernel], (names, want_kernel)
    assert all(t is None or t.intact() for t in (X, DY, Y, DX, DR, save, Sm, Ga))
    assert same_bits(X.read(), x) and same_bits(DY.read(), dy)
    want, terms = bn_ref.bwd_apply(g, x, d["save"][0], d["save"][1],
                                   d["gamma"] if use_gamma else None, sums64, count)
    tag = f"c={c} {shape} {layout} {variant} {want_kernel}"
    elementwise(5, f"bwd_apply dx {tag}", DX.read(), want, 8 * U * terms)
    if DR:
        check_bits(f"bwd_apply dres {tag}", DR.read(), g)


# ------------------------------------------------------ 8. the multi-layer launches ----

MULTI = [(18, (1, 5, 43)), (36, (1, 7, 11)), (72, (1, 5, 9)), (3, (1, 1, 1)), (270, (1, 5, 7)),
         (1024, (1, 1, 9)), (1, (1, 3, 7)), (18, (2, 1, 131))]  # 6 + 2 layers: two launches
MODES = {"mix": ["mask", "y", "recompute", "none", "mask", "y", "recompute", "mask"],  # ACT 3
         "act0": ["recompute", "recompute", "recompute", "none", "recompute", "recompute", "none",
                  "recompute"],
         "act1": ["mask"] * 8, "act2": ["y"] * 8}
ACT_OF = {"none": 0, "recompute": 0, "mask": 1, "y": 2}
RB_LAYER, ACC_LAYER, DRES_LAYERS, COUNTP_LAYERS, NOGAMMA_LAYER, TWICE_LAYER = 1, 0, (0, 2, 7), (0, 4), 5, 7
TUNES = {"default": (), "r4": ((8, 0),), "stride3": ((20, 3),)}


def launches(flags):
    """Per launch of up to 6 layers: the union of the layers' features, as the host forms it."""
    out = []
    for i0 in range(0, len(flags), 6):
        grp = flags[i0:i0 + 6]
        acts = {a for a, _, _ in grp}
        out.append((acts.pop() if len(acts) == 1 else 3, any(r for _, r, _ in grp),
                    any(a for _, _, a in grp)))
    return out


def tf(b):
    return "true" if b else "false"


@pytest.mark.parametrize("tuning", list(TUNES))
@pytest.mark.parametrize("dacc", [0, 1], ids=["dres=", "dres+="])
@pytest.mark.parametrize("rb", [0, 1], ids=["norb", "rb"])
@pytest.mark.parametrize("cfg", list(MODES))
def test_multi_apply_and_backward(cfg, rb, dacc, tuning):
    from vae2 import _lib
    call, lib, ptr, s = abi()
    modes = MODES[cfg]
    D = [layer_data(c, shape, seed=i) for i, (c, shape) in enumerate(MULTI)]
    n = len(D)
    r4k = tuning == "r4"
    with contextlib.ExitStack() as st:
        st.enter_context(tune(lib, 19, 1024))
        for key, val in TUNES[tuning]:
            st.enter_context(tune(lib, key, val))
        # ---- forward: y = relu?(fma(x, scale, shift) + residual | residual BN), mask bytes
        lay = (_lib.BnLayer * n)()
        keep = []
        for i, d in enumerate(D):
            c = d["c"]
            x = with_nan_inf(d["x"])
            has_rb = bool(rb) and i == RB_LAYER
            res = d["res"] if modes[i] in ("mask", "y") and not has_rb else None
            X, Y = S(x, "aligned"), S(torch.full(d["shape"], NAN), "aligned")
            R = S(res, "aligned") if res is not None else None
            RX = S(d["rx"], "aligned") if has_rb else None
            MK = Guarded(torch.full((d["p"] * ((c + 3) // 4),), 0xFF, dtype=torch.uint8)) \
                if modes[i] == "mask" else None
            save, rsave = Guarded(d["save"]), Guarded(d["rsave"])
            L = lay[i]
            L.x, L.xd, L.o, L.od, L.save = X.ptr.value, X.act, Y.ptr.value, Y.act, save.addr
            L.relu = int(modes[i] != "none")
            if R:
                L.a, L.ad = R.ptr.value, R.act
            if RX:
                L.rx, L.rxd, L.rsave = RX.ptr.value, RX.act, rsave.addr
            if MK:
                L.mask = MK.addr
            keep.append((x, res, X, Y, R, RX, MK, save, rsave, has_rb))
        names = []
        with logged(lib, names):
            call("vae2_bn_multi_apply", n, lay, s)
        torch.cuda.synchronize()
        assert names == ["bn_apply_multi_r4_kernel" if r4k else "bn_apply_multi_kernel"] * 2, names
        for i, d in enumerate(D):
            x, res, X, Y, R, RX, MK, save, rsave, has_rb = keep[i]
            assert all(t is None or t.intact() for t in (X, Y, R, RX, MK, save, rsave))
            want, bound = apply_truth(d, x, res, modes[i] != "none", has_rb)
            y = Y.read()
            elementwise(4, f"multi_apply {cfg} rb={rb} {tuning} layer {i} c={d['c']} p={d['p']}",
                        y, want, bound)
            if MK:
                bits = bn_ref.unpack_mask(MK.read().view(d["p"], -1), d["c"])
                assert torch.equal(bits, (y > 0).view(d["p"], d["c"])), ("mask bytes", i)
        # ---- backward: the mask bytes' bits of channels >= C all 0, then all 1
        runs = [_multi_backward(lib, call, s, D, modes, rb, dacc, pad, r4k) for pad in (0, 1)]
    for i, d in enumerate(D):
        for key in runs[0][i]:
            assert same_bits(runs[0][i][key], runs[1][i][key]), ("padding mask bits are read", i, key)


def _multi_backward(lib, call, s, D, modes, rb, dacc, pad, r4k):
    """vae2_bn_multi_bwd_reduce and _bwd_apply on fresh buffers, checked against the truth;
    returns every output per layer."""
    from vae2 import _lib
    n = len(D)
    lay = (_lib.BnLayer * n)()
    keep, flags = [], []
    cp = Guarded(torch.tensor([float(d["p"]) for d in D], dtype=torch.float64))
    for i, d in enumerate(D):
        c, p = d["c"], d["p"]
        y = with_nan_inf(d["y"])
        m = mask_truth(d, modes[i], y)
        g = bn_ref.masked(d["dy"], m)
        has_rb = bool(rb) and i == RB_LAYER
        f = 2 if i == TWICE_LAYER else 1
        want, terms = bn_ref.bwd_sums(g, d["x"], d["save"][0], d["save"][1])
        rwant, rterms = bn_ref.bwd_sums(g, d["rx"], d["rsave"][0], d["rsave"][1])
        ppb = ppb_of(p, c, 1024)
        rows = -(-p // ppb)
        X, DY = S(d["x"], "aligned"), S(d["dy"], "aligned", sent=333.0)
        DX = S(torch.full(d["shape"], NAN), "aligned")
        Y = S(y, "aligned", sent=555.0) if modes[i] == "y" else None
        MK = Guarded(bn_ref.pack_mask(m, pad)) if modes[i] == "mask" else None
        use_dres = i in DRES_LAYERS and not has_rb
        acc = bool(dacc) and i == ACC_LAYER and use_dres
        DR = S(d["prev"] if acc else torch.full(d["shape"], NAN), "aligned") if use_dres else None
        RX = S(d["rx"], "aligned") if has_rb else None
        RDX = S(torch.full(d["shape"], NAN), "aligned") if has_rb else None
        gamma = None if i == NOGAMMA_LAYER else d["gamma"]
        B = dict(save=Guarded(d["save"]), rsave=Guarded(d["rsave"]), gamma=G(gamma),
                 rgamma=Guarded(d["rgamma"]), part=Guarded(torch.full((2 * rows * c,), NAN)),
                 rpart=Guarded(torch.full((2 * rows * c,), NAN)), sums=Guarded(f * want),
                 rsums=Guarded(f * rwant))
        L = lay[i]
        assert int(lib.vae2_bn_partial_rows(X.ref)) == rows
        L.x, L.xd, L.o, L.od, L.dy, L.dyd = X.ptr.value, X.act, DX.ptr.value, DX.act, DY.ptr.value, DY.act
        L.save, L.gamma, L.partials, L.sums = B["save"].addr, B["gamma"] and B["gamma"].addr, \
            B["part"].addr, B["sums"].addr
        L.relu = int(modes[i] != "none")
        if i in COUNTP_LAYERS and f == 1:
            L.countp, L.count = cp.addr + 8 * i, -1.0  # the device count is the one used
        else:
            L.count = float(f * p)
        if Y:  # the first C channels of a descriptor that says more (ad.c >= c is allowed)
            L.a, L.ad = Y.ptr.value, _lib.Act(*d["shape"][:3], c + (4 if i == 1 else 0), Y.ps)
        if MK:
            L.mask = MK.addr
        if DR:
            L.dres, L.dresd, L.dres_acc = DR.ptr.value, DR.act, int(acc)
        if has_rb:
            L.rx, L.rxd, L.rsave, L.rgamma = RX.ptr.value, RX.act, B["rsave"].addr, B["rgamma"].addr
            L.rpartials, L.rsums, L.rdx, L.rdxd = B["rpart"].addr, B["rsums"].addr, RDX.ptr.value, RDX.act
        flags.append((ACT_OF[modes[i]], has_rb, acc))
        keep.append((X, DY, DX, Y, MK, DR, RX, RDX, B, g, want, terms, rwant, rterms, rows, ppb,
                     f, gamma, has_rb, acc))
    names = []
    with logged(lib, names):
        call("vae2_bn_multi_bwd_reduce", n, lay, s)
        call("vae2_bn_multi_bwd_apply", n, lay, s)
    torch.cuda.synchronize()
    want_names = ["bn_bwd_reduce_multi_r4_kernel"] * 2 + ["bn_bwd_apply_multi_r4_kernel"] * 2 if r4k else \
        [f"bn_bwd_reduce_multi_kernel<{a},{tf(r)}>" for a, r, _ in launches(flags)] + \
        [f"bn_bwd_apply_multi_kernel<{a},{tf(r)},{tf(ac)}>" for a, r, ac in launches(flags)]
    assert names == want_names, (names, want_names)
    assert cp.intact()
    out = []
    for i, d in enumerate(D):
        (X, DY, DX, Y, MK, DR, RX, RDX, B, g, want, terms, rwant, rterms, rows, ppb, f, gamma,
         has_rb, acc) = keep[i]
        c, p = d["c"], d["p"]
        assert all(t is None or t.intact() for t in (X, DY, DX, Y, MK, DR, RX, RDX, *B.values()))
        tag = f"{modes[i]} rb={int(has_rb)} acc={int(acc)} pad={pad} r4={int(r4k)} layer {i} c={c} p={p}"
        k = chain_k(c, ppb, True)
        o = dict(part=B["part"].read().view(2, rows, c), dx=DX.read())
        sums_rule(f"multi_bwd_reduce {tag}", o["part"], want, terms, k, k + 3)
        dxw, dterms = bn_ref.bwd_apply(g, d["x"], d["save"][0], d["save"][1], gamma, f * want, f * p)
        elementwise(5, f"multi_bwd_apply dx {tag}", o["dx"], dxw, 8 * U * dterms)
        if DR:
            o["dres"] = DR.read()
            check_bits(f"multi_bwd_apply dres {tag}", o["dres"], d["prev"] + g if acc else g)
        if has_rb:
            o["rpart"], o["rdx"] = B["rpart"].read().view(2, rows, c), RDX.read()
            sums_rule(f"multi_bwd_reduce rpartials {tag}", o["rpart"], rwant, rterms, k, k + 3)
            rw, rt = bn_ref.bwd_apply(g, d["rx"], d["rsave"][0], d["rsave"][1], d["rgamma"],
                                      f * rwant, f * p)
            elementwise(5, f"multi_bwd_apply rdx {tag}", o["rdx"], rw, 8 * U * rt)
        else:  # untouched
            assert bool(torch.isnan(B["rpart"].read()).all())
        out.append(o)
    return out


def _multi_forward(call, s, D, modes, rb):
    """vae2_bn_multi_apply on fresh buffers: y and the mask bytes per layer."""
    from vae2 import _lib
    lay = (_lib.BnLayer * len(D))()
    keep = []
    for i, d in enumerate(D):
        has_rb = bool(rb) and i == RB_LAYER
        res = d["res"] if modes[i] in ("mask", "y") and not has_rb else None
        X, Y = S(with_nan_inf(d["x"]), "aligned"), S(torch.full(d["shape"], NAN), "aligned")
        R = S(res, "aligned") if res is not None else None
        RX = S(d["rx"], "aligned") if has_rb else None
        MK = Guarded(torch.full((d["p"] * ((d["c"] + 3) // 4),), 0xFF, dtype=torch.uint8)) \
            if modes[i] == "mask" else None
        save, rsave = Guarded(d["save"]), Guarded(d["rsave"])
        L = lay[i]
        L.x, L.xd, L.o, L.od, L.save = X.ptr.value, X.act, Y.ptr.value, Y.act, save.addr
        L.relu = int(modes[i] != "none")
        if R:
            L.a, L.ad = R.ptr.value, R.act
        if RX:
            L.rx, L.rxd, L.rsave = RX.ptr.value, RX.act, rsave.addr
        if MK:
            L.mask = MK.addr
        keep.append((X, Y, R, RX, MK, save, rsave))
    call("vae2_bn_multi_apply", len(D), lay, s)
    torch.cuda.synchronize()
    out = []
    for X, Y, R, RX, MK, save, rsave in keep:
        assert all(t is None or t.intact() for t in (X, Y, R, RX, MK, save, rsave))
        out.append(dict(y=Y.read(), **({"mask": MK.read()} if MK else {})))
    return out


def test_multi_r4_matches_default_bits():
    """Tune key 8 = 0 (and with it the fallback for extents of 2 GB or more) runs the same
    arithmetic as the default buffer-resource kernels: every output of vae2_bn_multi_apply,
    _bwd_reduce and _bwd_apply agrees bit for bit (y, part, rpart, dx, dres, rdx), and so do the
    mask bytes' bits of the channels < C.  The bits of channels >= C in a partial quad's byte
    come from lanes that see different coefficients in the two forms (0 / the next coefficient
    row); they differ (C = 18 and 270 here), as they did before the bodies were shared, and no
    kernel reads them (test_multi_apply_and_backward runs the backward on both paddings)."""
    call, lib, ptr, s = abi()
    modes = MODES["mix"]
    D = [layer_data(c, shape, seed=i) for i, (c, shape) in enumerate(MULTI)]
    runs = []
    for r4k in (False, True):
        with contextlib.ExitStack() as st:
            st.enter_context(tune(lib, 19, 1024))
            if r4k:
                st.enter_context(tune(lib, 8, 0))
            fwd = _multi_forward(call, s, D, modes, 1)
            bwd = _multi_backward(lib, call, s, D, modes, 1, 1, 0, r4k)
        runs.append([{**f, **b} for f, b in zip(fwd, bwd)])
    seen = set()
    for i, (a, b) in enumerate(zip(*runs)):
        assert a.keys() == b.keys()
        for key in a:
            if key == "mask":  # one byte per (pixel, quad): the valid channels' bits
                va, vb = (bn_ref.unpack_mask(t.view(D[i]["p"], -1), D[i]["c"]) for t in (a[key], b[key]))
                assert torch.equal(va, vb), (i, key, MULTI[i])
            else:
                assert same_bits(a[key], b[key]), (i, key, MULTI[i])
            seen.add(key)
    assert seen == {"y", "mask", "part", "rpart", "dx", "dres", "rdx"}


def test_rejected_multi_call_writes_nothing():
    """A layer of the second launch disagrees in shape: -22, and no layer's output is touched."""
    from vae2 import _lib
    call, lib, ptr, s = abi()
    D = [layer_data(c, shape, seed=i) for i, (c, shape) in enumerate(MULTI)]
    lay = (_lib.BnLayer * len(D))()
    keep = []
    for i, d in enumerate(D):
        X, DY = S(d["x"], "aligned"), S(d["dy"], "aligned")
        DX, DR = S(torch.full(d["shape"], NAN), "aligned"), S(torch.full(d["shape"], NAN), "aligned")
        rows = -(-d["p"] // ppb_of(d["p"], d["c"], 1024))
        B = [Guarded(d["save"]), Guarded(torch.zeros(2 * d["c"], dtype=torch.float64)),
             Guarded(torch.full((2 * rows * d["c"],), NAN))]
        L = lay[i]
        L.x, L.xd, L.o, L.od, L.dy, L.dyd = X.ptr.value, X.act, DX.ptr.value, DX.act, DY.ptr.value, DY.act
        L.dres, L.dresd = DR.ptr.value, DR.act
        L.save, L.sums, L.partials, L.count, L.relu = B[0].addr, B[1].addr, B[2].addr, float(d["p"]), 1
        keep.append((X, DY, DX, DR, B))
    n_, h_, w_, c_ = D[7]["shape"]
    lay[7].dyd = _lib.Act(n_, h_, w_, c_ - 1, lay[7].dyd.ps)
    with tune(lib, 19, 1024):
        for entry in ("vae2_bn_multi_bwd_reduce", "vae2_bn_multi_bwd_apply"):
            names = []
            with logged(lib, names):
                rc = getattr(lib, entry)(len(D), lay, s)
            assert rc == -22 and b"matching shapes" in lib.vae2_last_error() and names == []
    torch.cuda.synchronize()
    for X, DY, DX, DR, B in keep:
        assert all(t.intact() for t in (X, DY, DX, DR, *B))
        assert bool(torch.isnan(DX.read()).all()) and bool(torch.isnan(DR.read()).all())
        assert bool(torch.isnan(B[2].read()).all())


# ------------------------------------- 9. multi-layer row reductions and finalize ----

FIN_C = [1, 18, 300, 3, 36, 72, 18, 270]
FIN_ROWS = [1, 255, 257, 2049, 5000, 7, 64, 300]
FIN_COUNT = 1000


def _fin_layers(cp, with_grads=False):
    """Eight vae2_bn_fin layers over synthetic partial rows; returns (array, per-layer data)."""
    from vae2 import _lib
    arr = (_lib.BnFin * 8)()
    keep = []
    for i, (c, rows) in enumerate(zip(FIN_C, FIN_ROWS)):
        g = gen(100 + i)
        target = synth(c, FIN_COUNT, "full", False, 50 + i)
        wgt = 0.5 + torch.rand(2, rows, c, generator=g, dtype=torch.float64)
        part = (target.view(2, 1, c) * wgt / wgt.sum(1, keepdim=True)).float()
        gamma, beta, rm0, rv0, nbt0, _ = fin_args(c, "null" if i == 3 else "full", False, i)
        if i == 5:
            rm0 = rv0 = nbt0 = None
        pg, pb = torch.randn(c, generator=g), torch.randn(c, generator=g)
        B = dict(part=Guarded(part), sums=Guarded(torch.full((2 * c,), NAN, dtype=torch.float64)),
                 gamma=G(gamma), beta=G(beta), rm=G(rm0), rv=G(rv0), nbt=G(nbt0),
                 save=Guarded(torch.full((4 * c,), NAN)),
                 dgamma=G(pg if with_grads and i != 2 else None), dbeta=G(pb if with_grads else None))
        a = lambda k: B[k].addr if B[k] is not None else None  # noqa: E731
        countp, count = (cp.addr + 8 * i, -1.0) if i in (0, 4) else (None, float(FIN_COUNT))
        arr[i] = _lib.BnFin(a("part"), rows, c, a("sums"), countp, count, a("gamma"), a("beta"),
                            a("rm"), a("rv"), a("nbt"), MOM, EPS, a("save"), a("dgamma"), a("dbeta"))
        keep.append(dict(B=B, part=part, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, pg=pg, pb=pb,
                         c=c, rows=rows))
    return arr, keep


def _fin_check(tag, keep, nbt_want):
    for i, k in enumerate(keep):
        B, c = k["B"], k["c"]
        assert all(b is None or b.intact() for b in B.values())
        finalize_rule(f"{tag} layer {i} c={c} rows={k['rows']}", B["save"].read().view(4, c),
                      B["rm"] and B["rm"].read(), B["rv"] and B["rv"].read(),
                      B["sums"].read().view(2, c), FIN_COUNT, k["gamma"], k["beta"], k["rm0"],
                      k["rv0"], None)
        if B["nbt"] is not None:
            assert int(B["nbt"].read()[0]) == nbt_want


def test_multi_reduce_and_finalize():
    call, lib, ptr, s = abi()
    cp = Guarded(torch.full((8,), float(FIN_COUNT), dtype=torch.float64))
    # mode 0: reduce + finalize
    arr0, k0 = _fin_layers(cp)
    names = []
    with logged(lib, names):
        call("vae2_bn_multi_reduce", 8, arr0, 0, s)
    torch.cuda.synchronize()
    assert names == ["reduce_then_multi_kernel<0>"] * 2, names
    for i, k in enumerate(k0):
        rows_rule(f"multi_reduce mode 0 layer {i}", k["B"]["sums"].read().view(2, k["c"]), k["part"])
    _fin_check("multi_reduce mode 0", k0, 42)
    # mode 2: sums only; then finalize from them: the same as mode 0
    arr2, k2 = _fin_layers(cp)
    names = []
    with logged(lib, names):
        call("vae2_bn_multi_reduce", 8, arr2, 2, s)
    torch.cuda.synchronize()
    assert names == ["reduce_then_multi_kernel<2>"] * 2, names
    for a, b in zip(k0, k2):
        assert torch.equal(a["B"]["sums"].read(), b["B"]["sums"].read())
        assert bool(torch.isnan(b["B"]["save"].read()).all())  # not finalized yet
        assert b["B"]["nbt"] is None or int(b["B"]["nbt"].read()[0]) == 41
        assert b["B"]["rm"] is None or same_bits(b["B"]["rm"].read(), b["rm0"])
    names = []
    with logged(lib, names):
        call("vae2_bn_multi_finalize", 8, arr2, s)
    torch.cuda.synchronize()
    assert names == ["bn_finalize_multi_kernel"] * 2, names
    _fin_check("multi_reduce mode 2 + multi_finalize", k2, 42)
    assert cp.intact()
    # mode 1: sums + parameter gradients onto earlier values (one dgamma NULL)
    arr1, k1 = _fin_layers(cp, with_grads=True)
    names = []
    with logged(lib, names):
        call("vae2_bn_multi_reduce", 8, arr1, 1, s)
    torch.cuda.synchronize()
    assert names == ["reduce_then_multi_kernel<1>"] * 2, names
    for i, k in enumerate(k1):
        B, c = k["B"], k["c"]
        assert all(b is None or b.intact() for b in B.values())
        got = B["sums"].read().view(2, c)
        rows_rule(f"multi_reduce mode 1 layer {i}", got, k["part"])
        if B["dgamma"] is not None:
            grads_rule(f"multi_reduce mode 1 layer {i} dgamma", B["dgamma"].read(), got[1], k["pg"])
        grads_rule(f"multi_reduce mode 1 layer {i} dbeta", B["dbeta"].read(), got[0], k["pb"])
        assert bool(torch.isnan(B["save"].read()).all())
        assert B["nbt"] is None or int(B["nbt"].read()[0]) == 41

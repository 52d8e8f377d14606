"""A plain high-precision reference of the BatchNorm operations of csrc/bn.hip, each written as
include/vae2_hip.h documents it.  Activations are (N, H, W, C) tensors, per-channel vectors have
C elements; everything is computed in float64 (finalize optionally in numpy longdouble) from
whatever precision the inputs have.  test_bn_ref.py checks it against
torch.nn.functional.batch_norm with autograd; test_bn_gpu.py takes its truth from here."""
import numpy as np
import torch


def _d(t):
    return None if t is None else torch.as_tensor(t).double()


# -------------------------------------------------------------- statistics ----

def stats_sums(x, shift=None):
    """(sum x, sum x^2) per channel over the pixels, of x - shift[c] when shift is given, and
    the sums of the absolute terms (sum |x|, the second sum itself)."""
    v = _d(x).reshape(-1, x.shape[-1])
    if shift is not None:
        v = v - _d(shift)
    return torch.stack([v.sum(0), (v * v).sum(0)]), torch.stack([v.abs().sum(0), (v * v).sum(0)])


def finalize(sums, count, gamma=None, beta=None, eps=1e-5, momentum=0.01, running_mean=None,
             running_var=None, num_batches_tracked=None, mean_shift=None, dtype=np.float64):
    """sums [2][C] = (sum x, sum x^2) (of x - mean_shift when given) over `count` values per
    channel -> save = (mean, invstd, scale, shift), scale = gamma * invstd, shift = beta -
    mean * scale; the variance is biased and clamped at 0; the running statistics take the
    unbiased variance (the biased one when count is 1); num_batches_tracked goes up by 1.
    Returns a dict of numpy arrays of `dtype` (np.longdouble for a truth beyond double)."""
    def a(t, fill=None):
        if t is None:
            return None if fill is None else np.full(c, fill, dtype=dtype)
        return np.asarray(torch.as_tensor(t).double().numpy(), dtype=dtype)
    s = np.asarray(torch.as_tensor(sums).double().numpy(), dtype=dtype).reshape(2, -1)
    c = s.shape[1]
    n = dtype(count)
    m0 = s[0] / n
    var = np.maximum(s[1] / n - m0 * m0, dtype(0))
    ms = a(mean_shift)
    mean = m0 + ms if ms is not None else m0
    invstd = 1 / np.sqrt(var + dtype(eps))
    g, b = a(gamma, 1.0), a(beta, 0.0)
    scale = g * invstd
    out = {"mean": mean, "invstd": invstd, "scale": scale, "shift": b - mean * scale,
           "var": var, "m0": m0}
    if running_mean is not None:
        unbiased = var * n / (n - 1) if count > 1 else var
        mom = dtype(momentum)
        out["running_mean"] = (1 - mom) * a(running_mean) + mom * mean
        out["running_var"] = (1 - mom) * a(running_var) + mom * unbiased
        out["unbiased"] = unbiased
    if num_batches_tracked is not None:
        out["num_batches_tracked"] = int(num_batches_tracked) + 1
    return out


def save_of(fin):
    """The [4][C] float64 tensor (mean, invstd, scale, shift) of a finalize() result."""
    return torch.from_numpy(np.stack([np.asarray(fin[k], dtype=np.float64)
                                      for k in ("mean", "invstd", "scale", "shift")]))


def eval_coeffs(gamma, beta, running_mean, running_var, eps=1e-5):
    """Eval mode: save [4][C] from the running statistics."""
    rm, rv = _d(running_mean), _d(running_var)
    invstd = 1.0 / torch.sqrt(rv + float(eps))
    g = _d(gamma) if gamma is not None else torch.ones_like(rm)
    b = _d(beta) if beta is not None else torch.zeros_like(rm)
    return torch.stack([rm, invstd, g * invstd, b - rm * g * invstd])


# ------------------------------------------------------------------ forward ----

def pre_act(x, scale, shift):
    """x * scale + shift.  With fp32 inputs the product is exact in float64 and the sum is
    rounded once, so the sign (and a zero) of the exact value is kept."""
    return _d(x) * _d(scale) + _d(shift)


def relu(t):
    """torch.relu: NaN propagates, a negative zero becomes +0."""
    return torch.where(t < 0, torch.zeros_like(t), t)


def apply(x, scale, shift, res=None, rx=None, rscale=None, rshift=None, relu_on=False):
    """y = relu?(x * scale + shift (+ res | + rx * rscale + rshift))."""
    t = pre_act(x, scale, shift)
    if res is not None:
        t = t + _d(res)
    elif rx is not None:
        t = t + pre_act(rx, rscale, rshift)
    return relu(t) if relu_on else t


def mask_of(y):
    """threshold_backward's test: y > 0 (false for 0, -0 and NaN)."""
    return torch.as_tensor(y) > 0


def pack_mask(m, pad=0):
    """A boolean (N, H, W, C) mask as bytes [P][ceil(C/4)]: bit k of byte [p][q] = channel
    4q + k; the bits of channels >= C are `pad` (0 or 1), bits 4-7 are 0."""
    c = m.shape[-1]
    c4 = (c + 3) // 4
    mm = torch.full((m.numel() // c, 4 * c4), bool(pad))
    mm[:, :c] = m.reshape(-1, c)
    w = torch.tensor([1, 2, 4, 8], dtype=torch.int32)
    return (mm.view(-1, c4, 4).to(torch.int32) * w).sum(-1).to(torch.uint8)


def unpack_mask(b, c):
    """The boolean [P][C] mask of the valid channels of mask bytes [P][ceil(C/4)]."""
    b = b.to(torch.int32)
    bits = torch.stack([(b >> k) & 1 for k in range(4)], -1).reshape(b.shape[0], -1)
    return bits[:, :c].bool()


# ----------------------------------------------------------------- backward ----

def masked(dy, m):
    """g = dy where the mask holds, else +0 (m None: no ReLU)."""
    dy = torch.as_tensor(dy)
    return dy if m is None else torch.where(m, dy, torch.zeros((), dtype=dy.dtype))


def xhat(x, mean, invstd):
    return (_d(x) - _d(mean)) * _d(invstd)


def bwd_sums(g, x, mean, invstd):
    """(sum g, sum g * xhat) per channel, and the sums of the absolute terms."""
    c = g.shape[-1]
    gg = _d(g).reshape(-1, c)
    t = gg * xhat(x, mean, invstd).reshape(-1, c)
    return torch.stack([gg.sum(0), t.sum(0)]), torch.stack([gg.abs().sum(0), t.abs().sum(0)])


def param_grads(sums, dgamma_prev=None, dbeta_prev=None):
    """dgamma (+)= sum g * xhat, dbeta (+)= sum g."""
    s = _d(sums).reshape(2, -1)
    dg = s[1] + (_d(dgamma_prev) if dgamma_prev is not None else 0.0)
    db = s[0] + (_d(dbeta_prev) if dbeta_prev is not None else 0.0)
    return dg, db


def bwd_apply(g, x, mean, invstd, gamma, sums, count):
    """dx = gamma * invstd * (g - sum_g / count - xhat * sum_gxhat / count), and the three
    absolute terms |g|, |sum_g / count|, |xhat * sum_gxhat / count| with |gamma * invstd|."""
    s = _d(sums).reshape(2, -1)
    mg, mgx = s[0] / float(count), s[1] / float(count)
    k = _d(invstd) * (_d(gamma) if gamma is not None else 1.0)
    xh = xhat(x, mean, invstd)
    gg = _d(g)
    dx = k * (gg - mg - xh * mgx)
    terms = k.abs() * (gg.abs() + mg.abs() + (xh * mgx).abs())
    return dx, terms

"""Torch restatement of the SSIM loss term (include/vae2_hip.h, vae2_ssim_loss_fwd / _bwd) in a
chosen dtype, for the tests of the kernels: the forward, and the closed-form gradient the
backward kernel implements.  Activations are host NHWC tensors (n, h, w, c)."""
import numpy as np
import torch

C1, C2 = 1e-4, 9e-4  # (0.01 * 1)^2, (0.03 * 1)^2: data_range 1


def window(dtype):
    """The kernels' 11-tap window: vae2.metrics._win's fp32 values, cast."""
    from vae2.metrics import _win
    return _win("cpu", 11, 1.5).to(dtype)


def consts(c1, c2, dtype):
    """The kernels take c1, c2 as fp32 arguments: every precision sees those values."""
    return (torch.tensor(float(np.float32(c1)), dtype=dtype),
            torch.tensor(float(np.float32(c2)), dtype=dtype))


def _filt(x, g):
    """valid separable filtering of (n, h, w, c) along h, then w"""
    k = g.numel()
    h, w = x.shape[1:3]
    y = sum(g[i] * x[:, i:h - k + 1 + i] for i in range(k))
    return sum(g[i] * y[:, :, i:w - k + 1 + i] for i in range(k))


def _filt_t(d, g):
    """the transpose of _filt: (n, h - 10, w - 10, c) back onto (n, h, w, c)"""
    k = g.numel()
    n, ho, wo, c = d.shape
    y = d.new_zeros((n, ho, wo + k - 1, c))
    for i in range(k):
        y[:, :, i:i + wo] += g[i] * d
    out = d.new_zeros((n, ho + k - 1, wo + k - 1, c))
    for i in range(k):
        out[:, i:i + ho] += g[i] * y
    return out


def _affine(p, t, a, b, dtype):
    p, t = p.to(dtype), t.to(dtype)
    if a is None:
        return p, t, None
    a, b = a.to(dtype), b.to(dtype)
    return a * p + b, a * t + b, a


def _maps(u, v, c1, c2, g):
    mu1, mu2 = _filt(u, g), _filt(v, g)
    s1 = _filt(u * u, g) - mu1 * mu1
    s2 = _filt(v * v, g) - mu2 * mu2
    s12 = _filt(u * v, g) - mu1 * mu2
    b1 = mu1 * mu1 + mu2 * mu2 + c1
    b2 = s1 + s2 + c2
    lum = (2 * mu1 * mu2 + c1) / b1
    cs = (2 * s12 + c2) / b2
    return mu1, mu2, b1, b2, lum, cs


def ssim_map(p, t, a=None, b=None, c1=C1, c2=C2, dtype=torch.float64, exact_consts=False):
    """exact_consts: c1, c2 as given (the oracle's fp64 constants), not rounded to fp32."""
    u, v, _ = _affine(p, t, a, b, dtype)
    c1, c2 = (c1, c2) if exact_consts else consts(c1, c2, dtype)
    _, _, _, _, lum, cs = _maps(u, v, c1, c2, window(dtype))
    return lum * cs


def loss(p, t, scale, a=None, b=None, c1=C1, c2=C2, dtype=torch.float64):
    """scale * sum (1 - ssim) over images, channels and valid pixels, in dtype."""
    return scale * (1 - ssim_map(p, t, a, b, c1, c2, dtype)).sum()


def grad_autograd(p, t, scale, a=None, b=None, c1=C1, c2=C2, dtype=torch.float64, gout=1.0):
    """d (gout * loss) / d p by torch.autograd, in dtype."""
    q = p.to(dtype).clone().requires_grad_(True)
    (gout * loss(q, t, scale, a, b, c1, c2, dtype)).backward()
    return q.grad


def grad_closed_form(p, t, scale, a=None, b=None, c1=C1, c2=C2, dtype=torch.float64, gout=1.0):
    """The header's formulas: D11, D12, Dmu on the valid domain, the transposed window, the
    chain rule through mu1, e11, e12."""
    u, v, a = _affine(p, t, a, b, dtype)
    c1, c2 = consts(c1, c2, dtype)
    g = window(dtype)
    mu1, mu2, b1, b2, lum, cs = _maps(u, v, c1, c2, g)
    d11 = -lum * cs / b2
    d12 = 2 * lum / b2
    dmu = cs * 2 * (mu2 - mu1 * lum) / b1 - 2 * mu1 * d11 - mu2 * d12
    inner = _filt_t(dmu, g) + 2 * u * _filt_t(d11, g) + v * _filt_t(d12, g)
    return -scale * gout * (inner if a is None else a * inner)


def make_inputs(shape, kind, seed):
    """The seeded host inputs of the GPU tests: 'near' t ~ N(0,1), p = t + 0.3 N(0,1) (mean
    SSIM about 0.95); 'indep' independent p, t (SSIM about 0); 'const' constant images
    (s1 = s2 = 0)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g)
    if kind == "near":
        p = t + 0.3 * torch.randn(shape, generator=g)
    elif kind == "indep":
        p = torch.randn(shape, generator=g)
    elif kind == "const":
        n, h, w, c = shape
        t = torch.randn((n, 1, 1, c), generator=g).expand(shape).contiguous()
        p = torch.randn((n, 1, 1, c), generator=g).expand(shape).contiguous()
    else:
        raise ValueError(kind)
    return p, t


def coeffs(c):
    """The model's per-channel coefficients: a = STD[c % 3], b = MEAN[c % 3] (fp32)."""
    from vae2.metrics import MEAN, STD
    return (torch.tensor([STD[i % 3] for i in range(c)], dtype=torch.float32),
            torch.tensor([MEAN[i % 3] for i in range(c)], dtype=torch.float32))

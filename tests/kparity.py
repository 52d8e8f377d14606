"""Helpers shared by the kernel-level parity tests that call the C ABI directly
(test_elbo_gpu.py, test_layout_pool_gpu.py, test_bn_gpu.py): sentinel-padded device buffers for
NHWC channel slices and for flat buffers of any dtype, bit comparison, and the three tolerance
rules of the first two files."""
import ctypes

import numpy as np
import torch

DEV = "cuda"
SENT = 777.0  # the sentinel: around every buffer and in the channels outside a slice
GUARD = 8
U = 2.0 ** -24  # unit roundoff of fp32 (half an ulp)
ULP = 2.0 ** -23


def abi():
    from vae2 import ops
    from vae2._lib import call, load
    return call, load(), ops.ptr, ops.stream_ptr()


class Slice:
    """A device copy of the host activation `x` (N, H, W, C) as channels [c0, c0 + C) of a
    pixel-major buffer of pixel stride ps, `offset` floats into an allocation; every other
    element of the allocation (guards, the other channels) holds the sentinel `sent`."""

    def __init__(self, x, ps=None, c0=0, offset=0, sent=SENT):
        from vae2 import ops
        n, h, w, c = x.shape
        self.shape, self.c0 = (n, h, w, c), c0
        self.ps = ps = c if ps is None else ps
        assert c0 + c <= ps
        self.pix = n * h * w
        self.lo = GUARD + offset
        self.sent = sent
        self.raw = torch.full((self.lo + self.pix * ps + GUARD,), sent, device=DEV)
        self.body = self.raw[self.lo:self.lo + self.pix * ps].view(n, h, w, ps)
        self.view = self.body[..., c0:c0 + c]
        self.view.copy_(x)
        self.ptr = ctypes.c_void_p(self.body.data_ptr() + 4 * c0)
        self.act = ops.Act(n, h, w, c, ps)
        self.ref = ctypes.byref(self.act)

    def read(self):
        return self.view.cpu().contiguous()

    def intact(self):
        """Nothing outside the slice was written."""
        r = self.raw.cpu()
        body = r[self.lo:self.lo + self.pix * self.ps].view(self.pix, self.ps)
        c1 = self.c0 + self.shape[3]
        outside = torch.cat([r[:self.lo], r[self.lo + self.pix * self.ps:],
                             body[:, :self.c0].reshape(-1), body[:, c1:].reshape(-1)])
        return bool((outside == self.sent).all())


class Guarded:
    """A device copy of a host tensor of any dtype (float partial rows, double sums, mask
    bytes, an int64 counter), flattened, between GUARD sentinel elements of that dtype."""

    def __init__(self, t, sent=None):
        t = t.contiguous().view(-1)
        self.sent = sent if sent is not None else (SENT if t.dtype.is_floating_point else 0x5A)
        self.n = t.numel()
        self.raw = torch.full((self.n + 2 * GUARD,), self.sent, dtype=t.dtype, device=DEV)
        self.view = self.raw[GUARD:GUARD + self.n]
        self.view.copy_(t)
        self.ptr = ctypes.c_void_p(self.view.data_ptr())
        self.addr = self.view.data_ptr()

    def read(self):
        return self.view.cpu()

    def intact(self):
        r = self.raw.cpu()
        return bool((r[:GUARD] == self.sent).all()) and bool((r[GUARD + self.n:] == self.sent).all())


def flat(x, offset=0):
    """A dense host vector as the (1, 1, n, 1) activation the flat loss paths use."""
    return Slice(x.reshape(1, 1, -1, 1), offset=offset)


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def scalar(fill=float("nan")):
    """A device scalar inside sentinels, pre-filled."""
    return Slice(torch.full((1, 1, 1, 1), fill))


def check_sum(what, got, want64, abs_terms, k, extra=0.0):
    """A sum: |got - want64| <= k * 2^-24 * sum|terms| + 2^-24 * |want64| (+ extra)."""
    got, want64 = float(got), float(want64)
    bound = k * U * float(abs_terms) + U * abs(want64) + extra
    err = abs(got - want64)
    print(f"{what}: got={got!r} want={want64!r} err={err:.3e} bound={bound:.3e} (K={k})")
    assert np.isfinite(got) and err <= bound, (what, got, want64, err, bound)


def check_sums(what, got, want64, abs_terms, k):
    """check_sum element-wise over a tensor of sums; prints the tightest element."""
    got, want64, abs_terms = got.double(), want64.double(), abs_terms.double()
    bound = k * U * abs_terms + U * want64.abs()
    err = (got - want64).abs()
    i = int((err - bound).argmax())
    print(f"{what}: worst element got={float(got.reshape(-1)[i])!r} "
          f"want={float(want64.reshape(-1)[i])!r} err={float(err.reshape(-1)[i]):.3e} "
          f"bound={float(bound.reshape(-1)[i]):.3e} (K={k}); max err={float(err.max()):.3e}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), what


def check_ew(what, got, x32, x64):
    """An element-wise fp32 result: err(gpu) <= 2 * err(cpu_fp32) + 2^-23 * max|x64|."""
    finite = torch.isfinite(x64)
    assert torch.equal(torch.isfinite(got), finite), what
    assert torch.equal(got[~finite].double().nan_to_num(1e300, 2e300, -2e300),
                       x64[~finite].nan_to_num(1e300, 2e300, -2e300)), what
    g, a, b = got[finite].double(), x32[finite].double(), x64[finite]
    e_gpu = float((g - b).abs().max()) if g.numel() else 0.0
    e_cpu = float((a - b).abs().max()) if g.numel() else 0.0
    bound = 2.0 * e_cpu + ULP * (float(b.abs().max()) if g.numel() else 0.0)
    print(f"{what}: err(gpu)={e_gpu:.3e} err(cpu_fp32)={e_cpu:.3e} bound={bound:.3e}")
    assert e_gpu <= bound, (what, e_gpu, e_cpu, bound)


def check_bits(what, got, want):
    ok = same_bits(got, want)
    nd = int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum()) \
        if got.shape == want.shape else -1
    print(f"{what}: bit-exact, {nd} of {want.numel()} words differ")
    assert ok, (what, nd)

"""Kernel-level parity of the layout and pooling ops: vae2_copy_act, vae2_nchw_to_nhwc /
vae2_nhwc_to_nchw, vae2_codemap_tile_fwd/_bwd, vae2_global_avgpool_fwd/_bwd,
vae2_weighted_avgpool_fwd/_bwd and vae2_relu_bwd / vae2_relu_bwd_dual (scalar and channel-quad
kernels), called through the C ABI on sentinel-padded device buffers.  Truth is computed on
the CPU in fp64 from the same fp32 inputs.

Tolerance rules (kparity.py), none tuned from the kernels' output:

* Bit-exact ops are compared bit for bit with torch fp32 evaluating the same expression:
  pure moves and masks (copy, layout conversion, tile forward, ReLU backward with beta2 0)
  and the single-rounding product of the global-avgpool backward with beta 0,
  float32(1 / float32(HW)) * dy.
* Spatial sums (tile backward, both pool forwards) satisfy
  |got - want64| <= K * 2^-24 * sum|terms_i| + 2^-24 * |want64|, K the longest fp32 add chain
  of spatial_partials_kernel + spatial_finish_kernel: a block sums ppb pixels of one chunk
  with R = 256 / C rows in flight, so a thread adds ceil(ppb / R) terms, thread c adds the R
  row sums, and the finish kernel adds the chunks:  K = ceil(ppb / R) + R + chunks.  With
  C > 256 a thread walks all ppb pixels of its channel (R = 1 in the formula, one add to
  spare).  chunks0 = min(256, ceil(HW / 128)), ppb = ceil(HW / chunks0), chunks =
  ceil(HW / ppb): the tables below carry them per (H, W) and R per C, and the tests check
  N * chunks * C against vae2_spatial_ws_size.  The final product with scale (or the add onto
  the accumulated value) is the 2^-24 * |want64| term; want64 uses the fp32 value of scale.
  K counts the adds; the two products inside a weighted term, x * (wr * wc), are not counted,
  so for the weighted pool the bound is the chain's first-order worst case (kept as it is).
* Other element-wise fp32 results (the weighted pool backward, anything with beta != 0, where
  the compiler may contract to an fma):  err(gpu) <= 2 * err(cpu_fp32) + 2^-23 * max|x64|.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from kparity import DEV, Slice, abi, check_bits, check_ew, check_sums, flat, same_bits

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------- copy_act ----

# C -> ((ps, c0) of the source, of the destination)
COPY_CASES = {3: ((27, 6), (12, 5)), 1: ((3, 1), (4, 2)), 18: ((20, 1), (21, 2)),
              257: ((259, 1), (260, 2))}


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("c", list(COPY_CASES))
def test_copy_act(c, beta):
    call, lib, ptr, s = abi()
    xl, yl = COPY_CASES[c]
    x = _rand((2, 5, 7, c), 100 + c)
    x.view(-1)[0], x.view(-1)[1 % x.numel()] = -0.0, NAN  # moved as they are
    prev = _rand(x.shape, 101) if beta else torch.full(x.shape, NAN)
    X, Y = Slice(x, *xl), Slice(prev, *yl)
    call("vae2_copy_act", X.ptr, X.ref, Y.ptr, Y.ref, float(beta), s)
    torch.cuda.synchronize()
    assert X.intact() and Y.intact() and same_bits(X.read(), x)
    if beta == 0:
        check_bits(f"copy_act C={c}", Y.read(), x)
    else:
        ok = ~torch.isnan(x)
        check_ew(f"copy_act C={c} beta=1", Y.read()[ok], (x + prev)[ok],
                 (x.double() + prev.double())[ok])
        assert bool(torch.isnan(Y.read()[~ok]).all())


# ------------------------------------------------------- layout conversion ----

LAYOUT_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 27, 4, 6), (2, 20, 1, 9)]  # (N, C, H, W)


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("shape", LAYOUT_SHAPES)
def test_nchw_to_nhwc_and_back(shape, beta):
    call, lib, ptr, s = abi()
    n, c, h, w = shape
    x = _rand(shape, 200 + c)  # NCHW
    x.view(-1)[0] = -0.0
    want = x.permute(0, 2, 3, 1).contiguous()
    prev = _rand(want.shape, 201) if beta else torch.full(want.shape, NAN)
    X = flat(x)
    Y = Slice(prev, c + 3, 1)  # the NHWC side: a slice of a wider buffer
    call("vae2_nchw_to_nhwc", X.ptr, Y.ptr, Y.ref, float(beta), s)
    torch.cuda.synchronize()
    assert X.intact() and Y.intact() and same_bits(X.read().view(-1), x.view(-1))
    if beta == 0:
        check_bits(f"nchw_to_nhwc {shape}", Y.read(), want)
    else:
        check_ew(f"nchw_to_nhwc {shape} beta=1", Y.read(), want + prev,
                 want.double() + prev.double())
    # back from the slice into a dense NCHW array
    src = Slice(want, c + 3, 1)
    prev2 = _rand(shape, 202) if beta else torch.full(shape, NAN)
    Z = flat(prev2)
    call("vae2_nhwc_to_nchw", src.ptr, src.ref, Z.ptr, float(beta), s)
    torch.cuda.synchronize()
    assert src.intact() and Z.intact() and same_bits(src.read(), want)
    got = Z.read().view(shape)
    if beta == 0:
        check_bits(f"nhwc_to_nchw {shape}: the round trip", got, x)
    else:
        check_ew(f"nhwc_to_nchw {shape} beta=1", got, x + prev2, x.double() + prev2.double())


# ------------------------------------------- code-map tile and the pools ----

# (H, W) -> (chunks, ppb):  chunks0 = min(256, ceil(HW / 128)), ppb = ceil(HW / chunks0),
#                           chunks = ceil(HW / ppb)
SPATIAL = {
    (1, 1): (1, 1),          # HW 1: one chunk of 1 pixel
    (1, 127): (1, 127),      # HW 127: one chunk, one short of the chunk size
    (8, 16): (1, 128),       # HW 128: exactly one chunk
    (3, 43): (2, 65),        # HW 129: ceil(129 / 128) = 2 chunks of ceil(129 / 2) = 65 (65 + 64)
    (40, 2): (1, 80),        # HW 80, W = 2: with R > 2 rows in flight the column index wraps
    (128, 256): (256, 128),  # HW 32768 = 256 * 128: the chunk cap reached exactly
    (129, 256): (256, 129),  # HW 33024: 258 chunks capped to 256 of ceil(33024 / 256) = 129
}
# C -> R = 256 / C rows in flight (1 for C > 256: the per-channel loop)
ROWS = {1: 256, 3: 85, 100: 2, 256: 1, 257: 1, 300: 1}
SMALL_HW = [(1, 1), (1, 127), (8, 16), (3, 43), (40, 2)]
SPATIAL_CASES = [(2, c, hw) for c in ROWS for hw in SMALL_HW] + \
    [(1, c, hw) for c in (3, 300) for hw in ((128, 256), (129, 256))]
IDS = [f"n{n}-c{c}-{hw[0]}x{hw[1]}" for n, c, hw in SPATIAL_CASES]


def _sum_k(c, hw):
    """K = ceil(ppb / R) + R + chunks of the case."""
    chunks, ppb = SPATIAL[hw]
    r = ROWS[c]
    assert r == max(1, 256 // c)
    HW = hw[0] * hw[1]
    chunks0 = min(256, -(-HW // 128))
    assert ppb == -(-HW // chunks0) and chunks == -(-HW // ppb)
    return -(-ppb // r) + r + chunks, chunks


@functools.lru_cache(maxsize=4)
def _map(n, c, hw):
    """The (N, H, W, C) input of a case and its fp64 copy."""
    x = _rand((n, hw[0], hw[1], c), 300 + c + hw[0])
    return x, x.double()


def _weights(hw, seed):
    """Random positive row / column weights in one device buffer, wr then wc, followed by
    max(H, W) more floats so that either vector can be indexed by the other's extent."""
    h, w = hw
    g = torch.Generator().manual_seed(seed)
    wr = 0.25 + torch.rand(h, generator=g)
    wc = 0.25 + torch.rand(w, generator=g)
    buf = torch.full((h + w + max(h, w),), 777.0, device=DEV)
    buf[:h], buf[h:h + w] = wr.to(DEV), wc.to(DEV)
    return wr, wc, buf, ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 4 * h)


def _workspace(lib, X, n, c, hw):
    """Exactly vae2_spatial_ws_size floats, NaN-filled, a sentinel after them."""
    k, chunks = _sum_k(c, hw)
    wsz = int(lib.vae2_spatial_ws_size(X.ref))
    assert wsz == n * chunks * c
    return flat(torch.full((wsz,), NAN)), wsz, k


@pytest.mark.parametrize("case", SPATIAL_CASES, ids=IDS)
def test_codemap_tile(case):
    call, lib, ptr, s = abi()
    n, c, hw = case
    h, w = hw
    # forward: y[n, :, :, c] = v[n, c], a pure move; v's stride and y's are wider than C
    v = _rand((n, 1, 1, c), 400 + c)
    v.view(-1)[0] = -0.0
    V = Slice(v, c + 2, 1)
    Y = Slice(torch.full((n, h, w, c), NAN), c + 3, 2)
    call("vae2_codemap_tile_fwd", V.ptr, V.ps, Y.ptr, Y.ref, s)
    torch.cuda.synchronize()
    assert V.intact() and Y.intact() and same_bits(V.read(), v)
    check_bits(f"tile_fwd {IDS[SPATIAL_CASES.index(case)]}", Y.read(),
               v.expand(n, h, w, c).contiguous())
    # backward: dv[n, c] (+)= sum over h, w of dy
    dy, dy64 = _map(n, c, hw)
    want = dy64.sum((1, 2)).view(n, 1, 1, c)
    terms = dy64.abs().sum((1, 2)).view(n, 1, 1, c)
    for acc in (0, 1):
        prev = _rand((n, 1, 1, c), 401) if acc else torch.full((n, 1, 1, c), NAN)
        DY, DV = Slice(dy, c + 3, 2), Slice(prev, c + 2, 1)
        ws, wsz, k = _workspace(lib, DY, n, c, hw)
        call("vae2_codemap_tile_bwd", DY.ptr, DY.ref, DV.ptr, DV.ps, acc, ws.ptr, wsz, s)
        torch.cuda.synchronize()
        assert DY.intact() and DV.intact() and ws.intact() and same_bits(DY.read(), dy)
        assert not torch.isnan(ws.read()).any()  # every slot the finish pass reads was written
        check_sums(f"tile_bwd {IDS[SPATIAL_CASES.index(case)]} accumulate={acc}", DV.read(),
                   want + prev.double() if acc else want, terms, k)


@pytest.mark.parametrize("case", SPATIAL_CASES, ids=IDS)
def test_global_avgpool(case):
    call, lib, ptr, s = abi()
    n, c, hw = case
    h, w = hw
    tag = IDS[SPATIAL_CASES.index(case)]
    scale = np.float32(1.0) / np.float32(h * w)  # the launcher's 1.f / (float)(h * w)
    x, x64 = _map(n, c, hw)
    X, Y = Slice(x, c + 3, 2), Slice(torch.full((n, 1, 1, c), NAN), c + 5, 1)
    ws, wsz, k = _workspace(lib, X, n, c, hw)
    call("vae2_global_avgpool_fwd", X.ptr, X.ref, Y.ptr, Y.ref, ws.ptr, wsz, s)
    torch.cuda.synchronize()
    assert X.intact() and Y.intact() and ws.intact() and same_bits(X.read(), x)
    assert not torch.isnan(ws.read()).any()
    check_sums(f"global_avgpool_fwd {tag}", Y.read(), float(scale) * x64.sum((1, 2)).view(n, 1, 1, c),
               float(scale) * x64.abs().sum((1, 2)).view(n, 1, 1, c), k)
    # backward: dx = (1 / HW) * dy[n, c] broadcast, one rounding
    dy = _rand((n, 1, 1, c), 500 + c)
    want32 = (float(scale) * dy).expand(n, h, w, c).contiguous()
    for beta in (0, 1):
        prev = _rand((n, h, w, c), 501) if beta else torch.full((n, h, w, c), NAN)
        DY, DX = Slice(dy, c + 5, 1), Slice(prev, c + 3, 2)
        call("vae2_global_avgpool_bwd", DY.ptr, DY.ref, DX.ptr, DX.ref, float(beta), s)
        torch.cuda.synchronize()
        assert DY.intact() and DX.intact() and same_bits(DY.read(), dy)
        if beta == 0:
            check_bits(f"global_avgpool_bwd {tag}", DX.read(), want32)
        else:
            check_ew(f"global_avgpool_bwd {tag} beta=1", DX.read(), want32 + prev,
                     float(scale) * dy.double() + prev.double())


@pytest.mark.parametrize("case", SPATIAL_CASES, ids=IDS)
def test_weighted_avgpool(case):
    call, lib, ptr, s = abi()
    n, c, hw = case
    h, w = hw
    tag = IDS[SPATIAL_CASES.index(case)]
    scale = float(np.float32(1.0 / (3 * h * w)))
    wr, wc, wbuf, wrp, wcp = _weights(hw, 600 + h)
    w2_32 = (wr.view(h, 1) * wc.view(1, w)).view(1, h, w, 1)  # wr[iy] * wc[ix], rounded
    w2_64 = (wr.double().view(h, 1) * wc.double().view(1, w)).view(1, h, w, 1)
    x, x64 = _map(n, c, hw)
    X, Y = Slice(x, c + 3, 2), Slice(torch.full((n, 1, 1, c), NAN), c + 5, 1)
    ws, wsz, k = _workspace(lib, X, n, c, hw)
    call("vae2_weighted_avgpool_fwd", X.ptr, X.ref, wrp, wcp, scale, Y.ptr, Y.ref, ws.ptr, wsz, s)
    torch.cuda.synchronize()
    assert X.intact() and Y.intact() and ws.intact() and same_bits(X.read(), x)
    assert not torch.isnan(ws.read()).any()
    check_sums(f"weighted_avgpool_fwd {tag}", Y.read(),
               scale * (x64 * w2_64).sum((1, 2)).view(n, 1, 1, c),
               scale * (x64 * w2_64).abs().sum((1, 2)).view(n, 1, 1, c), k)
    # backward: dx = (scale * dy[n, c]) * (wr[iy] * wc[ix]) (+ beta * dx)
    dy = _rand((n, 1, 1, c), 601 + c)
    v32 = (scale * dy) * w2_32
    v64 = scale * dy.double() * w2_64
    for beta in (0, 1):
        prev = _rand((n, h, w, c), 602) if beta else torch.full((n, h, w, c), NAN)
        DY, DX = Slice(dy, c + 5, 1), Slice(prev, c + 3, 2)
        call("vae2_weighted_avgpool_bwd", DY.ptr, DY.ref, wrp, wcp, scale, DX.ptr, DX.ref,
             float(beta), s)
        torch.cuda.synchronize()
        assert DY.intact() and DX.intact() and same_bits(DY.read(), dy)
        check_ew(f"weighted_avgpool_bwd {tag} beta={beta}", DX.read(),
                 v32 + prev if beta else v32, v64 + prev.double() if beta else v64)
    assert bool((wbuf[h + w:] == 777.0).all()) and torch.equal(wbuf[:h].cpu(), wr)


# ------------------------------------------------------------ ReLU backward ----

RELU_C = [1, 3, 18, 36]
DENORM = float(np.float32(1e-45))  # the smallest denormal
# the padding channels of y pass the gradient and those of dy differ from g's and g2's
# sentinel, so a store past channel C changes g and g2 whatever beta2 is
Y_SENT, DY_SENT = 555.0, 333.0


def _relu_inputs(c):
    dy = _rand((2, 5, 7, c), 700 + c)
    y = _rand((2, 5, 7, c), 701 + c)
    yf, df = y.view(-1), dy.view(-1)
    edge = [0.0, -0.0, DENORM, -DENORM]  # only the positive denormal passes the gradient
    for i, v in enumerate(edge):
        yf[(3 + 11 * i) % yf.numel()] = v
    df[1 % df.numel()] = -0.0
    return dy, y


def _ps_of(c, wide):
    return (c + 3) // 4 * 4 + 4 if wide else c


def _kernels(lib):
    buf = ctypes.create_string_buffer(4096)
    lib.vae2_kernel_log_read(buf, 4096)
    return buf.value.decode().split(";")


@pytest.mark.parametrize("wide", [False, True], ids=["ps=C", "ps=C4+4"])
@pytest.mark.parametrize("c", RELU_C)
def test_relu_bwd(c, wide):
    call, lib, ptr, s = abi()
    ps = _ps_of(c, wide)
    dy, y = _relu_inputs(c)
    DY, Y = Slice(dy, ps, sent=DY_SENT), Slice(y, ps, sent=Y_SENT)
    G = Slice(torch.full(dy.shape, NAN), ps)
    call("vae2_relu_bwd", DY.ptr, DY.ref, Y.ptr, Y.ref, G.ptr, G.ref, s)
    torch.cuda.synchronize()
    assert DY.intact() and Y.intact() and G.intact()
    want = torch.where(y > 0, dy, torch.zeros(()))
    assert int((y > 0).sum()) not in (0, y.numel())
    check_bits(f"relu_bwd C={c} ps={ps}", G.read(), want)


def _run_dual(c, ps, beta2, offset, scalar_kernel):
    """(g, g2, kernel name) of one vae2_relu_bwd_dual call."""
    call, lib, ptr, s = abi()
    dy, y = _relu_inputs(c)
    prev = _rand(dy.shape, 702) if beta2 else torch.full(dy.shape, NAN)
    DY = Slice(dy, ps, offset=offset, sent=DY_SENT)
    Y = Slice(y, ps, offset=offset, sent=Y_SENT)
    G, G2 = Slice(torch.full(dy.shape, NAN), ps, offset=offset), Slice(prev, ps, offset=offset)
    old = lib.vae2_heads_set_algo(0)
    try:
        lib.vae2_heads_set_algo(old | 128 if scalar_kernel else old & ~128)
        lib.vae2_kernel_log(1)
        call("vae2_relu_bwd_dual", DY.ptr, DY.ref, Y.ptr, Y.ref, G.ptr, G.ref, G2.ptr, G2.ref,
             float(beta2), s)
        names = _kernels(lib)
    finally:
        lib.vae2_kernel_log(0)
        lib.vae2_heads_set_algo(old)
    torch.cuda.synchronize()
    # with C % 4 != 0 the channels [C, ps) of g and g2 keep their sentinels
    assert DY.intact() and Y.intact() and G.intact() and G2.intact()
    assert same_bits(DY.read(), dy) and same_bits(Y.read(), y)
    assert len(names) == 1
    return G.read(), G2.read(), names[0], (dy, y, prev)


@pytest.mark.parametrize("beta2", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("wide", [False, True], ids=["ps=C", "ps=C4+4"])
@pytest.mark.parametrize("c", RELU_C)
def test_relu_bwd_dual(c, wide, beta2):
    ps = _ps_of(c, wide)
    quad_ok = ps % 4 == 0  # C = 36 at ps = C as well
    g_q, g2_q, k_q, (dy, y, prev) = _run_dual(c, ps, beta2, 0, scalar_kernel=False)
    g_s, g2_s, k_s, _ = _run_dual(c, ps, beta2, 0, scalar_kernel=True)
    g_o, g2_o, k_o, _ = _run_dual(c, ps, beta2, 1, scalar_kernel=False)  # unaligned pointers
    print(f"relu_bwd_dual C={c} ps={ps} beta2={beta2}: kernels {k_q} / {k_s} / {k_o}")
    # ps % 4 != 0 or a pointer offset by one float falls back to the scalar kernel
    assert k_q == ("relu_bwd_dual_q_kernel" if quad_ok else "relu_bwd_dual_kernel")
    assert k_s == "relu_bwd_dual_kernel" and k_o == "relu_bwd_dual_kernel"
    want = torch.where(y > 0, dy, torch.zeros(()))
    for tag, g, g2 in (("quad", g_q, g2_q), ("scalar", g_s, g2_s), ("offset", g_o, g2_o)):
        check_bits(f"relu_bwd_dual g {tag} C={c} ps={ps}", g, want)
        if beta2 == 0:
            check_bits(f"relu_bwd_dual g2 {tag} C={c} ps={ps}", g2, want)
        else:
            check_ew(f"relu_bwd_dual g2 {tag} C={c} ps={ps} beta2={beta2}", g2,
                     want + beta2 * prev, want.double() + beta2 * prev.double())
    # the two kernels agree bit for bit
    assert same_bits(g2_q, g2_s) and same_bits(g2_q, g2_o)

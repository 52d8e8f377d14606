// Weight gradients of the convolutions: wgrad_kernel (gather form, every geometry),
// wgrad3_kernel (LDS-tiled, 3x3 / stride 1), the fixed-order slab reductions with their
// deferral queue, and the weight-gradient C ABI.
#include <algorithm>
#include <mutex>
#include <vector>

#include "conv.h"

namespace vae2 {

// ------------------------------------------------------------ wgrad ----
// dW[co][(tap, ci4)] = sum_p dY[p][co] * X[src(p, tap)][ci].  MFMA m = co, n = column,
// k = pixel: lane group g takes pixels 4g..4g+3 of each 16-pixel chunk.
// Workgroup = 4 waves sharing one (co, column) tile; wave w takes chunks w, w+4, ...
// of the workgroup's pixel range, the 4 partial tiles are summed in LDS (fixed
// order) and written as one fp32 slab part[split][cout][ncol4].
struct WGrad {
  const float* x;
  int x_ps, cin, cin4, x_h, x_w;
  const float* dy;
  int dy_ps, cout, o_n, o_h, o_w;
  int k, stride, pad;
  int P, px_split;
  uint32_t x_bytes, dy_bytes;
  float* part;
  FastDiv ohw_div, ow_div, cin4_div;
};

// V4 (16-byte aligned NHWC operands): lane (g, 4Q + k) loads ONE 16-byte channel quad
// of pixel 4g + k per operand tile -- dY[px][co 4Q..4Q+3], X[src(px)][ci 4Q..4Q+3] -- and
// a 4x4 transpose inside its lane quad (quad_transpose, DPP) turns those into the MFMA
// fragments (4 pixels of one co / ci), instead of four 4-byte loads with four pixel
// address computations per operand tile.
template <int TM, int TN, bool BF = false, bool V4 = false>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(WGrad p) {
  extern __shared__ __attribute__((aligned(16))) float wred[];  // [3][TM*TN*4][64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, r = lane & 15;
  const int ncol4 = p.k * p.k * p.cin4;
  const int co0 = blockIdx.y * 16 * TM;
  const int col0 = blockIdx.x * 16 * TN;
  const int pbeg = blockIdx.z * p.px_split;
  const int pend = min(pbeg + p.px_split, p.P);
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t dr = make_rsrc(p.dy, p.dy_bytes);

  int aco[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int co = co0 + i * 16 + r;
    aco[i] = co < p.cout ? co : -1;
  }
  int bkh[TN], bkw[TN], boff[TN];
  bool bok[TN];
  const int kq = r & 3;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = col0 + j * 16 + (V4 ? 4 * (r >> 2) : r);  // (V4: the lane's channel quad)
    const int t = (int)p.cin4_div.div((uint32_t)col);
    const int ci = col - t * p.cin4;
    bkh[j] = t / p.k;
    bkw[j] = t - bkh[j] * p.k;
    bok[j] = col < ncol4 && ci < p.cin;
    boff[j] = (bkh[j] * p.x_w + bkw[j]) * p.x_ps + ci;
  }
  f4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  const int ohw = p.o_h * p.o_w;
  // chunk loads (pixels past pend load 0), double-buffered in registers: the next
  // chunk's loads are in flight across this chunk's MFMAs
  auto load = [&](int pc, f4* fa, f4* fb) {
    if constexpr (V4) {
      const int pix = pc + 4 * g + kq;
      const bool pv = pix < pend;
      const int pp = pv ? pix : pbeg;
      const int n = (int)p.ohw_div.div((uint32_t)pp);
      const int rem = pp - n * ohw;
      const int oh = (int)p.ow_div.div((uint32_t)rem);
      const int ow = rem - oh * p.o_w;
      const uint32_t drow = (uint32_t)(pp * p.dy_ps);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int co = co0 + i * 16 + 4 * (r >> 2);
        fa[i] = load4(dr, (pv && co < p.cout) ? (drow + co) * 4u : kOOB);
      }
      const int ih0 = oh * p.stride - p.pad, iw0 = ow * p.stride - p.pad;
      const int xc = ((n * p.x_h + ih0) * p.x_w + iw0) * p.x_ps;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int ih = ih0 + bkh[j], iw = iw0 + bkw[j];
        const bool ok = pv && bok[j] && (unsigned)ih < (unsigned)p.x_h &&
                        (unsigned)iw < (unsigned)p.x_w;
        fb[j] = load4(xr, ok ? (uint32_t)(xc + boff[j]) * 4u : kOOB);
      }
      return;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int pix = pc + 4 * g + s;
      const bool pv = pix < pend;
      const int pp = pv ? pix : pbeg;
      const int n = (int)p.ohw_div.div((uint32_t)pp);
      const int rem = pp - n * ohw;
      const int oh = (int)p.ow_div.div((uint32_t)rem);
      const int ow = rem - oh * p.o_w;
      const uint32_t drow = (uint32_t)(pp * p.dy_ps);
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[i][s] = load1(dr, (pv && aco[i] >= 0) ? (drow + aco[i]) * 4u : kOOB);
      const int ih0 = oh * p.stride - p.pad, iw0 = ow * p.stride - p.pad;
      const int xc = ((n * p.x_h + ih0) * p.x_w + iw0) * p.x_ps;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int ih = ih0 + bkh[j], iw = iw0 + bkw[j];
        const bool ok = pv && bok[j] && (unsigned)ih < (unsigned)p.x_h &&
                        (unsigned)iw < (unsigned)p.x_w;
        fb[j][s] = load1(xr, ok ? (uint32_t)(xc + boff[j]) * 4u : kOOB);
      }
    }
  };
  auto quads = [&](f4* fa, f4* fb) {  // V4: quad loads -> fragments (after they landed)
    if constexpr (V4) {
#pragma unroll
      for (int i = 0; i < TM; ++i) quad_transpose(fa[i], kq);
#pragma unroll
      for (int j = 0; j < TN; ++j) quad_transpose(fb[j], kq);
    }
  };
  auto mma = [&](f4* fa, f4* fb) {
    quads(fa, fb);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);
  };
  {
    f4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
    int pc = pbeg + 16 * wave;
    if (!BF) {
      if (pc < pend) load(pc, fa0, fb0);
      for (; pc < pend; pc += 128) {
        load(pc + 64, fa1, fb1);
        mma(fa0, fb0);
        load(pc + 128, fa0, fb0);
        mma(fa1, fb1);
      }
    } else if (pc < pend) {  // bf16 operands: one 16x16x32 MFMA per chunk pair
      load(pc, fa0, fb0);
      load(pc + 64, fa1, fb1);
      for (; pc < pend; pc += 128) {
        bf16x8 A[TM], B[TN];
        quads(fa0, fb0);
        quads(fa1, fb1);
#pragma unroll
        for (int i = 0; i < TM; ++i) A[i] = pack_bf16(fa0[i], fa1[i]);
#pragma unroll
        for (int j = 0; j < TN; ++j) B[j] = pack_bf16(fb0[j], fb1[j]);
        load(pc + 128, fa0, fb0);
        load(pc + 192, fa1, fb1);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[i], B[j], acc[i][j], 0, 0, 0);
      }
    }
  }

  // cross-wave reduction in a fixed order: waves 1..3 park their tiles in LDS
  constexpr int NV = TM * TN * 4;
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          wred[((wave - 1) * NV + (i * TN + j) * 4 + e) * 64 + lane] = acc[i][j][e];
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int w = 0; w < 3; ++w)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc[i][j][e] += wred[(w * NV + (i * TN + j) * 4 + e) * 64 + lane];

  float* out = p.part + (int64_t)blockIdx.z * p.cout * ncol4;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int co = co0 + i * 16 + g * 4 + e;
      if (co >= p.cout) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = col0 + j * 16 + r;
        if (col < ncol4) out[(int64_t)co * ncol4 + col] = acc[i][j][e];
      }
    }
}

// --------------------------------------------------- direct 3x3 wgrad (LDS) ----
// dW of 3x3 / stride-1 / pad-1 convs.  A workgroup owns a (co slab, ci slab) of dW
// and a run of BH x 32 pixel tiles; per tile it stages dY (transposed: [co][px]) and
// the X halo tile (transposed: [ci][halo px]) in LDS once, then every wave sweeps all
// the tile's pixels (MFMA k) for its own TN column tiles (columns = (tap, ci) of the
// slab), so no cross-wave reduction is needed.  Partial slabs part[split][co][(t,ci)]
// are summed by wgrad_reduce_kernel in a fixed order (deterministic).
struct WGrad3 {
  const float* x;
  int x_ps, cin, cin4, h, w;
  const float* dy;
  int dy_ps, cout;
  int tiles_h, tiles_w, ntiles, tiles_per_split;
  int csw, n_ci_slabs;  // channels per ci slab (multiple of 4), slabs
  uint32_t x_bytes, dy_bytes;
  float* part;  // [splits][cout][9*cin4]
  // x is the pre-BN output of a BatchNorm(+ReLU) layer whose normalised activation is
  // never stored (DConv::isave): staging applies relu?(x*scale + shift) to in-image pixels
  const float* isave;
  int irelu;
};

// NR > 0 (fp32 operands, one co slab): cout = 16*TM + NR (the 18 / 36-channel layers)
// -- the last NR output channels are computed on the VALU beside the MFMAs instead of in a
// further 16-row MFMA tile that would be mostly padding: every lane already holds the X
// fragment of its column for 4 pixels (the MFMA B operand), so it adds those pixels'
// dY[co][px] * X products for each remainder co (dY rows staged with the others) and
// the 4 lane groups' sums are combined at the end.  The MFMA work of an 18-channel
// layer halves (32 -> 16 rows), of a 36-channel one drops by 1/3.  With several co slabs
// (72 = 2 x (32 + 4)) each slab is 16*TM + NR channels wide.
// NW = waves per workgroup: 4, or 8 (each wave half the column tiles: twice the waves per
// SIMD for layers whose grid leaves one workgroup per CU)
template <int TM, int TN, int BH, bool PF, int KS, bool BF = false, int NR = 0, int NW = 4>
__global__ __launch_bounds__(64 * NW) void wgrad3_kernel(WGrad3 p) {
  constexpr int NT = 64 * NW;
  constexpr int HALO = KS / 2, TAPS = KS * KS;
  constexpr int LH = BH + KS - 1, LW = 32 + KS - 1, NPX = BH * 32, LPX = LH * LW;
  constexpr int QMAX = KS == 1 ? 16 : 9;  // channel quads per slab
  constexpr int DYS = NPX + 4;  // dY^T row stride (floats)
  constexpr int NRQ = (NR + 3) / 4;        // remainder co quads staged
  constexpr int NQ = 4 * TM + NRQ;         // dY co quads staged per tile
  static_assert(NR == 0 || (!BF && NR <= 4), "remainder shape");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* dyt = sm;                  // [16*TM + 4*NRQ][DYS]
  float* xt = sm + NQ * 4 * DYS;    // [csw + 1][LPX], row csw = zeros
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, r = lane & 15;
  const int cis = blockIdx.y % p.n_ci_slabs, cos = blockIdx.y / p.n_ci_slabs;
  const int co0 = cos * (16 * TM + NR), c0 = cis * p.csw;
  const int csw_real = p.cin4 - c0 < p.csw ? p.cin4 - c0 : p.csw;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t dr = make_rsrc(p.dy, p.dy_bytes);

  int bbase[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = (wave * TN + j) * 16 + r;
    const int t = n / p.csw;
    const int cl = n - t * p.csw;
    const bool ok = t < TAPS && cl < csw_real;
    bbase[j] = ok ? cl * LPX + (t / KS) * LW + (t % KS) : p.csw * LPX;
  }
  for (int i = threadIdx.x; i < LPX; i += NT) xt[p.csw * LPX + i] = 0.f;
  // input BatchNorm: the slab's scale / shift (read after the tile loop's first barrier)
  __shared__ float ibn[2][QMAX * 4];
  if (p.isave && threadIdx.x < QMAX * 4) {
    const int ch = c0 + (int)threadIdx.x < p.cin ? c0 + (int)threadIdx.x : p.cin - 1;
    ibn[0][threadIdx.x] = p.isave[2 * p.cin + ch];
    ibn[1][threadIdx.x] = p.isave[3 * p.cin + ch];
  }
  auto ibn_apply = [&](f4& v, int q) {  // = bn_apply_body's arithmetic
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float t = __builtin_fmaf(v[k], ibn[0][4 * q + k], ibn[1][4 * q + k]);
      v[k] = (p.irelu && t < 0.f) ? 0.f : t;
    }
  };

  f4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  float racc[TN][NR > 0 ? NR : 1];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int q = 0; q < NR; ++q) racc[j][q] = 0.f;

  const int per_img = p.tiles_h * p.tiles_w;
  const int tb = blockIdx.x * p.tiles_per_split;
  const int te = tb + p.tiles_per_split < p.ntiles ? tb + p.tiles_per_split : p.ntiles;
  // Register prefetch: tile t+1's global loads are in flight while tile t computes.
  constexpr int NDY = NPX * NQ;                 // dY items (f4 = 4 co of one pixel)
  constexpr int NI = (NDY + NT - 1) / NT;         // dY items per thread
  constexpr int NX = (LPX * QMAX + NT - 1) / NT;  // X items per thread
  const int xtotal = LPX * (csw_real >> 2);
  f4 pdy[NI], pxx[NX];
  static_assert(NX <= 32, "x item mask");
  uint32_t xok = 0;  // in-image x items of the prefetched tile (input BatchNorm)
  auto fetch = [&](int tile) {
    const int img = tile / per_img;
    const int trem = tile - img * per_img;
    const int th = trem / p.tiles_w;
    const int oh0 = th * BH, ow0 = (trem - th * p.tiles_w) * 32;
    const int ibase = img * p.h;
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      const int i = threadIdx.x + u * NT;
      const int q = i / NPX, px = i - q * NPX;
      const int oh = oh0 + px / 32, ow = ow0 + (px & 31);
      const int co = co0 + 4 * q;
      const bool ok = i < NDY && oh < p.h && ow < p.w && co < p.cout;
      pdy[u] = load4(dr, ok ? (uint32_t)(((ibase + oh) * p.w + ow) * p.dy_ps + co) * 4u : kOOB);
    }
#pragma unroll
    for (int u = 0; u < NX; ++u) {
      const int i = threadIdx.x + u * NT;
      const int q = i / LPX, hp = i - q * LPX;
      const int lr = hp / LW, lc = hp - lr * LW;
      const int ih = oh0 - HALO + lr, iw = ow0 - HALO + lc;
      const int c = c0 + 4 * q;
      const bool ok = i < xtotal && (unsigned)ih < (unsigned)p.h && (unsigned)iw < (unsigned)p.w;
      pxx[u] = load4(xr, ok ? (uint32_t)(((ibase + ih) * p.w + iw) * p.x_ps + c) * 4u : kOOB);
      xok = u == 0 ? (uint32_t)ok : (xok | ((uint32_t)ok << u));
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      const int i = threadIdx.x + u * NT;
      if (NDY % NT != 0 && i >= NDY) break;
      const int q = i / NPX, px = i - q * NPX;
      const int co = co0 + 4 * q;
#pragma unroll
      for (int k = 0; k < 4; ++k) dyt[(4 * q + k) * DYS + px] = co + k < p.cout ? pdy[u][k] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < NX; ++u) {
      const int i = threadIdx.x + u * NT;
      if (i < xtotal) {
        const int q = i / LPX, hp = i - q * LPX;
        const int c = c0 + 4 * q;
        if (p.isave && ((xok >> u) & 1u)) ibn_apply(pxx[u], q);
#pragma unroll
        for (int k = 0; k < 4; ++k) xt[(4 * q + k) * LPX + hp] = c + k < p.cin ? pxx[u][k] : 0.f;
      }
    }
  };
  if (PF && tb < te) fetch(tb);
  for (int tile = tb; tile < te; ++tile) {
    __syncthreads();  // the previous tile's fragment reads are done
    if (PF) {
      store();
    } else {  // lower register footprint: dY at once, X in batches of 4 loads per thread
      const int img = tile / per_img;
      const int trem = tile - img * per_img;
      const int th = trem / p.tiles_w;
      const int oh0 = th * BH, ow0 = (trem - th * p.tiles_w) * 32;
      const int ibase = img * p.h;
      {
        f4 v[NI];
#pragma unroll
        for (int u = 0; u < NI; ++u) {
          const int i = threadIdx.x + u * NT;
          const int q = i / NPX, px = i - q * NPX;
          const int oh = oh0 + px / 32, ow = ow0 + (px & 31);
          const int co = co0 + 4 * q;
          const bool ok = i < NDY && oh < p.h && ow < p.w && co < p.cout;
          v[u] = load4(dr, ok ? (uint32_t)(((ibase + oh) * p.w + ow) * p.dy_ps + co) * 4u : kOOB);
        }
#pragma unroll
        for (int u = 0; u < NI; ++u) {
          const int i = threadIdx.x + u * NT;
          if (NDY % NT != 0 && i >= NDY) break;
          const int q = i / NPX, px = i - q * NPX;
          const int co = co0 + 4 * q;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            dyt[(4 * q + k) * DYS + px] = co + k < p.cout ? v[u][k] : 0.f;
        }
      }
      for (int i0 = threadIdx.x; i0 < xtotal; i0 += 4 * NT) {
        f4 v[4];
        bool okv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * NT;
          const int q = i / LPX, hp = i - q * LPX;
          const int lr = hp / LW, lc = hp - lr * LW;
          const int ih = oh0 - HALO + lr, iw = ow0 - HALO + lc;
          const int c = c0 + 4 * q;
          const bool ok =
              i < xtotal && (unsigned)ih < (unsigned)p.h && (unsigned)iw < (unsigned)p.w;
          okv[u] = ok;
          v[u] = load4(xr, ok ? (uint32_t)(((ibase + ih) * p.w + iw) * p.x_ps + c) * 4u : kOOB);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * NT;
          if (i >= xtotal) break;
          const int q = i / LPX, hp = i - q * LPX;
          const int c = c0 + 4 * q;
          if (p.isave && okv[u]) ibn_apply(v[u], q);
#pragma unroll
          for (int k = 0; k < 4; ++k) xt[(4 * q + k) * LPX + hp] = c + k < p.cin ? v[u][k] : 0.f;
        }
      }
    }
    __syncthreads();
    if (PF && tile + 1 < te) fetch(tile + 1);
    auto frag = [&](int ch, f4* fa, f4* fb) {
      const int px0 = ch * 16 + 4 * g;
      const int poff = (px0 >> 5) * LW + (px0 & 31);
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[i] = *reinterpret_cast<const f4*>(&dyt[(i * 16 + r) * DYS + px0]);
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const float* b = &xt[bbase[j] + poff];
        if (KS == 1) fb[j] = *reinterpret_cast<const f4*>(b);  // 16-byte aligned: no tap shift
        else fb[j] = f4{b[0], b[1], b[2], b[3]};
      }
    };
    if (!BF) {
#pragma unroll 2
      for (int ch = 0; ch < NPX / 16; ++ch) {
        f4 fa[TM], fb[TN];
        frag(ch, fa, fb);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][s2], fb[j][s2], acc[i][j], 0, 0, 0);
        if constexpr (NR > 0) {  // this lane's 4 pixels x its columns, remainder rows
          const int px0 = ch * 16 + 4 * g;
#pragma unroll
          for (int q = 0; q < NR; ++q) {
            const f4 d = *reinterpret_cast<const f4*>(&dyt[(16 * TM + q) * DYS + px0]);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              racc[j][q] = __builtin_fmaf(d[0], fb[j][0], racc[j][q]);
              racc[j][q] = __builtin_fmaf(d[1], fb[j][1], racc[j][q]);
              racc[j][q] = __builtin_fmaf(d[2], fb[j][2], racc[j][q]);
              racc[j][q] = __builtin_fmaf(d[3], fb[j][3], racc[j][q]);
            }
          }
        }
      }
    } else {  // bf16 operands: one 16x16x32 MFMA per pair of 16-pixel chunks
#pragma unroll 2
      for (int ch = 0; ch < NPX / 16; ch += 2) {
        f4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
        frag(ch, fa0, fb0);
        frag(ch + 1, fa1, fb1);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                pack_bf16(fa0[i], fa1[i]), pack_bf16(fb0[j], fb1[j]), acc[i][j], 0, 0, 0);
      }
    }
  }

  const int ncol4 = TAPS * p.cin4;
  float* out = p.part + (int64_t)blockIdx.x * p.cout * ncol4;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = (wave * TN + j) * 16 + r;
    const int t = n / p.csw;
    const int cl = n - t * p.csw;
    if (t >= TAPS || cl >= csw_real) continue;
    const int col = t * p.cin4 + c0 + cl;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = co0 + i * 16 + g * 4 + e;
        if (co < p.cout) out[(int64_t)co * ncol4 + col] = acc[i][j][e];
      }
  }
  if constexpr (NR > 0) {  // the 4 lane groups' pixel sums (fixed order), rows 16*TM + q
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = (wave * TN + j) * 16 + r;
      const int t = n / p.csw;
      const int cl = n - t * p.csw;
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        float v = racc[j][q];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (g == 0 && t < TAPS && cl < csw_real)
          out[(int64_t)(co0 + 16 * TM + q) * ncol4 + t * p.cin4 + c0 + cl] = v;
      }
    }
  }
}

// dw[co][ci][kh][kw] (+)= sum_s part[s][co][(kh*k+kw)*cin4 + ci]
// Block = 32 slab columns x 8 split groups: thread (g, col) sums splits g, g+8, ...
// (unrolled: its loads are independent), the 8 group sums are combined in LDS in a fixed
// order (deterministic).  Small slabs still get ceil(slab/32) blocks and short chains.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part,
                                                           int splits, int cout, int cin,
                                                           int cin4, int k,
                                                           float* __restrict__ dw, int64_t ld,
                                                           int accumulate) {
  __shared__ float red[8][32];
  const int kk = k * k;
  const int ncol4 = kk * cin4;
  const int total = cout * ncol4;  // slab elements
  const int cl = threadIdx.x & 31, sg = threadIdx.x >> 5;
  const int idx = blockIdx.x * 32 + cl;
  float s = 0.f;
  if (idx < total) {
    const float* src = part + idx;
    const int64_t stride = (int64_t)total;
#pragma unroll 8
    for (int sp = sg; sp < splits; sp += 8) s += src[sp * stride];
  }
  red[sg][cl] = s;
  __syncthreads();
  if (sg != 0 || idx >= total) return;
  s = red[0][cl];
#pragma unroll
  for (int j = 1; j < 8; ++j) s += red[j][cl];
  const int co = idx / ncol4;
  const int col = idx - co * ncol4;
  const int t = col / cin4;
  const int ci = col - t * cin4;
  if (ci >= cin) return;
  const int64_t o = (int64_t)co * ld + ci * kk + t;
  dw[o] = accumulate ? dw[o] + s : s;
}

// Deferred reductions (vae2_wgrad_defer / vae2_wgrad_flush): the weight gradients of
// one BatchNorm depth level (the lock-stepped branch convs, a head's branch blocks) share
// one reduce launch; blocks are partitioned between the jobs by prefix.
struct WRJob {
  const float* part;
  float* dw;
  int64_t ld;
  int splits, cout, cin, cin4, k, accumulate, blk0;
};
constexpr int kWrMaxJobs = 32;  // (kernel argument: 32 x 56 B)
struct WRMulti {
  WRJob j[kWrMaxJobs];
  int n;
};

__global__ __launch_bounds__(256) void wgrad_reduce_multi_kernel(WRMulti m) {
  int i = 0;
  while (i + 1 < m.n && (int)blockIdx.x >= m.j[i + 1].blk0) ++i;
  const WRJob& J = m.j[i];
  __shared__ float red[8][32];
  const int kk = J.k * J.k;
  const int ncol4 = kk * J.cin4;
  const int total = J.cout * ncol4;
  const int cl = threadIdx.x & 31, sg = threadIdx.x >> 5;
  const int idx = ((int)blockIdx.x - J.blk0) * 32 + cl;
  float s = 0.f;
  if (idx < total) {
    const float* src = J.part + idx;
    const int64_t stride = (int64_t)total;
#pragma unroll 8
    for (int sp = sg; sp < J.splits; sp += 8) s += src[sp * stride];
  }
  red[sg][cl] = s;
  __syncthreads();
  if (sg != 0 || idx >= total) return;
  s = red[0][cl];
#pragma unroll
  for (int q = 1; q < 8; ++q) s += red[q][cl];
  const int co = idx / ncol4;
  const int col = idx - co * ncol4;
  const int t = col / J.cin4;
  const int ci = col - t * J.cin4;
  if (ci >= J.cin) return;
  const int64_t o = (int64_t)co * J.ld + ci * kk + t;
  J.dw[o] = J.accumulate ? J.dw[o] + s : s;
}


struct WRQueued {
  WRJob job;
  hipStream_t stream;
};
// the deferral switch is per thread (set inside the calling thread's backward functions);
// the queue is shared, so the end-of-backward flush may run on any thread
static thread_local bool g_wr_defer = false;
static std::vector<WRQueued> g_wr_queue;
static std::mutex g_wr_mu;

struct WTile {
  int tm, tn, gx, gy, splits, px_split;
};

static WTile pick_wtile(int64_t P, int cout, int ncol4) {
  WTile t;
  int mt = (cout + 15) / 16;
  t.tm = mt <= 4 ? mt : 4;
  t.gy = (int)ceil_div(cout, 16 * t.tm);
  int ct = (ncol4 + 15) / 16;
  // tune key 1: when 4 row tiles would leave a third-empty second column block (ct = 4:
  // 64 columns as 48 + 48), take 2 row tiles and all 64 columns in one block instead
  if (g_wgrad_cols && t.tm == 4 && ct == 4) {
    t.tm = 2;
    t.gy = (int)ceil_div(cout, 32);
  }
  const int tn_max = t.tm == 4 ? 3 : 4;  // <4,4> would not fit 2 waves/SIMD without spills
  t.tn = ct <= tn_max ? ct : tn_max;
  t.gx = (int)ceil_div(ncol4, 16 * t.tn);
  int64_t tiles = (int64_t)t.gx * t.gy;
  // ~1024 workgroups (4 waves each; set_tune key 18), at least 256 pixels (4 chunks per
  // wave) each: small layers get enough workgroups in flight to hide the load latency
  // (512 / 256 measured 0.5 / 1.2 % slower in the step)
  int64_t want = ceil_div(g_wgrad_wgs, tiles);
  int64_t maxs = ceil_div(P, 256);
  int64_t s = want < maxs ? want : maxs;
  if (s < 1) s = 1;
  t.px_split = (int)(ceil_div(ceil_div(P, s), 64) * 64);
  t.splits = (int)ceil_div(P, t.px_split);
  return t;
}

template <int TM, bool V4>
static void launch_wgrad_tn_v(const WGrad& p, int tn, dim3 grid, hipStream_t s) {
  const size_t lds = (size_t)3 * TM * 4 * 4 * 64 * sizeof(float) / 4 * tn;  // 3 waves x NV x 64
  switch (tn) {
#define CASE(T) \
  case T: \
    if (g_bf16) VAE2_LAUNCH((wgrad_kernel<TM, T, true, V4>), grid, dim3(256), lds, s, p); \
    else VAE2_LAUNCH((wgrad_kernel<TM, T, false, V4>), grid, dim3(256), lds, s, p); \
    break;
    CASE(1) CASE(2) CASE(3)
    default: CASE(4)
#undef CASE
  }
}

template <int TM>
static void launch_wgrad_tn(const WGrad& p, int tn, dim3 grid, hipStream_t s, bool v4) {
  if (v4) launch_wgrad_tn_v<TM, true>(p, tn, grid, s);
  else launch_wgrad_tn_v<TM, false>(p, tn, grid, s);
}


// ---------------------------------------- direct 3x3 wgrad: host dispatch ----
struct W3Tile {
  int ks, tm, tn, bh, csw, n_ci_slabs, n_co_slabs, tiles_h, tiles_w, ntiles, tps, splits;
  bool pf;
  int nr = 0;  // output channels on the VALU beside the MFMA rows (wgrad3_kernel NR)
  int nw = 4;  // waves per workgroup (wgrad3_kernel NW)
};

// Resident workgroups per CU of the wgrad3_kernel instance a tile selects (the
// launch dispatch run in probe mode + hipOccupancyMaxActiveBlocksPerMultiprocessor).
int wgrad3_blocks_per_cu(const W3Tile& t, size_t lds);
static size_t wgrad3_lds(const W3Tile& t);

bool wgrad3_shape_ok(const vae2_act* xd, const vae2_act* dyd, int k, int stride, int pad) {
  // (the KS = 1 form of the kernel measured slower than the gather kernel on 1x1 convs:
  //  without the 9-tap reuse the staging does not pay for itself)
  return k == 3 && pad == 1 && stride == 1 && xd->h == dyd->h &&
         xd->w == dyd->w && xd->ps % 4 == 0 && dyd->ps % 4 == 0 && dyd->w >= 16;
}

static W3Tile pick_w3tile(const vae2_act* xd, const vae2_act* dyd, int k) {
  W3Tile t;
  t.ks = k;
  const int cin4 = round_up((int)xd->c, 4);
  const int maxc = k == 1 ? 64 : 36;  // channels per slab (columns = taps x channels)
  int nsl = (cin4 + maxc - 1) / maxc;
  t.csw = round_up((int)ceil_div(cin4, nsl), 4);
  t.n_ci_slabs = (int)ceil_div(cin4, t.csw);
  const int nt = (k * k * t.csw + 15) / 16;
  t.tn = (nt + 3) / 4;
  const int mt = (int)((dyd->c + 15) / 16);
  t.n_co_slabs = (mt + 3) / 4;
  t.tm = (mt + t.n_co_slabs - 1) / t.n_co_slabs;
  // 18 / 36 / 72 output channels: co slabs of 16 + 2, 32 + 4, 2 x (32 + 4): MFMA rows
  // plus VALU rows (fp32 operands)
  if (k == 3 && g_dconv_nr && !g_bf16 && (dyd->c == 18 || dyd->c == 36 || dyd->c == 72)) {
    t.tm = dyd->c == 18 ? 1 : 2;
    t.nr = dyd->c == 18 ? 2 : 4;
    t.n_co_slabs = (int)(dyd->c / (16 * t.tm + t.nr));
  }
  // tune key 3: the remainder layers' column tiles over 8 waves (twice the waves per SIMD)
  if (g_wgrad_nw8 && t.nr && !g_bf16) {
    const int tn2 = (nt + 7) / 8;
    if ((t.tm == 1 && tn2 == 2) || (t.tm == 2 && tn2 == 3)) {
      t.tn = tn2;
      t.nw = 8;
    }
  }
  t.bh = (t.tm <= 2 && t.csw <= 24 && k == 3) ? 8 : 4;
  t.tiles_h = (int)ceil_div(dyd->h, t.bh);
  t.tiles_w = (int)ceil_div(dyd->w, 32);
  t.ntiles = (int)(dyd->n * t.tiles_h * t.tiles_w);
  const int gy = t.n_ci_slabs * t.n_co_slabs;
  // ~1024 workgroups in all and at most ~48 MB of partial slabs; layers with >= 1024
  // tile-slabs use >= 2 tiles per workgroup and prefetch tile t+1 while t computes
  int64_t want = ceil_div(1024, gy);
  const int64_t slab = (int64_t)dyd->c * k * k * cin4 * 4;
  const int64_t cap = 48ll << 20;
  if (want * slab > cap) want = cap / slab > 0 ? cap / slab : 1;
  if (want > t.ntiles) want = t.ntiles;
  t.tps = (int)ceil_div(t.ntiles, want);
  t.pf = (int64_t)t.ntiles * gy >= 1024;
  if (t.pf) {
    // one wave of workgroups: exactly as many as are resident at once (no straggler wave);
    // the residency comes from the instance's registers / LDS (the 18-channel 8-wave form
    // holds 145 VGPRs: one 512-thread workgroup per CU, not the 2 assumed before)
    const int64_t resident = 256 * (int64_t)wgrad3_blocks_per_cu(t, wgrad3_lds(t));
    int64_t w2 = resident / gy > 0 ? resident / gy : 1;
    if (w2 * slab > cap) w2 = cap / slab > 0 ? cap / slab : 1;
    t.tps = (int)ceil_div(t.ntiles, w2);
    if (t.tps < 2) t.tps = 2;
  }
  // at least 2 tiles per split: half the partial dW slabs (written here, read back by the
  // end-of-backward reductions) -- 36 -> 36 at 64x128 wrote 24 MB of slabs per launch,
  // 2.5x its dY.  In the concurrent training step: 814.7 -> 822.6 frames/s (A/B, same
  // box); 4 tiles per split: 789
  if (t.tps < 2) t.tps = 2;
  t.splits = (int)ceil_div(t.ntiles, t.tps);
  return t;
}

static size_t wgrad3_lds(const W3Tile& t) {
  const int npx = t.bh * 32, lpx = (t.bh + t.ks - 1) * (32 + t.ks - 1);
  const int rows = 16 * t.tm + 4 * ((t.nr + 3) / 4);
  return ((size_t)rows * (npx + 4) + (size_t)(t.csw + 1) * lpx) * sizeof(float);
}

// Probe mode of the wgrad3 dispatch: record the instance (and its block size) instead of
// launching it.
struct W3Probe {
  bool on = false;
  const void* fn = nullptr;
  unsigned threads = 0;
};
static thread_local W3Probe g_w3probe;
#define W3_LAUNCH(K, GRID, BLOCK, SHM, S, ...)                         \
  do {                                                                \
    if (g_w3probe.on) {                                               \
      g_w3probe.fn = reinterpret_cast<const void*>(K);                \
      g_w3probe.threads = dim3(BLOCK).x;                              \
    } else {                                                          \
      VAE2_LAUNCH(K, GRID, BLOCK, SHM, S, __VA_ARGS__);               \
    }                                                                 \
  } while (0)

template <int TM, int BH, bool PF>
static void wgrad3_launch_tn(const WGrad3& p, int tn, int ks, dim3 grid, size_t shm,
                             hipStream_t s, int nr = 0, int nw = 4) {
  if constexpr (TM == 1 || TM == 2) {
    if (nr && nw == 8) {  // 8 waves: (TM, TN) = (1, 2) or (2, 3) (pick_w3tile)
      constexpr int R = TM == 1 ? 2 : 4, T8 = TM == 1 ? 2 : 3;
      W3_LAUNCH((wgrad3_kernel<TM, T8, BH, PF, 3, false, R, 8>), grid, dim3(512), shm, s, p);
      return;
    }
    if (nr) {  // (TM, NR) = (1, 2) or (2, 4): pick_w3tile, fp32 operands
      constexpr int R = TM == 1 ? 2 : 4;
      switch (tn) {
#define CASE(T) \
  case T: W3_LAUNCH((wgrad3_kernel<TM, T, BH, PF, 3, false, R>), grid, dim3(256), shm, s, p); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6)
#undef CASE
      }
      return;
    }
  }
  if (ks == 1) {  // 1x1: at most 64 channels = 4 column tiles per slab, one per wave
    if (g_bf16) W3_LAUNCH((wgrad3_kernel<TM, 1, BH, PF, 1, true>), grid, dim3(256), shm, s, p);
    else W3_LAUNCH((wgrad3_kernel<TM, 1, BH, PF, 1>), grid, dim3(256), shm, s, p);
    return;
  }
  switch (tn) {
#define CASE(T) \
  case T:                                                                         \
    if (g_bf16) W3_LAUNCH((wgrad3_kernel<TM, T, BH, PF, 3, true>), grid, dim3(256), shm, s, p); \
    else W3_LAUNCH((wgrad3_kernel<TM, T, BH, PF, 3>), grid, dim3(256), shm, s, p);   \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6)
#undef CASE
  }
}

template <int BH, bool PF>
static void wgrad3_launch_tm(const WGrad3& p, const W3Tile& t, dim3 grid, size_t shm,
                             hipStream_t s) {
  switch (t.tm) {
    case 1: wgrad3_launch_tn<1, BH, PF>(p, t.tn, t.ks, grid, shm, s, t.nr, t.nw); break;
    case 2: wgrad3_launch_tn<2, BH, PF>(p, t.tn, t.ks, grid, shm, s, t.nr, t.nw); break;
    case 3: wgrad3_launch_tn<3, BH, PF>(p, t.tn, t.ks, grid, shm, s); break;
    default: wgrad3_launch_tn<4, BH, PF>(p, t.tn, t.ks, grid, shm, s); break;
  }
}

template <int BH>
static void wgrad3_launch(const WGrad3& p, const W3Tile& t, dim3 grid, size_t shm,
                          hipStream_t s) {
  if (t.pf) wgrad3_launch_tm<BH, true>(p, t, grid, shm, s);
  else wgrad3_launch_tm<BH, false>(p, t, grid, shm, s);
}

int wgrad3_blocks_per_cu(const W3Tile& t, size_t lds) {
  struct Key {
    int tm, tn, bh, ks, nr, nw, pf, bf;
    size_t lds;
    int n;
  };
  static Key cache[32];
  static int ncache = 0;
  const int bf = g_bf16;
  for (int i = 0; i < ncache; ++i) {
    const Key& k = cache[i];
    if (k.tm == t.tm && k.tn == t.tn && k.bh == t.bh && k.ks == t.ks && k.nr == t.nr &&
        k.nw == t.nw && k.pf == (int)t.pf && k.bf == bf && k.lds == lds)
      return k.n;
  }
  WGrad3 p{};
  g_w3probe = W3Probe{};
  g_w3probe.on = true;
  if (t.bh == 8) wgrad3_launch<8>(p, t, dim3(1), lds, nullptr);
  else wgrad3_launch<4>(p, t, dim3(1), lds, nullptr);
  g_w3probe.on = false;
  int n = 0;
  if (!g_w3probe.fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(
                           &n, g_w3probe.fn, (int)g_w3probe.threads, lds) != hipSuccess ||
      n < 1) {
    (void)hipGetLastError();
    n = 1;
  }
  if (ncache < 32) cache[ncache++] = Key{t.tm, t.tn, t.bh, t.ks, t.nr, t.nw, (int)t.pf, bf, lds, n};
  return n;
}

}  // namespace vae2

using namespace vae2;

extern "C" {

int vae2_wgrad_defer(int on) {
  const int prev = g_wr_defer ? 1 : 0;
  g_wr_defer = on != 0;
  return prev;
}

static int wgrad_flush_impl(void* stream, bool own_only) {
  const char* fn = "vae2_wgrad_flush";
  hipStream_t want = as_stream(stream);
  std::vector<WRQueued> q;
  {
    std::lock_guard<std::mutex> lk(g_wr_mu);
    if (own_only) {  // only the jobs queued from this stream (no cross-stream ordering)
      std::vector<WRQueued> keep;
      for (const WRQueued& j : g_wr_queue) (j.stream == want ? q : keep).push_back(j);
      g_wr_queue.swap(keep);
    } else {
      q.swap(g_wr_queue);
    }
  }
  size_t i = 0;
  // every job on the given stream: the caller orders it after the jobs' own streams
  while (i < q.size()) {  // kWrMaxJobs per launch
    WRMulti m{};
    hipStream_t st = want;
    int blocks = 0;
    while (i < q.size() && m.n < kWrMaxJobs) {
      WRJob j = q[i].job;
      // a job accumulating into dW elements a job of this launch writes waits for the
      // next launch (e.g. a discriminator applied to real and fake inputs)
      const float* lo = j.dw;
      const float* hi = j.dw + (int64_t)(j.cout - 1) * j.ld + (int64_t)j.cin * j.k * j.k;
      bool clash = false;
      for (int u = 0; u < m.n; ++u) {
        const float* lo2 = m.j[u].dw;
        const float* hi2 = m.j[u].dw + (int64_t)(m.j[u].cout - 1) * m.j[u].ld +
                           (int64_t)m.j[u].cin * m.j[u].k * m.j[u].k;
        if (lo < hi2 && lo2 < hi) clash = true;
      }
      if (clash) break;
      j.blk0 = blocks;
      blocks += (int)ceil_div((int64_t)j.cout * j.k * j.k * j.cin4, 32);
      m.j[m.n++] = j;
      ++i;
    }
    VAE2_LAUNCH(wgrad_reduce_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, st, m);
    const int rc = check_launch(fn);
    if (rc) return rc;
  }
  return 0;
}

int vae2_wgrad_flush(void* stream) { return wgrad_flush_impl(stream, false); }

int vae2_wgrad_flush_stream(void* stream) { return wgrad_flush_impl(stream, true); }


// Workspace layout: `part` floats of partial dW slabs (the largest any kernel form may
// write for the layer), then the bias-gradient partials [2][rows][cout], then 4 spare.
struct WgradWs {
  int64_t part, total;
};
static WgradWs wgrad_ws(const vae2_act* xd, const vae2_act* dyd, int k) {
  const int ncol4 = k * k * round_up((int)xd->c, 4);
  const WTile t = pick_wtile(act_pixels(dyd), (int)dyd->c, ncol4);
  int64_t splits = t.splits;
  if ((k == 3 || k == 1) && xd->h == dyd->h && xd->w == dyd->w) {  // direct kernel may run
    splits = std::max<int64_t>(splits, pick_w3tile(xd, dyd, k).splits);
    splits = std::max<int64_t>(splits, wgrad3n_splits(xd, dyd));
  }
  const int64_t part = splits * dyd->c * ncol4;
  return WgradWs{part, part + 2 * vae2_bn_partial_rows(dyd) * dyd->c + 4};
}

int64_t vae2_conv2d_bwd_weight_ws_size(const vae2_act* xd, const vae2_act* dyd, int k) {
  if (!act_ok(xd) || !act_ok(dyd)) return 0;
  return wgrad_ws(xd, dyd, k).total;
}

static int bwd_weight_impl(const float* x, const vae2_act* xd, const float* dy,
                           const vae2_act* dyd, float* dw, int64_t dw_ld, float* dbias,
                           int k, int stride, int pad, int accumulate, float* ws,
                           int64_t ws_size, void* stream, const float* isave, int irelu,
                           const char* fn) {
  VAE2_REQUIRE(xd && dw_ld >= xd->c * k * k, fn, "bad dW row stride");
  VAE2_REQUIRE(x && dy && dw && ws, fn, "null pointer");
  VAE2_REQUIRE(conv_shapes_ok(xd, dyd, k, stride, pad), fn, "inconsistent conv shapes");
  VAE2_REQUIRE(fits32(xd) && fits32(dyd), fn, "tensor too large for 32-bit indexing");
  const WgradWs wsl = wgrad_ws(xd, dyd, k);
  VAE2_REQUIRE(ws_size >= wsl.total, fn, "workspace too small");
  hipStream_t s = as_stream(stream);
  const int cin4 = round_up((int)xd->c, 4);
  const int ncol4 = k * k * cin4;
  int splits = 0;
  const bool direct = g_conv_algo != 1 && wgrad3_shape_ok(xd, dyd, k, stride, pad) &&
                      vec_ok(x, (int)xd->ps) && vec_ok(dy, (int)dyd->ps);
  VAE2_REQUIRE(direct || !isave, fn,
               "input BatchNorm needs the direct 3x3 weight-gradient kernel (vae2_conv2d_bnin_ok)");
  if (direct && k == 3) {  // the 18 / 36 / 72-channel branches (wgrad_narrow.hip)
    splits = wgrad3n_launch(x, xd, dy, dyd, ws, isave, irelu, act_bytes(xd), act_bytes(dyd), s);
    if (splits < 0) return check_launch(fn);
  }
  if (direct && !splits) {
    W3Tile t3 = pick_w3tile(xd, dyd, k);
    WGrad3 q{};
    q.x = x; q.x_ps = (int)xd->ps; q.cin = (int)xd->c; q.cin4 = cin4;
    q.h = (int)xd->h; q.w = (int)xd->w;
    q.dy = dy; q.dy_ps = (int)dyd->ps; q.cout = (int)dyd->c;
    q.tiles_h = t3.tiles_h; q.tiles_w = t3.tiles_w; q.ntiles = t3.ntiles;
    q.tiles_per_split = t3.tps;
    q.csw = t3.csw; q.n_ci_slabs = t3.n_ci_slabs;
    q.x_bytes = act_bytes(xd); q.dy_bytes = act_bytes(dyd);
    q.part = ws;
    q.isave = isave;
    q.irelu = irelu ? 1 : 0;
    dim3 grid((unsigned)t3.splits, (unsigned)(t3.n_ci_slabs * t3.n_co_slabs));
    const size_t shm = wgrad3_lds(t3);
    if (t3.bh == 8) wgrad3_launch<8>(q, t3, grid, shm, s);
    else wgrad3_launch<4>(q, t3, grid, shm, s);
    int rc = check_launch(fn);
    if (rc) return rc;
    splits = t3.splits;
  }
  WTile t = pick_wtile(act_pixels(dyd), (int)dyd->c, ncol4);
  if (splits) goto reduce;
  {
  WGrad p{};
  p.x = x; p.x_ps = (int)xd->ps; p.cin = (int)xd->c; p.cin4 = cin4;
  p.x_h = (int)xd->h; p.x_w = (int)xd->w;
  p.dy = dy; p.dy_ps = (int)dyd->ps; p.cout = (int)dyd->c;
  p.o_n = (int)dyd->n; p.o_h = (int)dyd->h; p.o_w = (int)dyd->w;
  p.k = k; p.stride = stride; p.pad = pad;
  p.P = (int)act_pixels(dyd);
  p.px_split = t.px_split;
  p.part = ws;
  p.x_bytes = act_bytes(xd);
  p.dy_bytes = act_bytes(dyd);
  p.ohw_div = FastDiv((uint32_t)(dyd->h * dyd->w));
  p.ow_div = FastDiv((uint32_t)dyd->w);
  p.cin4_div = FastDiv((uint32_t)cin4);
  dim3 grid(t.gx, t.gy, (unsigned)t.splits);
  // 16-byte channel-quad operand loads (quad-transposed into fragments)
  const bool v4 = g_vec_out && vec_ok(x, (int)xd->ps) && vec_ok(dy, (int)dyd->ps);
  switch (t.tm) {
    case 1: launch_wgrad_tn<1>(p, t.tn, grid, s, v4); break;
    case 2: launch_wgrad_tn<2>(p, t.tn, grid, s, v4); break;
    case 3: launch_wgrad_tn<3>(p, t.tn, grid, s, v4); break;
    default: launch_wgrad_tn<4>(p, t.tn, grid, s, v4); break;
  }
  int rc = check_launch(fn);
  if (rc) return rc;
  splits = t.splits;
  }
reduce:
  int64_t slab = dyd->c * (int64_t)ncol4;
  int rc = 0;
  if (g_wr_defer) {
    WRJob j{ws, dw, dw_ld, splits, (int)dyd->c, (int)xd->c, cin4, k, accumulate, 0};
    std::lock_guard<std::mutex> lk(g_wr_mu);
    g_wr_queue.push_back(WRQueued{j, s});
  } else {
    VAE2_LAUNCH(wgrad_reduce_kernel, dim3((unsigned)ceil_div(slab, 32)), dim3(256), 0, s,
                (const float*)ws, splits, (int)dyd->c, (int)xd->c, cin4, k, dw, dw_ld,
                accumulate);
    rc = check_launch(fn);
    if (rc) return rc;
  }
  if (dbias) {
    float* bp = ws + wsl.part;
    rc = vae2_bn_stats(dy, dyd, bp, stream);
    if (rc) return rc;
    rc = bias_grad_from_partials(bp, vae2_bn_partial_rows(dyd), dyd->c, dbias, accumulate,
                                 stream);
    if (rc) return rc;
  }
  return 0;
}

int vae2_conv2d_bwd_weight_ld(const float* x, const vae2_act* xd, const float* dy,
                              const vae2_act* dyd, float* dw, int64_t dw_ld, float* dbias,
                              int k, int stride, int pad, int accumulate, float* ws,
                              int64_t ws_size, void* stream) {
  return bwd_weight_impl(x, xd, dy, dyd, dw, dw_ld, dbias, k, stride, pad, accumulate, ws,
                         ws_size, stream, nullptr, 0, "vae2_conv2d_bwd_weight");
}

int vae2_conv2d_bwd_weight_bnin(const float* x, const vae2_act* xd, const float* bn_save,
                                int relu, const float* dy, const vae2_act* dyd, float* dw,
                                float* dbias, int k, int stride, int pad, int accumulate,
                                float* ws, int64_t ws_size, void* stream) {
  const char* fn = "vae2_conv2d_bwd_weight_bnin";
  if (!xd || !bn_save) return fail(fn, "null pointer");
  return bwd_weight_impl(x, xd, dy, dyd, dw, xd->c * k * k, dbias, k, stride, pad, accumulate,
                         ws, ws_size, stream, bn_save, relu, fn);
}

int vae2_conv2d_bwd_weight(const float* x, const vae2_act* xd, const float* dy,
                           const vae2_act* dyd, float* dw, float* dbias, int k,
                           int stride, int pad, int accumulate, float* ws,
                           int64_t ws_size, void* stream) {
  if (!xd) return fail("vae2_conv2d_bwd_weight", "null descriptor");
  return vae2_conv2d_bwd_weight_ld(x, xd, dy, dyd, dw, xd->c * k * k, dbias, k, stride, pad,
                                   accumulate, ws, ws_size, stream);
}

}  // extern "C"

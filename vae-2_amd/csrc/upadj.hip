// Adjoints of bilinear upsampling (F.interpolate, align_corners=False) into up to three
// targets at once, dx_s = up_s^T(dy) ("Heads and resampling units"):
//   enc_hrnet.py:835-837 / :893-895 / :951-953 (heads)  -> vae2_upsample_bilinear_bwd_multi
//   enc_hrnet.py:242-245 (fuse rows, accumulating)      -> vae2_upsample_bilinear_bwd_pow2
#include "heads.h"

namespace vae2 {

int g_adj_stream = 1, g_adj_fused = 1, g_adj_band = kAdjBandDefault, g_fuse_adj3 = 0;  // heads.h

// ------------------------------------------- upsampling adjoint, all sources ----
// dx_s = up_s^T(dy) for every source s at once, separably.
// Horizontal pass, workgroup = (dY row, 64-pixel chunk, 64-channel block): source
// columns are partitioned between chunks (ix belongs to the chunk holding the output
// coordinate of its centre), the chunk's dY pixels plus the interpolation halo are
// staged in LDS once with per-pixel forward tables {i0, i1, l0, l1}, and each owned
// column gathers hb_s[n][oy][ix][c] = sum_ox w(ox, ix) dy[n][oy][ox][c] from LDS.
// Vertical pass, workgroup = (target row, 64-channel block): the row's weights are
// tabulated once, then dx_s[n][iy][ix][c] = sum_oy w(oy, iy) hb_s[n][oy][ix][c].
// The weights are exactly upsample_fwd_kernel's (lerp_index).  Lane = channel.
struct UpAdj {
  const float* dy;
  int dy_ps, H, W, C;
  float* hb[3];
  float* dx[3];
  int zh[3], zw[3], dx_ps[3];
  float sh[3], sw[3];  // (up_adj3_kernel reads neither; adj_plan fills them on every route)
  int halo, nxb;
  float beta[3];  // up_adj3_kernel: dx_s = adjoint + beta_s * dx_s (the fuse adjoints)
};

__device__ __forceinline__ void adj_window(int i, int in_size, int out_size, float scale,
                                           int& lo, int& hi) {
  lo = (int)floorf(((float)i - 0.5f) / scale - 0.5f) - 1;
  hi = (int)ceilf(((float)i + 1.5f) / scale - 0.5f) + 1;
  if (lo < 0) lo = 0;
  if (hi > out_size - 1) hi = out_size - 1;
  if (i == in_size - 1) hi = out_size - 1;  // clamped sources beyond the last input
}

// First source column owned by chunk xb (monotone in xb; xb = nxb gives zw).
__device__ __forceinline__ int adj_owned_begin(int xb, int nxb, int zw, float sw) {
  if (xb >= nxb) return zw;
  if (xb <= 0) return 0;
  int b = (int)ceilf(((float)(xb * kUsXB) + 0.5f) * sw - 0.5f);
  return b < 0 ? 0 : (b > zw ? zw : b);
}

template <int NUP>
__global__ __launch_bounds__(256) void up_adj_h_kernel(UpAdj p) {
  extern __shared__ __attribute__((aligned(16))) float asm_[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ncb = (p.C + 63) / 64;
  const int xb = blockIdx.x % p.nxb;
  const int cbi = (blockIdx.x / p.nxb) % ncb;
  const int row = blockIdx.x / (p.nxb * ncb);  // n*H + oy
  const int span = kUsXB + 2 * p.halo;
  f4* tab = reinterpret_cast<f4*>(asm_);              // [NUP][span]
  float* st = asm_ + 4 * NUP * span;                  // [span][64]
  int ib[3], ie[3], wlo = 1 << 30, whi = -1;
#pragma unroll
  for (int s = 0; s < NUP; ++s) {
    ib[s] = adj_owned_begin(xb, p.nxb, p.zw[s], p.sw[s]);
    ie[s] = adj_owned_begin(xb + 1, p.nxb, p.zw[s], p.sw[s]);
    if (ie[s] > ib[s]) {
      int lo, hi, lo2, hi2;
      adj_window(ib[s], p.zw[s], p.W, p.sw[s], lo, hi);
      adj_window(ie[s] - 1, p.zw[s], p.W, p.sw[s], lo2, hi2);
      wlo = lo < wlo ? lo : wlo;
      whi = hi2 > whi ? hi2 : whi;
    }
  }
  if (whi < wlo) return;  // no owned columns (uniform over the workgroup)
  const int cnt = whi - wlo + 1;  // <= span (host-sized halo)
#pragma unroll
  for (int s = 0; s < NUP; ++s) {
    for (int i = threadIdx.x; i < cnt; i += 256) {
      const Lerp lx = lerp_index(wlo + i, p.zw[s], p.sw[s]);
      tab[s * span + i] = f4{__int_as_float(lx.i0), __int_as_float(lx.i1), lx.l0, lx.l1};
    }
  }
  {
    const int c = cbi * 64 + lane;
    const bool cok = c < p.C;
    const float* drow = p.dy + (int64_t)row * p.W * p.dy_ps + c;
    {
      constexpr int SU = 24;  // pixels per wave in flight (span <= 96: one round trip)
      for (int i0 = wave; i0 < cnt; i0 += 4 * SU) {
        float v[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          const int i = i0 + 4 * u;
          v[u] = (cok && i < cnt) ? drow[(int64_t)(wlo + i) * p.dy_ps] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          const int i = i0 + 4 * u;
          if (i < cnt) st[i * 64 + lane] = v[u];
        }
      }
    }
    __syncthreads();
    if (!cok) return;
    // Work items: (source, half of its owned columns); wave w streams items w, w+4, ...
    // Streaming: pixels ox ascend, so each ox adds l0 to column i0 and l1 to i1 in
    // {i0, i0+1} with i0 non-decreasing; two running sums (columns cur, cur+1) are kept
    // and column cur is final (stored) once i0 moves past it.
    for (int item = wave; item < 2 * NUP; item += 4) {
      const int s = item % NUP, half = item / NUP;
      const int mid = ib[s] + (ie[s] - ib[s] + 1) / 2;
      const int cb = half ? mid : ib[s], ce = half ? ie[s] : mid;
      if (cb >= ce) continue;
      int lo, hi, lo2, hi2;
      adj_window(cb, p.zw[s], p.W, p.sw[s], lo, hi);
      adj_window(ce - 1, p.zw[s], p.W, p.sw[s], lo2, hi2);
      float* hrow = p.hb[s] + (int64_t)row * p.zw[s] * p.C + c;
      const f4* ts = tab + s * span - wlo;
      const float* sv = st - wlo * 64 + lane;
      int cur = cb - 1;
      float a0 = 0.f, a1 = 0.f;  // sums of columns cur, cur + 1
      for (int ox = lo; ox <= hi2; ++ox) {
        const f4 t = ts[ox];  // wave-uniform: moved to scalar registers
        const int i0 = __builtin_amdgcn_readfirstlane(__float_as_int(t[0]));
        const int i1 = __builtin_amdgcn_readfirstlane(__float_as_int(t[1]));
        const float l0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t[2])));
        const float l1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t[3])));
        const float v = sv[ox * 64];
        while (cur < i0) {  // wave-uniform
          if (cur >= cb && cur < ce) hrow[(int64_t)cur * p.C] = a0;
          a0 = a1;
          a1 = 0.f;
          ++cur;
        }
        // now i0 <= cur (i0 < cur only left of the owned range: not ours)
        if (i0 == cur) a0 = __builtin_fmaf(l0, v, a0);
        if (i1 == cur) a0 = __builtin_fmaf(l1, v, a0);
        else if (i1 == cur + 1) a1 = __builtin_fmaf(l1, v, a1);
      }
      if (cur >= cb && cur < ce) hrow[(int64_t)cur * p.C] = a0;
      if (cur + 1 >= cb && cur + 1 < ce) hrow[(int64_t)(cur + 1) * p.C] = a1;
    }
  }
}

__global__ __launch_bounds__(256) void up_adj_v_kernel(UpAdj p, int s) {
  __shared__ float wy[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x;  // n*zh + iy
  const int n = row / p.zh[s], iy = row - n * p.zh[s];
  const int c = blockIdx.y * 64 + lane;
  int lo, hi;
  adj_window(iy, p.zh[s], p.H, p.sh[s], lo, hi);
  const int cnt = hi - lo + 1 < 64 ? hi - lo + 1 : 64;  // host guarantees <= 64
  if (threadIdx.x < cnt) {
    const Lerp ly = lerp_index(lo + threadIdx.x, p.zh[s], p.sh[s]);
    wy[threadIdx.x] = (ly.i0 == iy ? ly.l0 : 0.f) + (ly.i1 == iy ? ly.l1 : 0.f);
  }
  __syncthreads();
  if (c >= p.C) return;
  const float* hb = p.hb[s] + ((int64_t)n * p.H + lo) * p.zw[s] * p.C + c;
  float* out = p.dx[s] + (int64_t)row * p.zw[s] * p.dx_ps[s] + c;
  const int64_t rs = (int64_t)p.zw[s] * p.C;
  for (int ix = wave; ix < p.zw[s]; ix += 8) {
    const bool two = ix + 4 < p.zw[s];
    const float* h0 = hb + (int64_t)ix * p.C;
    const float* h1 = hb + (int64_t)(two ? ix + 4 : ix) * p.C;
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll 4
    for (int t = 0; t < cnt; ++t) {
      acc0 = __builtin_fmaf(wy[t], h0[t * rs], acc0);
      acc1 = __builtin_fmaf(wy[t], h1[t * rs], acc1);
    }
    out[(int64_t)ix * p.dx_ps[s]] = acc0;
    if (two) out[(int64_t)(ix + 4) * p.dx_ps[s]] = acc1;
  }
}

// Exact 2^(s+1) ratios: static stencils (hat_w, common.h).
constexpr int kAdjHalo = 4;  // F/2 for F <= 8

// Horizontal pass, workgroup = (dY row, 64-pixel chunk, 64-channel block); the chunk and a
// 4-pixel halo are staged in LDS (lane = channel); wave w computes the owned source
// columns j = w, w + 4, ... of every source with immediate LDS offsets.
template <int NUP>
__global__ __launch_bounds__(256) void up_adj2_h_kernel(UpAdj p) {
  constexpr int SPAN = kUsXB + 2 * kAdjHalo, PER = SPAN / 4;
  __shared__ float st[SPAN][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ncb = (p.C + 63) / 64;
  const int xb = blockIdx.x % p.nxb;
  const int cbi = (blockIdx.x / p.nxb) % ncb;
  const int row = blockIdx.x / (p.nxb * ncb);  // n*H + oy
  const int c = cbi * 64 + lane;
  const bool cok = c < p.C;
  const int x0 = xb * kUsXB;
  const float* drow = p.dy + (int64_t)row * p.W * p.dy_ps + (cok ? c : 0);
  float v[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int ox = x0 - kAdjHalo + wave + 4 * u;
    v[u] = (cok && ox >= 0 && ox < p.W) ? drow[(int64_t)ox * p.dy_ps] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) st[wave + 4 * u][lane] = v[u];
  __syncthreads();
  if (!cok) return;
#pragma unroll
  for (int s = 0; s < NUP; ++s) {
    const int F = 2 << s, zw = p.zw[s];
    const float* sw = &st[F * wave + kAdjHalo][lane];  // column j = wave: pixels F*wave + d
    float* hrow = p.hb[s] + (int64_t)row * zw * p.C + c;
#pragma unroll
    for (int jj = 0; jj < kUsXB / (2 << s) / 4; ++jj) {
      const int j = wave + 4 * jj, ix = x0 / F + j;
      float acc = 0.f;
#pragma unroll
      for (int d = -(1 << s); d < 3 * (1 << s); ++d) acc += hat_w(d, F) * sw[(4 * F * jj + d) * 64];
      if (ix == 0) {  // virtual column -1 (pixels d - F)
#pragma unroll
        for (int d = 2 << s; d < 3 * (1 << s); ++d) acc += hat_w(d, F) * sw[(d - F) * 64];
      }
      if (ix == zw - 1) {  // virtual column zw (pixels F*(j+1) + d)
#pragma unroll
        for (int d = -(1 << s); d < 0; ++d) acc += hat_w(d, F) * sw[(4 * F * jj + F + d) * 64];
      }
      hrow[(int64_t)ix * p.C] = acc;
    }
  }
}

// Vertical pass of source S (F = 2^(S+1)), workgroup = (target row, 64-channel block).
template <int S>
__global__ __launch_bounds__(256) void up_adj2_v_kernel(UpAdj p) {
  constexpr int F = 2 << S, HF = 1 << S;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = blockIdx.x;  // n*zh + iy
  const int zh = p.zh[S], zw = p.zw[S];
  const int n = row / zh, iy = row - n * zh;
  const int c = blockIdx.y * 64 + lane;
  if (c >= p.C) return;
  const int64_t rs = (int64_t)zw * p.C;
  const float* hb = p.hb[S] + (int64_t)n * p.H * rs + c;
  float* out = p.dx[S] + (int64_t)row * zw * p.dx_ps[S] + c;
  const int oy0 = F * iy;
  constexpr int U = 4;  // target columns per wave iteration (their loads in flight together)
  constexpr int NT = 3 * F;  // 2F taps + the two edge folds (HF rows each)
  for (int ix0 = wave; ix0 < zw; ix0 += 4 * U) {
    float v[U][NT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ix = ix0 + 4 * u;
      const float* h = hb + (int64_t)(ix < zw ? ix : zw - 1) * p.C;
#pragma unroll
      for (int d = -HF; d < 3 * HF; ++d) {
        const int oy = oy0 + d;
        v[u][d + HF] = (oy >= 0 && oy < p.H) ? h[(int64_t)oy * rs] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < HF; ++e) {  // edge folds: rows d - F (top, d = F + e), F*zh + d
        v[u][2 * F + e] = iy == 0 ? h[(int64_t)e * rs] : 0.f;
        v[u][2 * F + HF + e] = iy == zh - 1 ? h[(int64_t)(F * zh - HF + e) * rs] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ix = ix0 + 4 * u;
      if (ix >= zw) break;
      float acc = 0.f;
#pragma unroll
      for (int d = -HF; d < 3 * HF; ++d) acc += hat_w(d, F) * v[u][d + HF];
      if (iy == 0) {
#pragma unroll
        for (int e = 0; e < HF; ++e) acc += hat_w(F + e, F) * v[u][2 * F + e];
      }
      if (iy == zh - 1) {
#pragma unroll
        for (int e = 0; e < HF; ++e) acc += hat_w(e - HF, F) * v[u][2 * F + HF + e];
      }
      out[(int64_t)ix * p.dx_ps[S]] = acc;
    }
  }
}

// Streaming form of the vertical pass: it only mixes hb rows, and an hb row
// (zw * C floats, ix-major) is contiguous, so thread = 4 consecutive floats of the row:
// one 16-byte load per contributing row (2F taps, plus the edge folds on the first / last
// target row: uniform per workgroup), the same weights and summation order as
// up_adj2_v_kernel, then the 4 results go to (ix, c) = divmod(k, C) of the (possibly
// channel-padded) dx layout.  Workgroup = (target row, slice of the row).  Needs
// zw * C % 4 == 0 (16-byte aligned rows).
template <int S>
__global__ __launch_bounds__(256) void up_adj2_vs_kernel(UpAdj p, FastDiv cdiv) {
  constexpr int F = 2 << S, HF = 1 << S;
  const int row = blockIdx.x;  // n*zh + iy
  const int zh = p.zh[S], zw = p.zw[S];
  const int n = row / zh, iy = row - n * zh;
  const int64_t rs = (int64_t)zw * p.C;
  const int nq = (int)(rs >> 2);
  const float* hb = p.hb[S] + (int64_t)n * p.H * rs;
  float* out = p.dx[S] + (int64_t)row * zw * p.dx_ps[S];
  const int oy0 = F * iy;
  const uint32_t C = (uint32_t)p.C, dps = (uint32_t)p.dx_ps[S];
  for (int q = blockIdx.y * 256 + threadIdx.x; q < nq; q += gridDim.y * 256) {
    const int64_t k4 = 4 * (int64_t)q;
    f4 v[4 * HF];
#pragma unroll
    for (int d = -HF; d < 3 * HF; ++d) {
      const int oy = oy0 + d;
      v[d + HF] = (oy >= 0 && oy < p.H) ? *reinterpret_cast<const f4*>(hb + oy * rs + k4)
                                        : f4{0.f, 0.f, 0.f, 0.f};
    }
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = -HF; d < 3 * HF; ++d) acc += hat_w(d, F) * v[d + HF];
    if (iy == 0) {
#pragma unroll
      for (int e = 0; e < HF; ++e)
        acc += hat_w(F + e, F) * *reinterpret_cast<const f4*>(hb + e * rs + k4);
    }
    if (iy == zh - 1) {
#pragma unroll
      for (int e = 0; e < HF; ++e)
        acc += hat_w(e - HF, F) *
               *reinterpret_cast<const f4*>(hb + (int64_t)(F * zh - HF + e) * rs + k4);
    }
    uint32_t ix = cdiv.div((uint32_t)k4), c = (uint32_t)k4 - ix * C;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      out[(int64_t)ix * dps + c] = acc[i];
      if (++c == C) { c = 0; ++ix; }
    }
  }
}

// One-pass form of the power-of-two adjoint: dx_s = V_s^T H_s^T dy for every source with
// dy read once (plus a row halo) and no hb intermediate (the two-pass form above writes and
// re-reads 1/2 + 1/4 + 1/8 of dy).  Workgroup = (image, band of `br` dy rows, 64-pixel
// chunk, 64-channel block); lane = channel; wave w owns the source columns whose pixels
// start in [x0 + 16w, x0 + 16w + 16): 16/F per source.  The band's dy rows plus HF_max rows
// above and below stream through registers (the next row's loads in flight during the
// current row's arithmetic).  A dy row oy feeds exactly two target rows of source s,
// ih = (oy + HF) / F and ih - 1 (taps d = oy - F*ih and d + F); per source and owned column
// two accumulators follow them, and a row is stored once oy has moved past it.  Virtual
// rows / columns -1 and z are folded into 0 / z-1 as in up_adj2_h / up_adj2_vs, with the
// same hat_w weights; interior outputs keep the two-pass summation order.

// Per-source state of up_adj3_kernel: the wave's 16/F owned columns in the two target rows
// the current dy row feeds (lo = ih - 1, hi = ih), cur = ih.
template <int S>
struct Adj3Src {
  static constexpr int F = 2 << S, HF = 1 << S, J = 8 >> S;
  float lo[J], hi[J];
  int cur;
};

template <int S>
__device__ __forceinline__ void adj3_store(const Adj3Src<S>& a, const UpAdj& p, int n, int iy,
                                           int b0, int b1, int px0, int c, bool cok) {
  constexpr int F = Adj3Src<S>::F;
  if (!cok || iy < b0 / F || iy >= b1 / F) return;
  float* out = p.dx[S] + ((int64_t)n * p.zh[S] + iy) * p.zw[S] * p.dx_ps[S] + c;
  const int ix0 = px0 / F;
  const float beta = p.beta[S];
  if (beta != 0.f) {
    float old[Adj3Src<S>::J];
#pragma unroll
    for (int j = 0; j < Adj3Src<S>::J; ++j) old[j] = out[(int64_t)(ix0 + j) * p.dx_ps[S]];
#pragma unroll
    for (int j = 0; j < Adj3Src<S>::J; ++j)
      out[(int64_t)(ix0 + j) * p.dx_ps[S]] = a.lo[j] + beta * old[j];
    return;
  }
#pragma unroll
  for (int j = 0; j < Adj3Src<S>::J; ++j) out[(int64_t)(ix0 + j) * p.dx_ps[S]] = a.lo[j];
}

// dy row oy (pixels px0 - HM + i in v[i]) into source S's accumulators.
template <int S, int HM>
__device__ __forceinline__ void adj3_row(Adj3Src<S>& a, const float* v, int oy, const UpAdj& p,
                                         int n, int b0, int b1, int px0, int c, bool cok) {
  constexpr int F = Adj3Src<S>::F, HF = Adj3Src<S>::HF, J = Adj3Src<S>::J;
  const int ih = (oy + HF) >> (S + 1);
  if (ih != a.cur) {  // target row cur - 1 is complete
    adj3_store<S>(a, p, n, a.cur - 1, b0, b1, px0, c, cok);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      a.lo[j] = a.hi[j];
      a.hi[j] = 0.f;
    }
    a.cur = ih;
  }
  const int d = oy - F * ih;
  const float wh = hat_w(d, F), wl = hat_w(d + F, F);
  const int zw = p.zw[S], ix0 = px0 / F;
  const int mode = ih == p.zh[S] ? 2 : ih == 0 ? 1 : 0;  // 2: row zh folds into zh - 1; 1: -1 into 0
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const float* vj = v + HM + F * j;  // pixel px0 + F*j
    float h = 0.f;
#pragma unroll
    for (int dd = -HF; dd < 3 * HF; ++dd) h += hat_w(dd, F) * vj[dd];
    if (ix0 + j == 0) {  // virtual column -1 (pixels dd - F)
#pragma unroll
      for (int dd = F; dd < 3 * HF; ++dd) h += hat_w(dd, F) * vj[dd - F];
    }
    if (ix0 + j == zw - 1) {  // virtual column zw (pixels F*(j+1) + dd)
#pragma unroll
      for (int dd = -HF; dd < 0; ++dd) h += hat_w(dd, F) * vj[F + dd];
    }
    if (mode == 2) {
      a.lo[j] += wh * h;
      a.lo[j] += wl * h;
    } else if (mode == 1) {
      a.hi[j] += wh * h;
      a.hi[j] += wl * h;
    } else {
      a.hi[j] += wh * h;
      a.lo[j] += wl * h;
    }
  }
}

template <int NUP>
__global__ __launch_bounds__(256) void up_adj3_kernel(UpAdj p, int br, int nband) {
  constexpr int HM = 1 << (NUP - 1);  // row / pixel halo: HF of the coarsest source
  constexpr int NV = 16 + 2 * HM;     // dy pixels per wave and row
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ncb = (p.C + 63) >> 6;
  // consecutive logical blocks on one XCD: neighbouring chunks / bands share dy halo rows
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int xb = lb % p.nxb;
  int t = lb / p.nxb;
  const int cbi = t % ncb;
  t /= ncb;
  const int band = t % nband, n = t / nband;
  const int c = cbi * 64 + lane;
  const bool cok = c < p.C;
  const int b0 = band * br, b1 = b0 + br < p.H ? b0 + br : p.H;
  const int ys = b0 - HM > 0 ? b0 - HM : 0, ye = b1 + HM < p.H ? b1 + HM : p.H;
  const int px0 = xb * kUsXB + 16 * wave;
  // One buffer resource per dy row (num_records = the row's bytes): pixels left of the row
  // wrap to huge offsets and pixels right of it exceed the row, so both load 0 with no
  // per-pixel test; pad channels use an offset past any row.
  const uint32_t pstep = (uint32_t)p.dy_ps * 4u, rbytes = (uint32_t)p.W * pstep;
  const uint32_t loff = cok ? (uint32_t)(px0 - HM) * pstep + 4u * (uint32_t)c : kOOB;
  const float* img = p.dy + (int64_t)n * p.H * p.W * p.dy_ps;
  auto load_row = [&](int oy, float* dst) {
    const __amdgpu_buffer_rsrc_t dr = make_rsrc(img + (int64_t)oy * p.W * p.dy_ps, rbytes);
#pragma unroll
    for (int i = 0; i < NV; ++i) dst[i] = load1(dr, loff + (uint32_t)i * pstep);
  };
  Adj3Src<0> a0;
  Adj3Src<1> a1;
  Adj3Src<2> a2;
  a0.cur = (ys + 1) >> 1;
  a1.cur = (ys + 2) >> 2;
  a2.cur = (ys + 4) >> 3;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a0.lo[j] = a0.hi[j] = 0.f;
    if (j < 4) a1.lo[j] = a1.hi[j] = 0.f;
    if (j < 2) a2.lo[j] = a2.hi[j] = 0.f;
  }
  float v[NV], nv[NV];
  load_row(ys, v);
  for (int oy = ys; oy < ye; ++oy) {
    if (oy + 1 < ye) load_row(oy + 1, nv);
    adj3_row<0, HM>(a0, v, oy, p, n, b0, b1, px0, c, cok);
    if constexpr (NUP > 1) adj3_row<1, HM>(a1, v, oy, p, n, b0, b1, px0, c, cok);
    if constexpr (NUP > 2) adj3_row<2, HM>(a2, v, oy, p, n, b0, b1, px0, c, cok);
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = nv[i];
  }
  adj3_store<0>(a0, p, n, a0.cur - 1, b0, b1, px0, c, cok);
  if constexpr (NUP > 1) adj3_store<1>(a1, p, n, a1.cur - 1, b0, b1, px0, c, cok);
  if constexpr (NUP > 2) adj3_store<2>(a2, p, n, a2.cur - 1, b0, b1, px0, c, cok);
}

// ------------------------------------------------- channel-quad form ----
// The adjoint for up to 3 targets at exact 2, 4, 8 ratios (a fuse row's lower branches),
// one thread per (pixel, channel quad) so that narrow layers (18 channels) keep every
// lane busy: a horizontal pass of all targets (one launch) into a quad-padded workspace
// hb[s] = [n][H][zw][4Q], then a vertical pass of all targets (one launch), both with the
// static hat stencils.  dy is read once from HBM; hb (1/F of dy each) twice from L2.
struct UpAdjQ {
  const float* g;
  int64_t g_ps;
  int H, W, Q, C, nt;
  float* hb[3];
  float* dx[3];
  int64_t dx_ps[3];
  int zh[3], zw[3], lf[3];  // lf = log2 of the ratio (1..3)
  float beta[3];
  uint32_t cnt_h[3], cnt_v[3];
  FastDiv zwq[3], zh_d[3], q_d;
};

// sum_d hat_w(d, F) v[F*i + d] over a line of `len` points with stride `st`, edges folded.
// Every tap's load is unconditional (out-of-line taps read a clamped in-line point with
// weight 0): guarded loads were branched around one by one, each waited for in turn.
template <int F>
__device__ __forceinline__ f4 hat_adj(const float* line, int64_t st, int len, int i, int n_src) {
  constexpr int HF = F / 2;
  const int x0 = F * i;
  f4 v[4 * HF];
#pragma unroll
  for (int d = -HF; d < 3 * HF; ++d) {
    const int x = x0 + d;
    const int xc = x < 0 ? 0 : (x >= len ? len - 1 : x);
    v[d + HF] = *reinterpret_cast<const f4*>(line + xc * st);
  }
  f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int d = -HF; d < 3 * HF; ++d) {
    const int x = x0 + d;
    if (x >= 0 && x < len) acc += hat_w(d, F) * v[d + HF];
  }
  if (i == 0) {  // virtual source -1: points d - F
#pragma unroll
    for (int d = F; d < 3 * HF; ++d)
      acc += hat_w(d, F) * *reinterpret_cast<const f4*>(line + (d - F) * st);
  }
  if (i == n_src - 1) {  // virtual source n_src: points len + d
#pragma unroll
    for (int d = -HF; d < 0; ++d)
      acc += hat_w(d, F) * *reinterpret_cast<const f4*>(line + (len + d) * st);
  }
  return acc;
}

template <bool VERT>
__global__ __launch_bounds__(256) void up_adjq_kernel(UpAdjQ p) {
  const int s = blockIdx.y;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (VERT ? p.cnt_v[s] : p.cnt_h[s])) return;
  const int zw = p.zw[s], Q = p.Q, lf = p.lf[s];
  const uint32_t row = p.zwq[s].div(i);  // horizontal: n*H + oy; vertical: n*zh + iy
  const uint32_t r = i - row * (uint32_t)(zw * Q);
  const uint32_t ix = p.q_d.div(r);
  const uint32_t q = r - ix * (uint32_t)Q;
  const int64_t hrow = (int64_t)zw * 4 * Q;  // hb row stride
  if (!VERT) {
    const float* line = p.g + (int64_t)row * p.W * p.g_ps + 4 * q;
    const f4 acc = lf == 1   ? hat_adj<2>(line, p.g_ps, p.W, (int)ix, zw)
                   : lf == 2 ? hat_adj<4>(line, p.g_ps, p.W, (int)ix, zw)
                             : hat_adj<8>(line, p.g_ps, p.W, (int)ix, zw);
    *reinterpret_cast<f4*>(p.hb[s] + (int64_t)row * hrow + 4 * (ix * Q + q)) = acc;
    return;
  }
  const uint32_t n = p.zh_d[s].div(row);
  const int iy = (int)(row - n * (uint32_t)p.zh[s]);
  const float* line = p.hb[s] + (int64_t)n * p.H * hrow + 4 * (ix * Q + q);
  const f4 acc = lf == 1   ? hat_adj<2>(line, hrow, p.H, iy, p.zh[s])
                 : lf == 2 ? hat_adj<4>(line, hrow, p.H, iy, p.zh[s])
                           : hat_adj<8>(line, hrow, p.H, iy, p.zh[s]);
  float* dst = p.dx[s] + ((int64_t)row * zw + ix) * p.dx_ps[s] + 4 * q;
  const float beta = p.beta[s];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if ((int)(4 * q) + k < p.C) dst[k] = (beta != 0.f) ? acc[k] + beta * dst[k] : acc[k];
}

// Route, launch geometry and workspace of one multi-target adjoint: the size
// query and both launchers read it, so the workspace is sized as the kernels write.
enum class AdjRoute { OnePass, Pow2TwoPass, Generic };

struct AdjPlan {
  AdjRoute route;
  int br, nband;       // OnePass: dy rows per workgroup, bands per image
  size_t shm;          // Generic: LDS bytes of the horizontal pass (p.halo pixels each side)
  unsigned cb;         // 64-channel blocks
  dim3 grid;           // of the one-pass kernel / the horizontal pass
  int64_t hb[3], ws;   // workspace floats: offset of source s's hb, total (>= 1)
  UpAdj p;             // the kernels' argument, shapes filled in (pointers: fill_adj)
};

// Needs act_ok(dyd) and 0 <= n <= 3.  The launchers validate the targets.
static AdjPlan adj_plan(const vae2_act* dyd, int n, const vae2_act* dxds) {
  AdjPlan pl{};
  UpAdj& p = pl.p;
  p.dy_ps = (int)dyd->ps; p.H = (int)dyd->h; p.W = (int)dyd->w; p.C = (int)dyd->c;
  p.nxb = (int)ceil_div(dyd->w, kUsXB);
  pl.cb = (unsigned)ceil_div(dyd->c, 64);
  bool pow2 = dyd->w % kUsXB == 0, valid = n >= 1;  // pow2: exact 2^(s+1) ratios, whole chunks
  float min_sw = 1.f;
  for (int s = 0; s < n; ++s) {
    const vae2_act& d = dxds[s];
    valid = valid && act_ok(&d);
    pow2 = pow2 && valid && dyd->w == d.w << (s + 1) && dyd->h == d.h << (s + 1);
    p.zh[s] = (int)d.h; p.zw[s] = (int)d.w; p.dx_ps[s] = (int)d.ps;
    p.sh[s] = (float)d.h / (float)dyd->h; p.sw[s] = (float)d.w / (float)dyd->w;
    if (p.sw[s] > 0.f && p.sw[s] < min_sw) min_sw = p.sw[s];
    pl.hb[s] = pl.ws;
    pl.ws += dyd->n * dyd->h * d.w * dyd->c;
  }
  // the one-pass kernel addresses a dy row with 32-bit buffer offsets; it has no hb
  const bool one = g_adj_fused && pow2 && dyd->w * dyd->ps * 4 < (int64_t)kOOB;
  pl.route = one ? AdjRoute::OnePass : pow2 ? AdjRoute::Pow2TwoPass : AdjRoute::Generic;
  if (one || pl.ws < 1) pl.ws = 1;
  pl.br = dyd->h < g_adj_band ? (int)dyd->h : g_adj_band;
  pl.nband = (int)ceil_div(dyd->h, pl.br);
  pl.grid = dim3((unsigned)(dyd->n * (one ? pl.nband : dyd->h) * p.nxb * pl.cb));
  if (!pow2) {  // the owned columns' windows reach at most 1/sw + 3 pixels past the chunk
    p.halo = (int)ceilf(1.f / min_sw) + 4;
    pl.shm = (size_t)(4 * n + 64) * (kUsXB + 2 * p.halo) * sizeof(float);
  }
  return pl;
}

static void fill_adj(UpAdj& p, const AdjPlan& pl, const float* dy, int n, float* const* dxs,
                     const float* betas, float* ws) {
  p = pl.p; p.dy = dy;
  for (int s = 0; s < n; ++s) {
    p.dx[s] = dxs[s]; p.hb[s] = ws + pl.hb[s]; p.beta[s] = betas ? betas[s] : 0.f;
  }
}

// Kernel tables: [n - 1] targets of a launch, [s] the source of a vertical pass.
using AdjKernel = void (*)(UpAdj);
constexpr AdjKernel kAdjH[3] = {up_adj_h_kernel<1>, up_adj_h_kernel<2>, up_adj_h_kernel<3>};
constexpr AdjKernel kAdj2H[3] = {up_adj2_h_kernel<1>, up_adj2_h_kernel<2>, up_adj2_h_kernel<3>};
constexpr AdjKernel kAdj2V[3] = {up_adj2_v_kernel<0>, up_adj2_v_kernel<1>, up_adj2_v_kernel<2>};
constexpr void (*kAdj2VS[3])(UpAdj, FastDiv) = {up_adj2_vs_kernel<0>, up_adj2_vs_kernel<1>,
                                                up_adj2_vs_kernel<2>};
constexpr void (*kAdj3[3])(UpAdj, int, int) = {up_adj3_kernel<1>, up_adj3_kernel<2>,
                                               up_adj3_kernel<3>};

static int launch_adj3(const AdjPlan& pl, const UpAdj& p, int n, hipStream_t st, const char* fn) {
  VAE2_LAUNCH(kAdj3[n - 1], pl.grid, dim3(256), 0, st, p, pl.br, pl.nband);
  return check_launch(fn);
}

// log2 of an exact power-of-two ratio in {2, 4, 8}, else 0.
static int pow2_ratio(int64_t big, int64_t small) {
  for (int k = 1; k <= 3; ++k)
    if (big == small << k) return k;
  return 0;
}

}  // namespace vae2

using namespace vae2;

extern "C" {

int64_t vae2_upsample_bilinear_bwd_multi_ws_size(const vae2_act* dyd, int n,
                                                 const vae2_act* dxds) {
  if (!act_ok(dyd) || n < 0 || n > 3 || (n && !dxds)) return 0;
  return adj_plan(dyd, n, dxds).ws;
}

int vae2_upsample_bilinear_bwd_multi(const float* dy, const vae2_act* dyd, int n,
                                     float* const* dxs, const vae2_act* dxds, float* ws,
                                     int64_t ws_size, void* stream) {
  const char* fn = "vae2_upsample_bilinear_bwd_multi";
  VAE2_REQUIRE(dy && act_ok(dyd) && n >= 0 && n <= 3 && (n == 0 || (dxs && dxds)) && ws, fn,
               "bad arguments");
  const AdjPlan pl = adj_plan(dyd, n, dxds);
  VAE2_REQUIRE(ws_size >= pl.ws, fn, "workspace too small");
  if (n == 0) return 0;
  for (int s = 0; s < n; ++s) {
    const vae2_act* d = &dxds[s];
    VAE2_REQUIRE(dxs[s] && act_ok(d) && d->n == dyd->n && d->c == dyd->c && d->h <= dyd->h &&
                     d->w <= dyd->w, fn, "dx shape mismatch");
    VAE2_REQUIRE(2.f / ((float)d->h / (float)dyd->h) + 6.f <= 64.f, fn,
                 "upsampling ratio too large (> 24)");
  }
  UpAdj p;
  fill_adj(p, pl, dy, n, dxs, nullptr, ws);
  hipStream_t st = as_stream(stream);
  if (pl.route == AdjRoute::OnePass) return launch_adj3(pl, p, n, st, fn);
  const bool pow2 = pl.route == AdjRoute::Pow2TwoPass;
  VAE2_REQUIRE(pl.shm <= 64 * 1024, fn, "upsampling ratio too large for the LDS tile");
  VAE2_LAUNCH((pow2 ? kAdj2H : kAdjH)[n - 1], pl.grid, dim3(256), pl.shm, st, p);
  int rc = check_launch(fn);
  for (int s = 0; s < n && !rc; ++s) {
    const unsigned rows = (unsigned)(dyd->n * p.zh[s]);
    const int64_t rs = (int64_t)p.zw[s] * p.C;
    if (!pow2) {
      VAE2_LAUNCH(up_adj_v_kernel, dim3(rows, pl.cb), dim3(256), 0, st, p, s);
    } else if (rs % 4 == 0 && g_adj_stream) {
      VAE2_LAUNCH(kAdj2VS[s], dim3(rows, (unsigned)ceil_div(rs / 4, 512)), dim3(256), 0, st, p,
                  FastDiv((uint32_t)p.C));
    } else {
      VAE2_LAUNCH(kAdj2V[s], dim3(rows, pl.cb), dim3(256), 0, st, p);
    }
    rc = check_launch(fn);
  }
  return rc;
}

int64_t vae2_upsample_bilinear_bwd_pow2_ws_size(const vae2_act* dyd, int n,
                                                const vae2_act* dxds) {
  if (!act_ok(dyd) || n < 1 || n > 3 || !dxds) return -1;
  const int64_t Q = (dyd->c + 3) / 4;
  int64_t t = 0;
  for (int s = 0; s < n; ++s) {
    const vae2_act* d = &dxds[s];
    const int k = pow2_ratio(dyd->w, d->w);
    if (!act_ok(d) || !k || pow2_ratio(dyd->h, d->h) != k || d->n != dyd->n || d->c != dyd->c)
      return -1;
    t += dyd->n * dyd->h * d->w * 4 * Q;
  }
  return t;
}

int vae2_upsample_bilinear_bwd_pow2(const float* dy, const vae2_act* dyd, int n,
                                    float* const* dxs, const vae2_act* dxds,
                                    const float* betas, float* ws, int64_t ws_size,
                                    void* stream) {
  const char* fn = "vae2_upsample_bilinear_bwd_pow2";
  VAE2_REQUIRE(dy && act_ok(dyd) && n >= 1 && n <= 3 && dxs && dxds && ws, fn,
               "bad arguments");
  const int64_t need = vae2_upsample_bilinear_bwd_pow2_ws_size(dyd, n, dxds);
  VAE2_REQUIRE(need >= 0, fn, "targets are not exact 2 / 4 / 8 downsamplings of dy");
  VAE2_REQUIRE(ws_size >= need, fn, "workspace too small");
  VAE2_REQUIRE(dyd->ps % 4 == 0 && (uintptr_t)dy % 16 == 0 && (uintptr_t)ws % 16 == 0, fn,
               "dy and ws must be 16-byte aligned with a pixel stride of 4k");
  hipStream_t st = as_stream(stream);
  for (int s = 0; s < n; ++s) VAE2_REQUIRE(dxs[s], fn, "null target");
  // one launch, dy read once (the band kernel), where the plan's one-pass rules hold
  const AdjPlan pl = adj_plan(dyd, n, dxds);
  if (g_fuse_adj3 && pl.route == AdjRoute::OnePass) {
    UpAdj a;
    fill_adj(a, pl, dy, n, dxs, betas, ws);
    return launch_adj3(pl, a, n, st, fn);
  }
  UpAdjQ p{};
  p.g = dy; p.g_ps = dyd->ps; p.H = (int)dyd->h; p.W = (int)dyd->w; p.C = (int)dyd->c;
  p.Q = (p.C + 3) / 4; p.nt = n; p.q_d = FastDiv((uint32_t)p.Q);
  float* hb = ws;
  uint32_t mh = 0, mv = 0;
  for (int s = 0; s < n; ++s) {
    const vae2_act* d = &dxds[s];
    const int64_t ch = dyd->n * dyd->h * d->w * p.Q, cv = dyd->n * d->h * d->w * p.Q;
    VAE2_REQUIRE(ch < (int64_t(1) << 31), fn, "tensor too large");
    p.dx[s] = dxs[s]; p.dx_ps[s] = d->ps; p.zh[s] = (int)d->h; p.zw[s] = (int)d->w;
    p.lf[s] = pow2_ratio(dyd->w, d->w);
    p.beta[s] = betas ? betas[s] : 0.f;
    p.cnt_h[s] = (uint32_t)ch; p.cnt_v[s] = (uint32_t)cv;
    p.zwq[s] = FastDiv((uint32_t)(d->w * p.Q)); p.zh_d[s] = FastDiv((uint32_t)d->h);
    p.hb[s] = hb;
    hb += dyd->n * dyd->h * d->w * 4 * p.Q;
    if (p.cnt_h[s] > mh) mh = p.cnt_h[s];
    if (p.cnt_v[s] > mv) mv = p.cnt_v[s];
  }
  VAE2_LAUNCH(up_adjq_kernel<false>, dim3((mh + 255) / 256, n), dim3(256), 0, st, p);
  int rc = check_launch(fn);
  if (rc) return rc;
  VAE2_LAUNCH(up_adjq_kernel<true>, dim3((mv + 255) / 256, n), dim3(256), 0, st, p);
  return check_launch(fn);
}

}  // extern "C"

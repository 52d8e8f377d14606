// Differentiable SSIM reconstruction term (MI355X.SSIM_LAMBDA; not in the reference, whose
// trainer optimises L1 + KL (+ LSGAN) and only reports SSIM at evaluation):
//
//   loss = scale * sum_{n,c} sum_{valid pixels} (1 - ssim)      -> vae2_ssim_loss_fwd
//   dp (+)= d loss / d p * gout[0]                               -> vae2_ssim_loss_bwd
//
// with the SSIM map of oracle/metrics_ref.py::_ssim (pytorch_msssim 1.0.0: 11-tap Gaussian
// window, sigma 1.5, valid separable filtering) of u = a_c p + b_c and v = a_c t + b_c.  The
// formulas are in include/vae2_hip.h.  metrics.hip's vae2_ssim is the evaluation kernel
// (NCHW planes, per-plane means on the host, no gradient); these read the NHWC views of
// FullModel_encdec's predictions directly.
//
// Memory access: a workgroup stages a pixel tile of kCG = 3 consecutive channels (12
// contiguous bytes per pixel, the affine applied while staging) and loops over them;
// blockIdx.z = n * ceil(c / 3) + channel group.  All c = 9 channels of the backward's
// (16 + 20)^2 halo tile of both images would take 93 KiB of LDS; three take 31 KiB, which
// with the filtered maps keeps the kernel under 64 KiB (two workgroups per CU).
//
// Determinism: no atomics.  The forward writes one fp64 partial per workgroup and a single
// block sums them in a fixed order; the backward is a gather (each thread owns dp pixels).
//
// Arithmetic: fp32, in a form without the two cancellations of the textbook one.  With
// x = 1 - A1/B1 = (mu1 - mu2)^2 / B1 and y = 1 - A2/B2 = var_G(u - v) / B2,
//   1 - ssim = x + y (1 - x),
// so a prediction near its target gives a small number directly instead of 1 - 0.99...; and
// every window moment is taken of u - mu, v - mv (mu, mv: the means of u and v over the
// workgroup's staged tile, rounded to a multiple of 1/64), because a variance e11 - mu1^2
// of [0, 1] images is the difference of two numbers near 0.25 against C2 = 9e-4 (for data
// far below 1/64 in size the shifts are 0 and nothing changes).  The window's taps sum to
// 1 - 3.1e-8, not 1, so a shifted variance differs from the unshifted one by
// (S - 1) (b mu1 + a mu2 - a b S) (S: the squared tap sum; shifts a, b): that term is put
// back, which keeps the value the header's formulas define.  (The textbook form missed the
// forward test's bound, 4 x the error of an fp32 torch evaluation, on constant images and
// one noisy case, at up to 35 x; its backward passed.  DESIGN.md has the figures.)  The
// backward takes l = A1/B1 and cs = A2/B2 as written (with the moment of u'v'): its maps
// divide by them where they are small, and there 1 - x and 1 - y lose their digits.
//
// Exact zero: floating-point contraction is off in this file (every fused multiply-add is
// an explicit fmaf), so for p == t the differences above are 0, x = y = 0, the loss is 0.0
// and the three backward maps cancel exactly.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace vae2 {

constexpr int kTaps = 11;          // window taps
constexpr int kHalo = kTaps - 1;   // 10
constexpr int kCG = 3;             // channels staged per workgroup
// forward: (kFH x kFW) tile of the valid (h - 10) x (w - 10) map
constexpr int kFH = 16, kFW = 32;
constexpr int kFIH = kFH + kHalo, kFIW = kFW + kHalo;
// backward: (kBH x kBW) tile of dp; the three derivative maps on (kBH + 10) x (kBW + 10),
// u and v on (kBH + 20) x (kBW + 20)
constexpr int kBH = 16, kBW = 16;
constexpr int kBDH = kBH + kHalo, kBDW = kBW + kHalo;
constexpr int kBIH = kBH + 2 * kHalo, kBIW = kBW + 2 * kHalo;

// vae2/metrics.py::_win(device, 11, 1.5): exp(-(i - 5)^2 / 4.5) in fp32, normalised.
// (tests/test_ssim_loss_ref.py compares these literals with that function's values.)
struct SsimWin {
  float g[kTaps];
};
constexpr SsimWin kWindow = {{0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f,
                              0x1.b43c3ep-3f, 0x1.10656p-2f, 0x1.b43c3ep-3f, 0x1.bff0fep-4f,
                              0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d957p-10f}};
constexpr double tap_sum() {
  double s = 0.0;
  for (int i = 0; i < kTaps; ++i) s += (double)kWindow.g[i];
  return s;
}
constexpr double kS = tap_sum() * tap_sum();  // G * 1: what the 2-D window sums to
constexpr float kSf = (float)kS;
constexpr float kSm1 = (float)(kS - 1.0);     // -6.1e-8

__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) s = red[0] + red[1] + red[2] + red[3];
  return s;  // valid in thread 0
}

struct SsimGroup {
  int64_t n;        // image
  int c0, ncg;      // first channel and channel count (1..kCG) of this workgroup
  float ca[kCG], cb[kCG];
};

__device__ __forceinline__ SsimGroup group_of(int64_t c, const float* __restrict__ a,
                                          const float* __restrict__ b) {
  const int groups = (int)((c + kCG - 1) / kCG);
  SsimGroup g;
  g.n = blockIdx.z / groups;
  g.c0 = (int)(blockIdx.z % groups) * kCG;
  g.ncg = (int)c - g.c0 < kCG ? (int)c - g.c0 : kCG;
#pragma unroll
  for (int j = 0; j < kCG; ++j) {
    const bool ok = j < g.ncg;
    g.ca[j] = (ok && a) ? a[g.c0 + j] : 1.f;
    g.cb[j] = (ok && b) ? b[g.c0 + j] : 0.f;
  }
  return g;
}

// u = a_c p + b_c and v = a_c t + b_c of the IH x IW pixel tile whose first pixel is
// (gy0, gx0) (may be negative), kCG channels interleaved; 0 outside the image / group.
template <int IH, int IW, int LD>
__device__ __forceinline__ void stage(const float* __restrict__ p, const Act& pd,
                                      const float* __restrict__ t, const Act& td,
                                      const SsimGroup& g, int gy0, int gx0, float (*su)[LD],
                                      float (*sv)[LD]) {
  const int h = (int)pd.h, w = (int)pd.w;
  for (int i = threadIdx.x; i < IH * IW; i += 256) {
    const int r = i / IW, col = i - r * IW;
    const int gy = gy0 + r, gx = gx0 + col;
    const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
    const int64_t px = (g.n * h + gy) * w + gx;
    const float* pp = p + px * pd.ps + g.c0;
    const float* tp = t + px * td.ps + g.c0;
#pragma unroll
    for (int j = 0; j < kCG; ++j) {
      const bool ok = in && j < g.ncg;
      const float pv = ok ? pp[j] : 0.f, tv = ok ? tp[j] : 0.f;
      su[r][col * kCG + j] = ok ? fmaf(g.ca[j], pv, g.cb[j]) : 0.f;
      sv[r][col * kCG + j] = ok ? fmaf(g.ca[j], tv, g.cb[j]) : 0.f;
    }
  }
}

// The shifts of channel ch: the means of u and v over the staged tile's `count` in-image
// pixels (the staged zeros outside the image add nothing; fp64 sums), rounded to a multiple
// of 1/64 so that u - mu is exact for data of order 1: an unrounded mean near 0 made every
// shifted value carry a rounding error of its own, and the backward 2.3 x less accurate
// than without a shift.  Every thread gets the same values.
template <int IH, int IW, int LD>
__device__ __forceinline__ void tile_means(const float (*su)[LD], const float (*sv)[LD], int ch,
                                           int count, double (*red)[4], float* mu, float* mv) {
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < IH * IW; i += 256) {
    const int r = i / IW, col = i - r * IW;
    a += (double)su[r][col * kCG + ch];
    b += (double)sv[r][col * kCG + ch];
  }
  a = wave_sum_d(a);
  b = wave_sum_d(b);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  const float ma = (float)((red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (double)count);
  const float mb = (float)((red[1][0] + red[1][1] + red[1][2] + red[1][3]) / (double)count);
  *mu = rintf(ma * 64.f) * 0.015625f;
  *mv = rintf(mb * 64.f) * 0.015625f;
}

// in-image pixels of the IH x IW tile at (gy0, gx0)
__device__ __forceinline__ int tile_count(int gy0, int gx0, int IH, int IW, int h, int w) {
  const int y1 = gy0 + IH < h ? gy0 + IH : h, x1 = gx0 + IW < w ? gx0 + IW : w;
  return (y1 - (gy0 > 0 ? gy0 : 0)) * (x1 - (gx0 > 0 ? gx0 : 0));
}

// hf[m][r][col] = sum_k g[k] f_m[r][col + k], f = (u', v', u'^2, v'^2, w) of the shifted
// u' = u - mu, v' = v - mv, channel ch; w = (u' - v')^2 (DIFF: the forward) or u' v'
template <int IH, int OW, int LD, int LDH, bool DIFF>
__device__ __forceinline__ void filter_rows(const float (*su)[LD], const float (*sv)[LD],
                                            int ch, float mu, float mv, const SsimWin& win,
                                            float (*hf)[IH][LDH]) {
  for (int i = threadIdx.x; i < IH * OW; i += 256) {
    const int r = i / OW, col = i - r * OW;
    float a1 = 0.f, a2 = 0.f, a11 = 0.f, a22 = 0.f, add = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float gk = win.g[k];
      const float u = su[r][(col + k) * kCG + ch] - mu, v = sv[r][(col + k) * kCG + ch] - mv;
      const float d = u - v;
      a1 = fmaf(gk, u, a1);
      a2 = fmaf(gk, v, a2);
      a11 = fmaf(gk, u * u, a11);
      a22 = fmaf(gk, v * v, a22);
      add = fmaf(gk, DIFF ? d * d : u * v, add);
    }
    hf[0][r][col] = a1;
    hf[1][r][col] = a2;
    hf[2][r][col] = a11;
    hf[3][r][col] = a22;
    hf[4][r][col] = add;
  }
}

struct SsimMoments {
  float m1, m2, e11, e22, edd;  // of the shifted u', v'; edd: of (u' - v')^2 or of u' v'
};

template <int IH, int LDH>
__device__ __forceinline__ SsimMoments filter_cols(const float (*hf)[IH][LDH], int r, int col,
                                                   const SsimWin& win) {
  SsimMoments q = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < kTaps; ++k) {
    const float gk = win.g[k];
    q.m1 = fmaf(gk, hf[0][r + k][col], q.m1);
    q.m2 = fmaf(gk, hf[1][r + k][col], q.m2);
    q.e11 = fmaf(gk, hf[2][r + k][col], q.e11);
    q.e22 = fmaf(gk, hf[3][r + k][col], q.e22);
    q.edd = fmaf(gk, hf[4][r + k][col], q.edd);
  }
  return q;
}

// What a (co)variance of functions shifted by a and b has too much, the window summing to
// S rather than 1: (S - 1) (b mx + a my - a b S), mx and my the unshifted window means.
__device__ __forceinline__ float shift_term(float a, float b, float mx, float my) {
  return kSm1 * ((b * mx + a * my) - (a * b) * kSf);
}

// The terms of the SSIM map at one valid pixel.  DIFF (the forward, its fifth moment that of
// (u' - v')^2): x = 1 - A1/B1, y = 1 - A2/B2 and l = 1 - x, so 1 - ssim = x + y l.  Else (the
// backward, fifth moment that of u' v'): l = A1/B1 and cs = A2/B2 as written, each accurate
// where it is small, and x.  Both: the unshifted means and the denominators.
struct SsimTerms {
  float x, y, l, cs, mu1, mu2, b1, b2;
};

template <bool DIFF>
__device__ __forceinline__ SsimTerms ssim_terms(const SsimMoments& q, float mu, float mv,
                                                float C1, float C2) {
  SsimTerms t;
  t.mu1 = fmaf(mu, kSf, q.m1);
  t.mu2 = fmaf(mv, kSf, q.m2);
  const float s1 = (q.e11 - q.m1 * q.m1) - shift_term(mu, mu, t.mu1, t.mu1);
  const float s2 = (q.e22 - q.m2 * q.m2) - shift_term(mv, mv, t.mu2, t.mu2);
  const float dmu = t.mu1 - t.mu2;
  t.b1 = (t.mu1 * t.mu1 + t.mu2 * t.mu2) + C1;
  t.b2 = (s1 + s2) + C2;
  t.x = (dmu * dmu) / t.b1;
  if (DIFF) {
    const float md = q.m1 - q.m2, dsh = mu - mv;
    const float sdd = (q.edd - md * md) - shift_term(dsh, dsh, dmu, dmu);
    t.y = sdd / t.b2;
    t.l = 1.f - t.x;
    t.cs = 1.f - t.y;
  } else {
    const float s12 = (q.edd - q.m1 * q.m2) - shift_term(mu, mv, t.mu1, t.mu2);
    t.l = (2.f * (t.mu1 * t.mu2) + C1) / t.b1;
    t.cs = (2.f * s12 + C2) / t.b2;
    t.y = 0.f;
  }
  return t;
}

__global__ __launch_bounds__(256) void ssim_loss_fwd_kernel(
    const float* __restrict__ p, Act pd, const float* __restrict__ t, Act td,
    const float* __restrict__ a, const float* __restrict__ b, float C1, float C2, SsimWin win,
    double* __restrict__ part) {
  constexpr int LD = kFIW * kCG + 1;
  __shared__ float su[kFIH][LD];
  __shared__ float sv[kFIH][LD];
  __shared__ float hf[5][kFIH][kFW + 1];
  __shared__ double red[2][4];
  const int ho = (int)pd.h - kHalo, wo = (int)pd.w - kHalo;
  const int x0 = blockIdx.x * kFW, y0 = blockIdx.y * kFH;
  const SsimGroup g = group_of(pd.c, a, b);
  const int count = tile_count(y0, x0, kFIH, kFIW, (int)pd.h, (int)pd.w);
  stage<kFIH, kFIW, LD>(p, pd, t, td, g, y0, x0, su, sv);
  __syncthreads();
  double acc = 0.0;
  for (int ch = 0; ch < g.ncg; ++ch) {
    float mu, mv;
    tile_means<kFIH, kFIW, LD>(su, sv, ch, count, red, &mu, &mv);
    filter_rows<kFIH, kFW, LD, kFW + 1, true>(su, sv, ch, mu, mv, win, hf);
    __syncthreads();
    for (int i = threadIdx.x; i < kFH * kFW; i += 256) {
      const int r = i / kFW, col = i - r * kFW;
      if (y0 + r >= ho || x0 + col >= wo) continue;
      const SsimTerms s =
          ssim_terms<true>(filter_cols<kFIH, kFW + 1>(hf, r, col, win), mu, mv, C1, C2);
      acc += (double)(s.x + s.y * s.l);
    }
    __syncthreads();
  }
  acc = block_sum_d(acc, red[0]);
  if (threadIdx.x == 0)
    part[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = acc;
}

// out[0] = scale * sum(part[0..count))   (single block, fixed order)
__global__ __launch_bounds__(256) void ssim_loss_finish_kernel(const double* __restrict__ part,
                                                               int64_t count, float scale,
                                                               float* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) s += part[i];
  s = block_sum_d(s, red);
  if (threadIdx.x == 0) out[0] = (float)(s * (double)scale);
}

__global__ __launch_bounds__(256) void ssim_loss_bwd_kernel(
    const float* __restrict__ p, Act pd, const float* __restrict__ t, Act td,
    const float* __restrict__ a, const float* __restrict__ b, float C1, float C2,
    const float* __restrict__ gout, float scale, float* __restrict__ dp, Act dpd, float beta,
    SsimWin win) {
  constexpr int LD = kBIW * kCG + 1;
  __shared__ float su[kBIH][LD];
  __shared__ float sv[kBIH][LD];
  __shared__ float hf[5][kBIH][kBDW + 1];
  __shared__ float dm[3][kBDH][kBDW + 1];
  __shared__ double red[2][4];
  // the horizontally back-filtered maps reuse hf (3 * 26 * 17 floats of its 5 * 36 * 27)
  float(*tt)[kBDH][kBW + 1] = reinterpret_cast<float(*)[kBDH][kBW + 1]>(&hf[0][0][0]);
  const int h = (int)pd.h, w = (int)pd.w;
  const int ho = h - kHalo, wo = w - kHalo;
  const int x0 = blockIdx.x * kBW, y0 = blockIdx.y * kBH;
  const SsimGroup g = group_of(pd.c, a, b);
  const float coef = -(scale * gout[0]);
  const int count = tile_count(y0 - kHalo, x0 - kHalo, kBIH, kBIW, h, w);
  stage<kBIH, kBIW, LD>(p, pd, t, td, g, y0 - kHalo, x0 - kHalo, su, sv);
  __syncthreads();
  for (int ch = 0; ch < g.ncg; ++ch) {
    float mu, mv;
    tile_means<kBIH, kBIW, LD>(su, sv, ch, count, red, &mu, &mv);
    filter_rows<kBIH, kBDW, LD, kBDW + 1, false>(su, sv, ch, mu, mv, win, hf);
    __syncthreads();
    // D_mu, D_11, D_12 at the valid-map position (y0 - 10 + r, x0 - 10 + col); 0 outside
    for (int i = threadIdx.x; i < kBDH * kBDW; i += 256) {
      const int r = i / kBDW, col = i - r * kBDW;
      const int oy = y0 - kHalo + r, ox = x0 - kHalo + col;
      float dmu = 0.f, d11 = 0.f, d12 = 0.f;
      if (oy >= 0 && oy < ho && ox >= 0 && ox < wo) {
        const SsimTerms s =
            ssim_terms<false>(filter_cols<kBIH, kBDW + 1>(hf, r, col, win), mu, mv, C1, C2);
        d11 = -(s.l * s.cs) / s.b2;
        d12 = (2.f * s.l) / s.b2;
        // mu2 - mu1 l = mu1 x - (mu1 - mu2)
        dmu = s.cs * (2.f * (s.mu1 * s.x - (s.mu1 - s.mu2))) / s.b1 - (2.f * s.mu1) * d11 -
              s.mu2 * d12;
      }
      dm[0][r][col] = dmu;
      dm[1][r][col] = d11;
      dm[2][r][col] = d12;
    }
    __syncthreads();
    // transposed window along x: tt[m][r][x] = sum_j g[j] dm[m][r][x + 10 - j]
    for (int i = threadIdx.x; i < kBDH * kBW; i += 256) {
      const int r = i / kBW, x = i - r * kBW;
      float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int j = 0; j < kTaps; ++j) {
        const float gj = win.g[j];
        t0 = fmaf(gj, dm[0][r][x + kHalo - j], t0);
        t1 = fmaf(gj, dm[1][r][x + kHalo - j], t1);
        t2 = fmaf(gj, dm[2][r][x + kHalo - j], t2);
      }
      tt[0][r][x] = t0;
      tt[1][r][x] = t1;
      tt[2][r][x] = t2;
    }
    __syncthreads();
    // transposed window along y, then the chain rule through mu1, e11, e12
    {
      const int y = threadIdx.x / kBW, x = threadIdx.x - y * kBW;  // kBH * kBW == 256
      const int gy = y0 + y, gx = x0 + x;
      if (gy < h && gx < w) {
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
        for (int j = 0; j < kTaps; ++j) {
          const float gj = win.g[j];
          r0 = fmaf(gj, tt[0][y + kHalo - j][x], r0);
          r1 = fmaf(gj, tt[1][y + kHalo - j][x], r1);
          r2 = fmaf(gj, tt[2][y + kHalo - j][x], r2);
        }
        const float u = su[y + kHalo][(x + kHalo) * kCG + ch];
        const float v = sv[y + kHalo][(x + kHalo) * kCG + ch];
        const float ac = ch == 0 ? g.ca[0] : (ch == 1 ? g.ca[1] : g.ca[2]);
        const float val = (coef * ac) * (r0 + ((2.f * u) * r1 + v * r2));
        float* dst = dp + ((g.n * h + gy) * w + gx) * dpd.ps + g.c0 + ch;
        *dst = (beta != 0.f) ? val + beta * *dst : val;
      }
    }
    __syncthreads();
  }
}

static_assert(kBH * kBW == 256, "one dp pixel per thread");
static_assert(3 * kBDH * (kBW + 1) <= 5 * kBIH * (kBDW + 1), "tt fits in hf");

struct SsimPlan {
  int64_t groups, planes, fx, fy, bx, by;
};

// Shared argument rules of the three entry points; nullptr when they hold.
static const char* check_views(const vae2_act* pd, const vae2_act* td, SsimPlan* pl) {
  if (!pd || !td) return "null descriptor";
  for (const vae2_act* d : {pd, td}) {
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0) return "bad descriptor";
    if (d->ps < d->c) return "pixel stride below the channel count";
  }
  if (!same_shape(pd, td)) return "predict / target shape mismatch";
  if (pd->h < kTaps || pd->w < kTaps) return "frame sides must be >= 11 (the window)";
  if (!idx32_ok(pd)) return kTooLarge;
  pl->groups = ceil_div(pd->c, kCG);
  pl->planes = pd->n * pl->groups;
  pl->fx = ceil_div(pd->w - kHalo, kFW);
  pl->fy = ceil_div(pd->h - kHalo, kFH);
  pl->bx = ceil_div(pd->w, kBW);
  pl->by = ceil_div(pd->h, kBH);
  if (pl->planes > 65535 || pl->by > 65535)
    return "too many planes: n * ceil(c / 3) and ceil(h / 16) must be <= 65535";
  return nullptr;
}

static const char* check_consts(const float* a, const float* b, float c1, float c2) {
  if ((a == nullptr) != (b == nullptr)) return "a and b must be given together";
  if (!(std::isfinite(c1) && std::isfinite(c2) && c1 > 0.f && c2 > 0.f))
    return "c1 and c2 must be finite and > 0";
  return nullptr;
}

}  // namespace vae2

using namespace vae2;

extern "C" {

int64_t vae2_ssim_loss_ws_size(const vae2_act* pd) {
  SsimPlan pl;
  if (check_views(pd, pd, &pl)) return 1;
  return pl.planes * pl.fx * pl.fy;
}

int vae2_ssim_loss_fwd(const float* p, const vae2_act* pd, const float* t, const vae2_act* td,
                       const float* a, const float* b, float c1, float c2, float scale,
                       double* ws, float* out, void* stream) {
  const char* fn = "vae2_ssim_loss_fwd";
  VAE2_REQUIRE(p && t && ws && out, fn, "null pointer");
  SsimPlan pl;
  const char* err = check_views(pd, td, &pl);
  VAE2_REQUIRE(!err, fn, err);
  err = check_consts(a, b, c1, c2);
  VAE2_REQUIRE(!err, fn, err);
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)pl.fx, (unsigned)pl.fy, (unsigned)pl.planes);
  VAE2_LAUNCH(ssim_loss_fwd_kernel, grid, dim3(256), 0, s, p, to_act(pd), t, to_act(td), a, b,
              c1, c2, kWindow, ws);
  int rc = check_launch(fn);
  if (rc) return rc;
  VAE2_LAUNCH(ssim_loss_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)ws,
              pl.planes * pl.fx * pl.fy, scale, out);
  return check_launch(fn);
}

int vae2_ssim_loss_bwd(const float* p, const vae2_act* pd, const float* t, const vae2_act* td,
                       const float* a, const float* b, float c1, float c2, const float* gout,
                       float scale, float* dp, const vae2_act* dpd, float beta, void* stream) {
  const char* fn = "vae2_ssim_loss_bwd";
  VAE2_REQUIRE(p && t && gout && dp, fn, "null pointer");
  SsimPlan pl;
  const char* err = check_views(pd, td, &pl);
  VAE2_REQUIRE(!err, fn, err);
  VAE2_REQUIRE(dpd && dpd->ps >= dpd->c, fn, "dp: pixel stride below the channel count");
  VAE2_REQUIRE(same_shape(dpd, pd), fn, "dp shape mismatch");
  err = check_consts(a, b, c1, c2);
  VAE2_REQUIRE(!err, fn, err);
  VAE2_REQUIRE(beta == 0.f || beta == 1.f, fn, "beta must be 0 or 1");
  const dim3 grid((unsigned)pl.bx, (unsigned)pl.by, (unsigned)pl.planes);
  VAE2_LAUNCH(ssim_loss_bwd_kernel, grid, dim3(256), 0, as_stream(stream), p, to_act(pd), t,
              to_act(td), a, b, c1, c2, gout, scale, dp, to_act(dpd), beta, kWindow);
  return check_launch(fn);
}

}  // extern "C"

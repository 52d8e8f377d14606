// Output stage of the HRNet heads: BatchNorm-apply + ReLU + the final narrow 1x1 conv
// (270 -> NUM_CLASSES), forward and backward, without materialising the ReLU output.
//
//   last_layer = Conv1x1(C->C, bias) -> BatchNorm2d -> ReLU -> Conv1x1(C->CO, bias)
//   (enc_hrnet.py:323-370 / :598-750; applied at :839-847, :897-905, :955-963)
//
// The wide 1x1 conv itself runs per branch (vae2_conv2d_fwd at the branch resolution,
// then upsum_kernel below: full-resolution block + upsampled branch terms + bias + BN
// statistics); the output-stage kernels take its pre-BN output y, the BN coefficients and
//   forward   out[p][o] = b2[o] + sum_c w2[o][c] * relu(y[p][c]*scale[c] + shift[c])
//   backward  g[p][c]  = (sum_o w2[o][c] * dout[p][o]) * [h > 0]      (h = ReLU input)
//             reduce:  sum_p g, sum_p g*xhat (BN backward sums), dW2, db2
//             apply:   dy = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)), sum_p dy (conv bias)
// Each pass reads y once (16-byte NHWC quads); h and g are recomputed in registers.
// Reductions are two-level with fixed orders (deterministic).
#include "heads.h"

namespace vae2 {

constexpr int kHeadMaxOut = 4;
constexpr int64_t kHeadMaxPpb = 2048;  // pixels per block of the backward passes (LDS dout)

// The block's dout rows [p0, p1) x CO, staged once in LDS (every channel quad of a pixel
// reads the same CO values: one coalesced pass instead of CO scalar loads per quad)
template <int CO>
__device__ __forceinline__ void head_stage_dout(float* sd, const float* dout, const Act& dod,
                                                int64_t p0, int64_t p1) {
  const int n = (int)(p1 - p0) * CO;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int pp = i / CO, o = i - pp * CO;
    sd[i] = dout[(p0 + pp) * dod.ps + o];
  }
}

__device__ __forceinline__ f4 hld4(const float* p) { return *reinterpret_cast<const f4*>(p); }

// The wide conv's output y lives in a 64-channel-blocked layout ("B64"):
//   element (p, c) at y[(c / 64) * P * 64 + p * 64 + c % 64],  P = N*H*W pixels,
// so a workgroup producing a 64-channel block of a pixel run writes one contiguous
// region (NHWC rows of C = 270 would be written in partial 128-byte lines).
__device__ __forceinline__ const float* yb_at(const float* y, int64_t P, int64_t p, int c) {
  return y + (int64_t)(c >> 6) * P * 64 + p * 64 + (c & 63);
}

__device__ __forceinline__ f4 hchan4(const float* a, int c, int C) {
  f4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (c + k < C) ? a[c + k] : 0.f;
  return v;
}

// Forward: 16 lanes per pixel (lane l takes channel quads l, l+16, ...), 16 pixels per
// block pass; the per-channel coefficients and W2 live in LDS as quads.
template <int CO>
__global__ __launch_bounds__(256) void head_out_fwd_kernel(
    const float* __restrict__ y, Act yd, const float* __restrict__ save,
    const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out,
    Act od) {
  extern __shared__ __attribute__((aligned(16))) float hsm[];
  const int C = (int)yd.c, c4 = (C + 3) >> 2;
  f4* ssc = reinterpret_cast<f4*>(hsm);
  f4* ssh = ssc + c4;
  f4* sw = ssh + c4;  // [CO][c4]
  for (int q = threadIdx.x; q < c4; q += 256) {
    ssc[q] = hchan4(save + 2 * C, 4 * q, C);
    ssh[q] = hchan4(save + 3 * C, 4 * q, C);
#pragma unroll
    for (int o = 0; o < CO; ++o) sw[o * c4 + q] = hchan4(w2 + (int64_t)o * C, 4 * q, C);
  }
  __syncthreads();
  const int l = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int64_t P = yd.n * yd.h * yd.w;
  for (int64_t p = (int64_t)blockIdx.x * 16 + grp; p < P; p += (int64_t)gridDim.x * 16) {
    float acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = 0.f;
    // up to kHeadQU quads per lane with their loads in flight together (the same
    // quad order as one at a time)
    constexpr int kHeadQU = 5;
    for (int q0 = l; q0 < c4; q0 += 16 * kHeadQU) {
      f4 vv[kHeadQU];
#pragma unroll
      for (int u = 0; u < kHeadQU; ++u) {
        const int q = q0 + 16 * u;
        vv[u] = q < c4 ? hld4(yb_at(y, P, p, 4 * q)) : f4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < kHeadQU; ++u) {
        const int q = q0 + 16 * u;
        if (q >= c4) break;
        const f4 v = vv[u];
        const f4 a = ssc[q], b = ssh[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float h = __builtin_fmaf(v[k], a[k], b[k]);
          h = (4 * q + k < C && !(h < 0.f)) ? h : 0.f;  // NaN propagates
#pragma unroll
          for (int o = 0; o < CO; ++o) acc[o] += h * sw[o * c4 + q][k];
        }
      }
    }
#pragma unroll
    for (int o = 0; o < CO; ++o) {
      acc[o] += __shfl_xor(acc[o], 8, 16);
      acc[o] += __shfl_xor(acc[o], 4, 16);
      acc[o] += __shfl_xor(acc[o], 2, 16);
      acc[o] += __shfl_xor(acc[o], 1, 16);
    }
    if (l == 0) {
#pragma unroll
      for (int o = 0; o < CO; ++o) out[p * od.ps + o] = acc[o] + (b2 ? b2[o] : 0.f);
    }
  }
}

// Per-thread state of the backward passes: thread (r, q) owns channels 4q..4q+3 and
// walks pixels p0 + r, p0 + r + rows, ... of its block's pixel range.
struct HeadCoef {
  f4 mean, invstd, sc, sh;
};

__device__ __forceinline__ HeadCoef head_coef(const float* save, int c, int C) {
  HeadCoef h;
  h.mean = hchan4(save, c, C);
  h.invstd = hchan4(save + C, c, C);
  h.sc = hchan4(save + 2 * C, c, C);
  h.sh = hchan4(save + 3 * C, c, C);
  return h;
}

// Partial-row columns: [0,C) sum g | [C,2C) sum g*xhat | [2C, 2C+CO*C) dW2[o][c] | CO x db2
template <int CO, int U = 2>
__global__ __launch_bounds__(256) void head_out_bwd_reduce_kernel(
    const float* __restrict__ y, Act yd, const float* __restrict__ save,
    const float* __restrict__ w2, const float* __restrict__ dout, Act dod, int64_t ppb,
    int rows, float* __restrict__ part) {
  extern __shared__ float red[];  // [rows][NC], then the dout rows [ppb][CO]
  const int C = (int)yd.c, c4 = (C + 3) >> 2;
  const int NC = 2 * C + CO * C + CO;
  const int tid = threadIdx.x;
  const int64_t P = yd.n * yd.h * yd.w;
  const int64_t p0 = blockIdx.x * ppb;
  const int64_t p1 = p0 + ppb < P ? p0 + ppb : P;
  const int r = tid / c4, q = tid - r * c4, c = 4 * q;
  float* sd = red + rows * NC;
  head_stage_dout<CO>(sd, dout, dod, p0, p1);
  __syncthreads();
  if (tid < rows * c4) {
    const HeadCoef hc = head_coef(save, c, C);
    f4 wv[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) wv[o] = hchan4(w2 + (int64_t)o * C, c, C);
    f4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    f4 dw[CO];
    float db[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) { dw[o] = s0; db[o] = 0.f; }
    // U pixels in flight per thread (2: 4 waves/SIMD, 120 -> 95 us per head in round 2)
    for (int64_t pb = p0 + r; pb < p1; pb += U * rows) {
      f4 vv[U];
      float dd[U][CO];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = pb + u * rows;
        const bool ok = p < p1;
        vv[u] = ok ? hld4(yb_at(y, P, p, c)) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int o = 0; o < CO; ++o) dd[u][o] = ok ? sd[(p - p0) * CO + o] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const f4 v = vv[u];
        const float* d = dd[u];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float h = __builtin_fmaf(v[k], hc.sc[k], hc.sh[k]);
          const bool m = h > 0.f;
          h = m ? h : 0.f;
          float dh = 0.f;
#pragma unroll
          for (int o = 0; o < CO; ++o) dh += wv[o][k] * d[o];
          const float g = m ? dh : 0.f;
          s0[k] += g;
          s1[k] += g * (v[k] - hc.mean[k]) * hc.invstd[k];
#pragma unroll
          for (int o = 0; o < CO; ++o) dw[o][k] += d[o] * h;
        }
#pragma unroll
        for (int o = 0; o < CO; ++o) db[o] += d[o];
      }
    }
    float* rr = red + r * NC;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (c + k >= C) break;
      rr[c + k] = s0[k];
      rr[C + c + k] = s1[k];
#pragma unroll
      for (int o = 0; o < CO; ++o) rr[2 * C + o * C + c + k] = dw[o][k];
    }
    if (q == 0) {
#pragma unroll
      for (int o = 0; o < CO; ++o) rr[2 * C + CO * C + o] = db[o];
    }
  }
  __syncthreads();
  for (int col = tid; col < NC; col += 256) {
    float a = 0.f;
    for (int i = 0; i < rows; ++i) a += red[i * NC + col];
    part[(int64_t)blockIdx.x * NC + col] = a;
  }
}

// Column sums of the reduce partials (lane = column; 16 waves over rows with four
// independent accumulators each, in double; combined in a fixed order) routed to their
// destinations.
__global__ __launch_bounds__(1024) void head_bwd_colsum_kernel(
    const float* __restrict__ part, int nrows, int C, int CO, double* __restrict__ sums,
    float* dgamma, float* dbeta, float* dw2, float* db2) {
  __shared__ double red[16][64];
  const int NC = 2 * C + CO * C + CO;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (col < NC) {
    int i = wave;
    for (; i + 48 < nrows; i += 64) {
      s0 += (double)part[(int64_t)i * NC + col];
      s1 += (double)part[(int64_t)(i + 16) * NC + col];
      s2 += (double)part[(int64_t)(i + 32) * NC + col];
      s3 += (double)part[(int64_t)(i + 48) * NC + col];
    }
    for (; i < nrows; i += 16) s0 += (double)part[(int64_t)i * NC + col];
  }
  red[wave][lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (wave != 0 || col >= NC) return;
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < 16; ++w) s += red[w][lane];
  if (col < C) {
    sums[col] = s;
    if (dbeta) dbeta[col] += (float)s;
  } else if (col < 2 * C) {
    sums[col] = s;
    if (dgamma) dgamma[col - C] += (float)s;
  } else if (col < 2 * C + CO * C) {
    if (dw2) dw2[col - 2 * C] += (float)s;
  } else {
    if (db2) db2[col - 2 * C - CO * C] += (float)s;
  }
}

// dy = gamma*invstd*(g - sum_g/count - xhat*sum_gxhat/count); partial rows [block][C]
// of sum_p dy (the wide conv's bias gradient).
template <int CO, int U = 2>
__global__ __launch_bounds__(256) void head_out_bwd_apply_kernel(
    const float* __restrict__ y, Act yd, const float* __restrict__ save,
    const float* __restrict__ gamma, const float* __restrict__ w2,
    const float* __restrict__ dout, Act dod, const double* __restrict__ sums, double count,
    int64_t ppb, int rows, float* __restrict__ dy, Act dyd, float* __restrict__ part) {
  extern __shared__ float red[];  // [rows][C], then the dout rows [ppb][CO]
  const int C = (int)yd.c, c4 = (C + 3) >> 2;
  const int tid = threadIdx.x;
  const int64_t P = yd.n * yd.h * yd.w;
  const int64_t p0 = blockIdx.x * ppb;
  const int64_t p1 = p0 + ppb < P ? p0 + ppb : P;
  const int r = tid / c4, q = tid - r * c4, c = 4 * q;
  float* sd = red + rows * C;
  head_stage_dout<CO>(sd, dout, dod, p0, p1);
  __syncthreads();
  if (tid < rows * c4) {
    const HeadCoef hc = head_coef(save, c, C);
    const float inv_n = (float)(1.0 / count);
    f4 wv[CO], mg, mgx, k4;
#pragma unroll
    for (int o = 0; o < CO; ++o) wv[o] = hchan4(w2 + (int64_t)o * C, c, C);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ch = c + k < C ? c + k : C - 1;
      mg[k] = (float)sums[ch] * inv_n;
      mgx[k] = (float)sums[C + ch] * inv_n;
      k4[k] = (gamma ? gamma[ch] : 1.f) * hc.invstd[k];
    }
    f4 sdy = {0.f, 0.f, 0.f, 0.f};
    // U pixels in flight per thread
    // the next U pixels' y loads go out before this group's dy stores (vmcnt counts
    // stores too: loads issued after them would wait for them)
    f4 nv[U];
    auto ldy = [&](int64_t pb) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = pb + u * rows;
        nv[u] = p < p1 ? hld4(yb_at(y, P, p, c)) : f4{0.f, 0.f, 0.f, 0.f};
      }
    };
    ldy(p0 + r);
    for (int64_t pb = p0 + r; pb < p1; pb += U * rows) {
      f4 vv[U];
      float dd[U][CO];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = pb + u * rows;
        const bool ok = p < p1;
        vv[u] = nv[u];
#pragma unroll
        for (int o = 0; o < CO; ++o) dd[u][o] = ok ? sd[(p - p0) * CO + o] : 0.f;
      }
      if (pb + U * rows < p1) ldy(pb + U * rows);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = pb + u * rows;
        if (p >= p1) break;
        const f4 v = vv[u];
        f4 o4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float h = __builtin_fmaf(v[k], hc.sc[k], hc.sh[k]);
          float dh = 0.f;
#pragma unroll
          for (int o = 0; o < CO; ++o) dh += wv[o][k] * dd[u][o];
          const float g = h > 0.f ? dh : 0.f;
          const float xh = (v[k] - hc.mean[k]) * hc.invstd[k];
          o4[k] = k4[k] * (g - mg[k] - xh * mgx[k]);
          sdy[k] += o4[k];
        }
        float* dst = dy + p * dyd.ps + c;
        if (c + 4 <= C) {
          *reinterpret_cast<f4*>(dst) = o4;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (c + k < C) dst[k] = o4[k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c + k < C) red[r * C + c + k] = sdy[k];
  }
  __syncthreads();
  for (int ch = tid; ch < C; ch += 256) {
    float a = 0.f;
    for (int i = 0; i < rows; ++i) a += red[i * C + ch];
    part[(int64_t)blockIdx.x * C + ch] = a;
  }
}

// ------------------------------------------------------------------ up-sum ----
// y[n,oy,x,c] = sum_k x0[n,oy,x,k] W0[c][k] + sum_s up(z_s)[n,oy,x,c] + bias[c]
// (the wide head conv split by branch; z_s = W_s y_s at the branch resolution).
// Workgroup = (band of kUsRows image rows, 64-pixel chunk, 64-channel block); wave w
// owns pixels 16w..16w+15 of each row.  The W0 fragments and the horizontal
// interpolation tables are set up once per workgroup; per row the full-resolution block
// W0 x0 (K = Cin0 <= 32) is a 16x64 MFMA tile per wave (v_mfma_f32_16x16x4f32), each
// source's two contributing rows are blended vertically into LDS (one batch of
// unconditional buffer loads, source columns clamped into the chunk's window), and the
// epilogue adds the two horizontal taps per source and the bias, stores y and
// accumulates the BN partial sums (written once per workgroup).
constexpr int kUsCB = 64, kUsMaxCin = 32;  // (kUsXB, the 64-pixel chunk: heads.h)
// LDS column stride of source s's blended row: the epilogue's 4 lane groups read columns
// 2 (s = 0), 1 (s = 1) or 0-1 (s = 2) apart, so stride * step = 16 (mod 32) puts each
// 32-lane half of a ds_read_b32 on distinct banks.
__host__ __device__ constexpr int us_vs(int s) { return s == 0 ? 72 : 80; }
constexpr int kUsRows = 8;                                          // image rows per workgroup

struct UpSum {
  const float* x;
  int x_ps, cin, cin4, H, W;
  uint32_t x_bytes;
  const float* wp;  // packed [round_up(C,64)][cin4]
  uint32_t wp_bytes;
  const float* bias;
  const float* z[3];
  uint32_t z_bytes[3];
  int zh[3], zw[3], zps[3];
  float sh[3], sw[3];
  int vcols[3];  // staged source columns per 64-pixel chunk
  float* y;
  uint32_t y_bytes;
  int C;
  float* stats;  // [2][rows][C], row = (n*nrb + band)*nxb + xb
  int rows, nxb, nrb;
};

// TIGHT: source s stages at most 4 * (12 >> s) columns per chunk (true for the HRNet
// heads, whose sources halve in resolution): 42 instead of 72 load / blend registers,
// so 3 instead of 2 waves per SIMD, and no clamped duplicate loads.
__host__ __device__ constexpr int us_vu(int s, bool tight) { return tight ? (12 >> s) : 12; }

// KQ: K quads of the W0 block held in registers (5 for Cin0 <= 20, the W18 heads'
// 18-channel branch; 8 up to kUsMaxCin): fewer fragment registers, 4 waves per SIMD.
template <int NUP, bool TIGHT, int KQ>
__global__ __launch_bounds__(256) void upsum_kernel(UpSum p) {
  extern __shared__ __attribute__((aligned(16))) float usm[];
  __shared__ double red[2][4][kUsCB];
  f4* tab = reinterpret_cast<f4*>(usm);                  // [NUP][kUsXB] {i0, i1, l0, l1}
  float* vs = usm + 4 * (NUP > 0 ? NUP : 1) * kUsXB;     // per source [vcols_s][us_vs(s)]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  // block order: chunk fastest, then channel block, then row band
  const int ncb = (p.C + kUsCB - 1) / kUsCB;
  const int xb = blockIdx.x % p.nxb, x0 = xb * kUsXB;
  const int cbi = (blockIdx.x / p.nxb) % ncb;
  const int band = blockIdx.x / (p.nxb * ncb);
  const int n = band / p.nrb, oy0 = (band - n * p.nrb) * kUsRows;
  const int ny = p.H - oy0 < kUsRows ? p.H - oy0 : kUsRows;
  const int c0 = cbi * kUsCB;
  const int xn = p.W - x0 < kUsXB ? p.W - x0 : kUsXB;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(p.wp, p.wp_bytes);
  const __amdgpu_buffer_rsrc_t yr = make_rsrc(p.y, p.y_bytes);
  // ---- W0 fragments (once) ----
  const int kq = p.cin4 >> 2;
  float fb[KQ][4];
#pragma unroll
  for (int kb = 0; kb < KQ; ++kb)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      fb[kb][j] = load1(wr, kb < kq ? (uint32_t)((c0 + 16 * j + r) * p.cin4 + 4 * kb + g) * 4u
                                    : kOOB);
  // ---- horizontal tables and source windows (once) ----
  const int c = c0 + lane;
  const bool cok = c < p.C;
  int vlo[3] = {0, 0, 0}, vhi[3] = {0, 0, 0}, voff[3] = {0, 0, 0};
#pragma unroll
  for (int s = 0; s < NUP; ++s) {
    vlo[s] = lerp_index(x0, p.zw[s], p.sw[s]).i0;
    vhi[s] = lerp_index(x0 + xn - 1, p.zw[s], p.sw[s]).i1;
    voff[s] = s == 0 ? 0 : voff[s - 1] + p.vcols[s - 1] * us_vs(s - 1);  // floats
    if (threadIdx.x < xn) {
      const Lerp lx = lerp_index(x0 + threadIdx.x, p.zw[s], p.sw[s]);
      tab[s * kUsXB + threadIdx.x] =
          f4{__int_as_float(voff[s] + (lx.i0 - vlo[s]) * us_vs(s)),
             __int_as_float(voff[s] + (lx.i1 - vlo[s]) * us_vs(s)), lx.l0, lx.l1};
    }
  }
  float bj[4];
  double s1[4], s2[4];  // BN partial sums over the band (per-row float sums added in double)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int cj = c0 + 16 * j + r;
    bj[j] = (p.bias && cj < p.C) ? p.bias[cj] : 0.f;
    s1[j] = 0.0;
    s2[j] = 0.0;
  }
  const int64_t P = (int64_t)(p.rows / p.nxb / p.nrb) * p.H * p.W;  // n * H * W
  constexpr int VU = 12;  // source columns per wave (host: vcols_s <= 4 * us_vu(s, TIGHT))
  const int pxa = 16 * wave + r;
  for (int ry = 0; ry < ny; ++ry) {
    const int oy = oy0 + ry, row = n * p.H + oy;
    // ---- loads: x0 fragments and the two source rows of every source ----
    float fa[KQ];
#pragma unroll
    for (int kb = 0; kb < KQ; ++kb) {
      const int k = 4 * kb + g;
      fa[kb] = load1(xr, (kb < kq && pxa < xn && k < p.cin)
                             ? (uint32_t)(((row * p.W + x0 + pxa) * p.x_ps + k) * 4u) : kOOB);
    }
    float a0[NUP > 0 ? NUP : 1][VU], a1[NUP > 0 ? NUP : 1][VU];  // only [s][< us_vu] live
    Lerp ly[3];
#pragma unroll
    for (int s = 0; s < NUP; ++s) {
      ly[s] = lerp_index(oy, p.zh[s], p.sh[s]);
      const __amdgpu_buffer_rsrc_t zr = make_rsrc(p.z[s], p.z_bytes[s]);
      const int rb0 = ((n * p.zh[s] + ly[s].i0) * p.zw[s]) * p.zps[s] + c;
      const int rb1 = ((n * p.zh[s] + ly[s].i1) * p.zw[s]) * p.zps[s] + c;
#pragma unroll
      for (int u = 0; u < us_vu(s, TIGHT); ++u) {
        int ix = vlo[s] + wave + 4 * u;
        ix = ix < vhi[s] ? ix : vhi[s];
        a0[s][u] = load1(zr, cok ? (uint32_t)(rb0 + ix * p.zps[s]) * 4u : kOOB);
        a1[s][u] = load1(zr, cok ? (uint32_t)(rb1 + ix * p.zps[s]) * 4u : kOOB);
      }
    }
    __syncthreads();  // the previous row's epilogue reads of vs are done (and tab is written)
#pragma unroll
    for (int s = 0; s < NUP; ++s) {
#pragma unroll
      for (int u = 0; u < us_vu(s, TIGHT); ++u) {
        const int j = wave + 4 * u;  // uniform per wave
        if (vlo[s] + j <= vhi[s])
          vs[voff[s] + j * us_vs(s) + lane] = ly[s].l0 * a0[s][u] + ly[s].l1 * a1[s][u];
      }
    }
    // ---- W0 x0: acc[j][e] = pixel 16*wave + 4g + e, channel c0 + 16j + r ----
    f4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KQ; ++kb) {
      if (kb < kq) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[kb], fb[kb][j], acc[j], 0, 0, 0);
      }
    }
    __syncthreads();
    // ---- epilogue ----
    const uint32_t ybase = (uint32_t)(cbi * P * 64 + ((int64_t)row * p.W + x0) * 64 + r);
    float r1[4] = {0.f, 0.f, 0.f, 0.f}, r2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int px = 16 * wave + 4 * g + e;
      f4 t[3];
#pragma unroll
      for (int s = 0; s < NUP; ++s) t[s] = tab[s * kUsXB + (px < xn ? px : xn - 1)];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = acc[j][e];
#pragma unroll
        for (int s = 0; s < NUP; ++s) {
          const float* vj = vs + 16 * j + r;
          v += t[s][2] * vj[__float_as_int(t[s][0])] + t[s][3] * vj[__float_as_int(t[s][1])];
        }
        const bool ok = px < xn && c0 + 16 * j + r < p.C;
        store1(yr, ok ? (ybase + px * 64 + 16 * j) * 4u : kOOB, v + bj[j]);
        r1[j] += ok ? v : 0.f;  // statistics of y - bias (shifted)
        r2[j] += ok ? v * v : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s1[j] += (double)r1[j];
      s2[j] += (double)r2[j];
    }
  }
  if (p.stats) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s1[j] += __shfl_xor(s1[j], 16, 64);
      s1[j] += __shfl_xor(s1[j], 32, 64);
      s2[j] += __shfl_xor(s2[j], 16, 64);
      s2[j] += __shfl_xor(s2[j], 32, 64);
    }
    if (g == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        red[0][wave][16 * j + r] = s1[j];
        red[1][wave][16 * j + r] = s2[j];
      }
    }
    __syncthreads();
    if (wave == 0 && cok) {
      const int rr = (n * p.nrb + oy0 / kUsRows) * p.nxb + xb;
      p.stats[(int64_t)rr * p.C + c] =
          (float)(red[0][0][lane] + red[0][1][lane] + red[0][2][lane] + red[0][3][lane]);
      p.stats[((int64_t)p.rows + rr) * p.C + c] =
          (float)(red[1][0][lane] + red[1][1][lane] + red[1][2][lane] + red[1][3][lane]);
    }
  }
}

// One-pass up-sum for exact 2^(s+1) sources (the HRNet heads' branches halve in size):
// lane = channel, wave w owns pixels [x0 + 16w, x0 + 16w + 16) of the workgroup's kUsRows
// rows, so nothing is staged in LDS and no barrier runs before the statistics.  W0 x0 is
// computed on the VALU (K = Cin0 <= 4*KQ, 2.6 GF per head: ~10 us of VALU chip-wide) with the
// x0 pixel -- uniform over the lanes -- in scalar registers (constant-address-space loads);
// each source keeps its two rows of the wave's 16/F + 2 source columns in registers,
// re-loaded only when the row pair moves (a row is loaded once per workgroup); the bilinear
// weights are exact (integer arithmetic on pow2 ratios, compile-time horizontally).  Same
// output layout (B64) and statistics rows (y - bias) as upsum_kernel.
__host__ __device__ constexpr int us2_off(int pp, int F) {  // floor((pp + 0.5) / F - 0.5)
  return 2 * pp + 1 - F >= 0 ? (2 * pp + 1 - F) / (2 * F) : -1;
}
__host__ __device__ constexpr float us2_frac(int pp, int F) {
  return (float)(2 * pp + 1 - F - 2 * F * us2_off(pp, F)) / (float)(2 * F);
}

template <int S>
struct Us2Src {
  static constexpr int F = 2 << S, NC = 16 / F + 2;  // source columns px0/F - 1 ... px0/F + 16/F
  float r0[NC], r1[NC];
  int h0, h1;      // rows held in r0 / r1
  float l0, l1;    // vertical weights of the row they serve
};

template <int S>
__device__ __forceinline__ void us2_rows(Us2Src<S>& a, const UpSum& p, int n, int oy, int px0,
                                         int c, bool cok) {
  constexpr int F = Us2Src<S>::F, NC = Us2Src<S>::NC;
  const int num = 2 * oy + 1 - F;
  const int i0 = num >= 0 ? num / (2 * F) : -1;
  a.l1 = (float)(num - 2 * F * i0) / (float)(2 * F);
  a.l0 = 1.f - a.l1;
  const int zh = p.zh[S], zw = p.zw[S];
  const int ra = i0 < 0 ? 0 : (i0 > zh - 1 ? zh - 1 : i0);
  const int rb = i0 + 1 > zh - 1 ? zh - 1 : i0 + 1;
  if (ra == a.h0 && rb == a.h1) return;
  const __amdgpu_buffer_rsrc_t zr = make_rsrc(p.z[S], p.z_bytes[S]);
  const int cb = px0 / F - 1;
  auto load = [&](int row, float* dst) {
    const int rbase = (n * zh + row) * zw;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      int col = cb + q;
      col = col < 0 ? 0 : (col > zw - 1 ? zw - 1 : col);
      dst[q] = load1(zr, cok ? (uint32_t)((rbase + col) * p.zps[S] + c) * 4u : kOOB);
    }
  };
  if (ra == a.h1) {
#pragma unroll
    for (int q = 0; q < NC; ++q) a.r0[q] = a.r1[q];
  } else {
    load(ra, a.r0);
  }
  if (rb != a.h1) load(rb, a.r1);
  a.h0 = ra;
  a.h1 = rb;
}

template <int S>
__device__ __forceinline__ void us2_add(const Us2Src<S>& a, float* v) {
  constexpr int F = Us2Src<S>::F, NC = Us2Src<S>::NC;
  float vb[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) vb[q] = a.l0 * a.r0[q] + a.l1 * a.r1[q];
#pragma unroll
  for (int pp = 0; pp < 16; ++pp) {
    const int o = us2_off(pp, F) + 1;
    const float h1 = us2_frac(pp, F), h0 = 1.f - us2_frac(pp, F);
    v[pp] += h0 * vb[o] + h1 * vb[o + 1];
  }
}

template <int NUP, int KQ>
__global__ __launch_bounds__(256) void upsum2_kernel(UpSum p) {
  __shared__ double red[2][4][kUsCB];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ncb = (p.C + kUsCB - 1) / kUsCB;
  const int xb = blockIdx.x % p.nxb, x0 = xb * kUsXB;
  const int cbi = (blockIdx.x / p.nxb) % ncb;
  const int band = blockIdx.x / (p.nxb * ncb);
  const int n = band / p.nrb, oy0 = (band - n * p.nrb) * kUsRows;
  const int ny = p.H - oy0 < kUsRows ? p.H - oy0 : kUsRows;
  const int c = cbi * kUsCB + lane;
  const bool cok = c < p.C;
  const int px0 = x0 + 16 * wave;
  const int g = lane >> 4, r = lane & 15;
  // W0 fragments: B[k = 4kq + g][n = 16j + r] of the channel block (packed, zero padded)
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(p.wp, p.wp_bytes);
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  float fb[KQ][4];
#pragma unroll
  for (int kq = 0; kq < KQ; ++kq)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      fb[kq][j] = load1(wr, (uint32_t)((cbi * kUsCB + 16 * j + r) * p.cin4 + 4 * kq + g) * 4u);
  __shared__ float xts[4][16 * 64];
  float* xt = xts[wave];
  const float bias = (p.bias && cok) ? p.bias[c] : 0.f;
  Us2Src<0> s0;
  Us2Src<1> s1;
  Us2Src<2> s2;
  s0.h0 = s0.h1 = s1.h0 = s1.h1 = s2.h0 = s2.h1 = -1;
  const __amdgpu_buffer_rsrc_t yr = make_rsrc(p.y, p.y_bytes);
  const int64_t P = (int64_t)(p.rows / p.nxb / p.nrb) * p.H * p.W;  // n * H * W
  double d1 = 0.0, d2 = 0.0;
  // Row ry + 1's loads (x0 fragments, source rows that move) are issued before row ry's
  // stores: vmcnt counts stores too, so a load issued after them would wait for them.
  float xa[KQ];
  auto prep = [&](int oy) {
    const int row = n * p.H + oy;
    const uint32_t xo = (uint32_t)(((row * p.W + px0 + r) * p.x_ps + g) * 4);
#pragma unroll
    for (int kq = 0; kq < KQ; ++kq) xa[kq] = load1(xr, 4 * kq + g < p.cin ? xo + 16u * kq : kOOB);
    if constexpr (NUP > 0) us2_rows<0>(s0, p, n, oy, px0, c, cok);
    if constexpr (NUP > 1) us2_rows<1>(s1, p, n, oy, px0, c, cok);
    if constexpr (NUP > 2) us2_rows<2>(s2, p, n, oy, px0, c, cok);
  };
  prep(oy0);
  for (int ry = 0; ry < ny; ++ry) {
    const int oy = oy0 + ry, row = n * p.H + oy;
    float v[16];
    {  // W0 x0 on MFMA (A = x0[px][k], B = W0 fragments), through this wave's LDS tile
       // to lane = channel: lane (g, r) holds channels 16j + r of pixels 4g + e
      f4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kq = 0; kq < KQ; ++kq)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[kq], fb[kq][j], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) xt[(4 * g + e) * 64 + 16 * j + r] = acc[j][e];
#pragma unroll
      for (int pp = 0; pp < 16; ++pp) v[pp] = xt[pp * 64 + lane];
    }
    if constexpr (NUP > 0) us2_add<0>(s0, v);
    if constexpr (NUP > 1) us2_add<1>(s1, v);
    if constexpr (NUP > 2) us2_add<2>(s2, v);
    if (ry + 1 < ny) prep(oy + 1);
    const uint32_t ybase = (uint32_t)(cbi * P * 64 + ((int64_t)row * p.W + px0) * 64 + lane);
    float q1 = 0.f, q2 = 0.f;
#pragma unroll
    for (int pp = 0; pp < 16; ++pp) {
      store1(yr, cok ? (ybase + pp * 64) * 4u : kOOB, v[pp] + bias);
      q1 += v[pp];
      q2 += v[pp] * v[pp];
    }
    d1 += (double)q1;
    d2 += (double)q2;
  }
  if (p.stats) {
    red[0][wave][lane] = d1;
    red[1][wave][lane] = d2;
    __syncthreads();
    if (wave == 0 && cok) {
      const int rr = (n * p.nrb + oy0 / kUsRows) * p.nxb + xb;
      p.stats[(int64_t)rr * p.C + c] =
          (float)(red[0][0][lane] + red[0][1][lane] + red[0][2][lane] + red[0][3][lane]);
      p.stats[((int64_t)p.rows + rr) * p.C + c] =
          (float)(red[1][0][lane] + red[1][1][lane] + red[1][2][lane] + red[1][3][lane]);
    }
  }
}

// Pixels per block of the backward passes (>= 64 each): the reduce pass with <= 2048
// blocks (a block holds only 3 pixel rows of 68 channel quads, so 1024 blocks left one
// wave per SIMD: 134 -> 122 us per head), the apply pass with <= 1024 (measured better).
static int64_t head_ppb(int64_t P, int64_t blocks = 2048) {
  int64_t ppb = ceil_div(P, blocks);
  ppb = ppb < 64 ? 64 : ppb;
  return ppb > kHeadMaxPpb ? kHeadMaxPpb : ppb;  // the block's dout rows are staged in LDS
}

static bool head_args_ok(const float* y, const vae2_act* yd, int cout2) {
  return y && act_ok(yd) && ((uintptr_t)y % 16 == 0) && (yd->c + 3) / 4 <= 256 &&
         cout2 >= 1 && cout2 <= kHeadMaxOut;
}

// Kernel tables: [cout2 - 1] (1..4) [U == 4 pixels in flight]; [nup] (0..3) and the one-pass
// up-sum's [cin4 / 4 - 1] K quads or the staged one's {tight KQ 5, tight KQ 8, wide KQ 8}.
constexpr decltype(&head_out_fwd_kernel<1>) kHeadFwd[4] = {
    head_out_fwd_kernel<1>, head_out_fwd_kernel<2>, head_out_fwd_kernel<3>,
    head_out_fwd_kernel<4>};
constexpr decltype(&head_out_bwd_reduce_kernel<1, 2>) kHeadReduce[4][2] = {
    {head_out_bwd_reduce_kernel<1, 2>, head_out_bwd_reduce_kernel<1, 4>},
    {head_out_bwd_reduce_kernel<2, 2>, head_out_bwd_reduce_kernel<2, 4>},
    {head_out_bwd_reduce_kernel<3, 2>, head_out_bwd_reduce_kernel<3, 4>},
    {head_out_bwd_reduce_kernel<4, 2>, head_out_bwd_reduce_kernel<4, 4>}};
constexpr decltype(&head_out_bwd_apply_kernel<1, 2>) kHeadApply[4][2] = {
    {head_out_bwd_apply_kernel<1, 2>, head_out_bwd_apply_kernel<1, 4>},
    {head_out_bwd_apply_kernel<2, 2>, head_out_bwd_apply_kernel<2, 4>},
    {head_out_bwd_apply_kernel<3, 2>, head_out_bwd_apply_kernel<3, 4>},
    {head_out_bwd_apply_kernel<4, 2>, head_out_bwd_apply_kernel<4, 4>}};
using UpSumKernel = void (*)(UpSum);
template <int N>
constexpr UpSumKernel kUpSum2Kq[5] = {upsum2_kernel<N, 1>, upsum2_kernel<N, 2>, upsum2_kernel<N, 3>,
                                      upsum2_kernel<N, 4>, upsum2_kernel<N, 5>};
constexpr const UpSumKernel* kUpSum2[4] = {kUpSum2Kq<0>, kUpSum2Kq<1>, kUpSum2Kq<2>, kUpSum2Kq<3>};
template <int N>
constexpr UpSumKernel kUpSumForm[3] = {upsum_kernel<N, true, 5>, upsum_kernel<N, true, 8>,
                                       upsum_kernel<N, false, 8>};
constexpr const UpSumKernel* kUpSum[4] = {kUpSumForm<0>, kUpSumForm<1>, kUpSumForm<2>,
                                          kUpSumForm<3>};

// vae2_heads_set_algo: a set bit stores `set`, a clear one `clear` (the default).
struct Switch { int* var; int bit, clear, set; };
static int g_upsum_tight = 1, g_upsum_one = 1, g_head_red_u = 2, g_head_app_u = 2;
static const Switch kSwitches[] = {
    // two-pass pow2 adjoint: vertical pass per channel lane (up_adj2_v), not streamed (_vs)
    {&g_adj_stream, 1, 1, 0},
    // the LDS-staged up-sum stages 12 columns per wave for every source, not 12 >> s
    // (us_vu: 42 instead of 72 load / blend registers, 3 instead of 2 waves per SIMD)
    {&g_upsum_tight, 2, 1, 0},
    {&g_adj_fused, 4, 1, 0},  // no one-pass band adjoint (up_adj3_kernel): two passes instead
    {&g_upsum_one, 8, 1, 0},  // no one-pass up-sum (upsum2_kernel): upsum_kernel everywhere
    // 4 instead of 2 pixels in flight per thread in the backward reduce (2: 4 waves per
    // SIMD, 120 -> 95 us per head in round 2) and in the backward apply
    {&g_head_red_u, 16, 2, 4},
    {&g_head_app_u, 32, 2, 4},
    // the fuse adjoints (vae2_upsample_bilinear_bwd_pow2) through the one-pass band kernel.
    // Off: with 18-72 channels a 64-lane channel block is mostly idle, and the step measured
    // 851-853 vs 861-866 frames/s through the two-pass quad kernels (A/B, same box)
    {&g_fuse_adj3, 64, 0, 1},
    {&g_relu_dual_q, 128, 1, 0},  // relu_bwd_dual a channel per thread, not a channel quad
};
// Bits 8-15 (g_adj_band): dy rows per workgroup of the one-pass adjoint, a multiple of 8
// from 8 up; any other value, 0 included, is the default, which reads back as 0.

}  // namespace vae2

using namespace vae2;

extern "C" {

int vae2_head_out_fwd(const float* y, const vae2_act* yd, const float* save, const float* w2,
                      const float* b2, int cout2, float* out, const vae2_act* outd,
                      void* stream) {
  const char* fn = "vae2_head_out_fwd";
  VAE2_REQUIRE(head_args_ok(y, yd, cout2) && save && w2 && out && act_ok(outd), fn,
               "bad arguments (y must be 16-byte aligned NHWC with ps % 4 == 0, cout2 <= 4)");
  VAE2_REQUIRE(outd->n == yd->n && outd->h == yd->h && outd->w == yd->w && outd->c >= cout2,
               fn, "output shape mismatch");
  const int c4 = (int)((yd->c + 3) / 4);
  const size_t shm = (size_t)(2 + cout2) * c4 * 16;
  const int64_t P = act_pixels(yd);
  const unsigned grid = (unsigned)(ceil_div(P, 16) < 8192 ? ceil_div(P, 16) : 8192);
  VAE2_LAUNCH(kHeadFwd[cout2 - 1], dim3(grid), dim3(256), shm, as_stream(stream), y,
              to_act(yd), save, w2, b2, out, to_act(outd));
  return check_launch(fn);
}

int64_t vae2_head_out_bwd_ws_size(const vae2_act* yd, int cout2) {
  if (!act_ok(yd)) return 0;
  const int64_t P = act_pixels(yd);
  const int64_t blocks = ceil_div(P, head_ppb(P));
  const int64_t NC = 2 * yd->c + cout2 * yd->c + cout2;
  return blocks * NC;
}

int vae2_head_out_bwd_reduce(const float* y, const vae2_act* yd, const float* save,
                             const float* w2, int cout2, const float* dout,
                             const vae2_act* doutd, double* sums, float* dgamma, float* dbeta,
                             float* dw2, float* db2, float* ws, int64_t ws_size, void* stream) {
  const char* fn = "vae2_head_out_bwd_reduce";
  VAE2_REQUIRE(head_args_ok(y, yd, cout2) && save && w2 && dout && sums && ws &&
                   act_ok(doutd), fn, "bad arguments");
  VAE2_REQUIRE(doutd->n == yd->n && doutd->h == yd->h && doutd->w == yd->w &&
                   doutd->c >= cout2, fn, "dout shape mismatch");
  VAE2_REQUIRE(ws_size >= vae2_head_out_bwd_ws_size(yd, cout2), fn, "workspace too small");
  const int C = (int)yd->c, c4 = (C + 3) / 4, rows = 256 / c4;
  const int NC = 2 * C + cout2 * C + cout2;
  const int64_t P = act_pixels(yd), ppb = head_ppb(P);
  const unsigned blocks = (unsigned)ceil_div(P, ppb);
  const size_t shm = ((size_t)rows * NC + (size_t)ppb * cout2) * sizeof(float);
  VAE2_REQUIRE(shm <= 64 * 1024, fn, "too many channels for the LDS reduction");
  VAE2_LAUNCH(kHeadReduce[cout2 - 1][g_head_red_u == 4], dim3(blocks), dim3(256), shm,
              as_stream(stream), y, to_act(yd), save, w2, dout, to_act(doutd), ppb, rows, ws);
  int rc = check_launch(fn);
  if (rc) return rc;
  VAE2_LAUNCH(head_bwd_colsum_kernel, dim3((unsigned)ceil_div(NC, 64)), dim3(1024), 0,
                     as_stream(stream), (const float*)ws, (int)blocks, C, cout2, sums, dgamma,
                     dbeta, dw2, db2);
  return check_launch(fn);
}

int vae2_head_out_bwd_apply(const float* y, const vae2_act* yd, const float* save,
                            const float* gamma, const float* w2, int cout2, const float* dout,
                            const vae2_act* doutd, const double* sums, double count, float* dy,
                            const vae2_act* dyd, float* dbias, float* ws, int64_t ws_size,
                            void* stream) {
  const char* fn = "vae2_head_out_bwd_apply";
  VAE2_REQUIRE(head_args_ok(y, yd, cout2) && save && w2 && dout && sums && dy && ws &&
                   act_ok(doutd) && act_ok(dyd) && count > 0, fn, "bad arguments");
  VAE2_REQUIRE(doutd->n == yd->n && doutd->h == yd->h && doutd->w == yd->w &&
                   doutd->c >= cout2, fn, "dout shape mismatch");
  VAE2_REQUIRE(dyd->n == yd->n && dyd->h == yd->h && dyd->w == yd->w && dyd->c == yd->c &&
                   ((uintptr_t)dy % 16 == 0) && dyd->ps % 4 == 0, fn, "dy shape mismatch");
  VAE2_REQUIRE(ws_size >= vae2_head_out_bwd_ws_size(yd, cout2), fn, "workspace too small");
  const int C = (int)yd->c, c4 = (C + 3) / 4, rows = 256 / c4;
  const int64_t P = act_pixels(yd), ppb = head_ppb(P, 1024);
  const unsigned blocks = (unsigned)ceil_div(P, ppb);
  const size_t shm = ((size_t)rows * C + (size_t)ppb * cout2) * sizeof(float);
  VAE2_LAUNCH(kHeadApply[cout2 - 1][g_head_app_u == 4], dim3(blocks), dim3(256), shm,
              as_stream(stream), y, to_act(yd), save, gamma, w2, dout, to_act(doutd), sums,
              count, ppb, rows, dy, to_act(dyd), ws);
  int rc = check_launch(fn);
  if (rc) return rc;
  if (dbias) return bias_grad_from_partials(ws, blocks, C, dbias, 1, stream);
  return 0;
}

int64_t vae2_conv1x1_upsum_stats_rows(const vae2_act* yd) {
  if (!act_ok(yd)) return 0;
  return yd->n * ceil_div(yd->h, kUsRows) * ceil_div(yd->w, kUsXB);
}

int vae2_conv1x1_upsum_fwd(const float* x, const vae2_act* xd, const float* wp,
                           const float* bias, int nup, const float* const* ups,
                           const vae2_act* upds, float* y, const vae2_act* yd, float* stats,
                           void* stream) {
  const char* fn = "vae2_conv1x1_upsum_fwd";
  VAE2_REQUIRE(x && wp && y && act_ok(xd) && act_ok(yd), fn, "bad arguments");
  VAE2_REQUIRE(xd->n == yd->n && xd->h == yd->h && xd->w == yd->w, fn, "x / y shape mismatch");
  VAE2_REQUIRE(xd->c <= kUsMaxCin, fn, "Cin0 > 32");
  VAE2_REQUIRE(nup >= 0 && nup <= 3 && (nup == 0 || (ups && upds)), fn, "bad up-sum terms");
  UpSum p{};
  p.x = x; p.x_ps = (int)xd->ps; p.cin = (int)xd->c; p.cin4 = ((int)xd->c + 3) / 4 * 4;
  p.H = (int)yd->h; p.W = (int)yd->w;
  p.wp = wp; p.bias = bias;
  const int64_t P = act_pixels(yd);
  const int64_t ncb = ceil_div(yd->c, kUsCB);
  const int64_t x_bytes = act_pixels(xd) * xd->ps * 4;
  const int64_t y_bytes = ncb * P * 64 * 4;
  VAE2_REQUIRE(x_bytes < (1ll << 31) && y_bytes < (1ll << 31), fn,
               "tensor too large for 32-bit offsets");
  p.x_bytes = (uint32_t)x_bytes;
  p.wp_bytes = (uint32_t)(ncb * kUsCB * p.cin4 * 4);
  int vtot = 0;
  for (int s = 0; s < nup; ++s) {
    const vae2_act* u = &upds[s];
    VAE2_REQUIRE(ups[s] && act_ok(u) && u->n == yd->n && u->c >= yd->c && u->h <= yd->h &&
                     u->w <= yd->w, fn, "up-sum term shape mismatch");
    const int64_t zb = act_pixels(u) * u->ps * 4;
    VAE2_REQUIRE(zb < (1ll << 31), fn, "up-sum term too large for 32-bit offsets");
    p.z[s] = ups[s]; p.zh[s] = (int)u->h; p.zw[s] = (int)u->w; p.zps[s] = (int)u->ps;
    p.z_bytes[s] = (uint32_t)zb;
    p.sh[s] = (float)u->h / (float)yd->h;
    p.sw[s] = (float)u->w / (float)yd->w;
    p.vcols[s] = (int)ceilf(p.sw[s] * kUsXB) + 3;
    VAE2_REQUIRE(p.vcols[s] <= 48, fn, "source wider than half the output (upsampling only)");
    vtot += p.vcols[s] * us_vs(s);
  }
  p.y = y; p.y_bytes = (uint32_t)y_bytes; p.C = (int)yd->c;
  p.stats = stats;
  p.nxb = (int)ceil_div(yd->w, kUsXB);
  p.nrb = (int)ceil_div(yd->h, kUsRows);
  p.rows = (int)vae2_conv1x1_upsum_stats_rows(yd);
  const int nu = nup > 0 ? nup : 1;
  const size_t shm = ((size_t)4 * nu * kUsXB + (size_t)(vtot > 0 ? vtot : 1)) * sizeof(float);
  dim3 grid((unsigned)(yd->n * p.nrb * p.nxb * ncb));
  hipStream_t st = as_stream(stream);
  bool one = g_upsum_one && yd->w % kUsXB == 0 && p.cin4 <= 20;
  for (int s = 0; s < nup; ++s)
    one = one && yd->h == (int64_t)p.zh[s] << (s + 1) && yd->w == (int64_t)p.zw[s] << (s + 1);
  if (one) {
    VAE2_LAUNCH(kUpSum2[nup][p.cin4 / 4 - 1], grid, dim3(256), 0, st, p);
    return check_launch(fn);
  }
  bool tight = g_upsum_tight != 0;
  for (int s = 0; s < nup; ++s) tight = tight && p.vcols[s] <= 4 * us_vu(s, true);
  const int form = !tight ? 2 : p.cin4 <= 20 ? 0 : 1;
  VAE2_LAUNCH(kUpSum[nup][form], grid, dim3(256), shm, st, p);
  return check_launch(fn);
}

int vae2_heads_set_algo(int algo) {
  int prev = g_adj_band == kAdjBandDefault ? 0 : g_adj_band << 8;
  for (const Switch& sw : kSwitches) {
    if (*sw.var == sw.set) prev |= sw.bit;
    *sw.var = (algo & sw.bit) ? sw.set : sw.clear;
  }
  const int band = (algo >> 8) & 0xff;
  g_adj_band = band >= 8 && band % 8 == 0 ? band : kAdjBandDefault;
  return prev;
}

}  // extern "C"

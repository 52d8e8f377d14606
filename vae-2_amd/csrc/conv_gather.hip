// The gather kernels of the convolutions: igemm_kernel (implicit GEMM, every geometry:
// forward and, per stride-parity class, the data gradient) and gemm1x1_kernel (persistent
// 1x1 GEMM for the full-resolution 1x1 convs), their tile rules and launchers.  The
// fragment layout is described at the top of conv.hip.
#include "conv.h"

namespace vae2 {

// KS = 4: in-workgroup K split for layers with too few row tiles to fill the chip: the 4
// waves share one (16*TM)-row tile, wave w takes K chunks w, w+4, ..., and the partial
// tiles are summed in LDS in a fixed order (deterministic) before wave 0's epilogue.
// NR > 0 (fp32, KS = 1, one N block): N = 16*TN + NR (18 = 16 + 2, 36 = 32 + 4) -- the
// last NR output channels on the VALU beside the MFMAs instead of a mostly-padding MFMA
// column tile: every lane already holds its A fragment (pixel r, 4 channels of the chunk),
// multiplies it with the remainder rows' weights for those channels, and the 4 lane
// groups' K shares are summed at the end (dconv3_kernel's remainder, for the gather GEMM).
constexpr int kIgTab = 1024;  // igemm K-step table entries (16 KB of LDS)

template <int TM, int TN, bool VEC, int ROLE, int KS = 1, bool BF = false, int NR = 0>
__global__ __launch_bounds__(256) void igemm_kernel(IGemm pin) {
  IGemm p = pin;
  if (gridDim.z > 1) {
    const IGemm::Cls& c = pin.cls[blockIdx.z];
    p.g_h = c.g_h; p.g_w = c.g_w; p.nth = c.nth; p.ntw = c.ntw;
    p.dh0 = c.dh0; p.dw0 = c.dw0; p.kh0 = c.kh0; p.kw0 = c.kw0;
    p.y_offh = c.y_offh; p.y_offw = c.y_offw; p.hw_div = c.hw_div; p.w_div = c.w_div;
  }
  constexpr int BN = 16 * TN;
  static_assert(NR == 0 || (KS == 1 && !BF && NR <= 4), "remainder form");
  __shared__ float red[4][2][BN + NR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, r = lane & 15;
  const int M = p.g_n * p.g_h * p.g_w;
  const int bm = xcd_remap(blockIdx.x, gridDim.x);
  const int mw = (KS == 1 ? bm * 4 + wave : bm) * (16 * TM);
  const int n0 = blockIdx.y * BN;
  const int kk4 = p.ksz * p.ksz * p.a_c4;

  // this lane's A rows: m = mw + i*16 + r
  int rpix[TM], ri[TM], rj[TM];
  bool rok[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    int m = mw + i * 16 + r;
    rok[i] = m < M;
    int mm = rok[i] ? m : 0;
    int gn = (int)p.hw_div.div((uint32_t)mm);
    int rem = mm - gn * p.g_h * p.g_w;
    int gi = (int)p.w_div.div((uint32_t)rem);
    int gj = rem - gi * p.g_w;
    ri[i] = gi * p.a_step;
    rj[i] = gj * p.a_step;
    rpix[i] = (gn * p.a_h + ri[i]) * p.a_w + rj[i];
  }
  // Buffer resources (wave-uniform): out-of-range offsets load 0, so padding taps,
  // rows past M and the K tail need no branches.
  const __amdgpu_buffer_rsrc_t arsrc = make_rsrc(p.a, p.a_bytes);
  const __amdgpu_buffer_rsrc_t wrsrc = make_rsrc(p.w, p.w_bytes);
  uint32_t wrow[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) wrow[j] = (uint32_t)((n0 + j * 16 + r) * kk4) * 4u;
  uint32_t wrowr[NR > 0 ? NR : 1];  // remainder rows BN + q of the packed weights
#pragma unroll
  for (int q = 0; q < NR; ++q) wrowr[q] = (uint32_t)((n0 + BN + q) * kk4) * 4u;
  float racc[TM][NR > 0 ? NR : 1];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int q = 0; q < NR; ++q) racc[i][q] = 0.f;

  const int ntaps = p.nth * p.ntw;
  const int K = ntaps * p.a_c4;
  const int nchunks = KS == 1 ? (K + 15) >> 4 : (((K + 15) >> 4) + KS - 1 - wave) / KS;
  int tt = 0, c0 = 4 * g + (KS == 1 ? 0 : 16 * wave);
  while (c0 >= p.a_c4) { c0 -= p.a_c4; ++tt; }
  const bool cpad = (p.a_c & 3) != 0;
  // K-step table (quad step k = (tap, quad) of the linear K order): the tap decode (a
  // division by ntw), the carry loop and the tap's A / B offsets computed once per
  // workgroup instead of per lane and chunk; entry = (dh, dw | c0 << 16, weight byte
  // offset, A element offset (dh * a_w + dw) * a_ps + c0).  Steps past K (the prefetch of
  // the chunk pairs) get dh far outside the image and kOOB weights: zero operands.
  __shared__ int4 ktab[kIgTab];
  const int nq = K >> 2;                                  // quad steps
  // entries the loop can read: every wave's chunks + the 2 prefetched past its last
  const int nqt = 4 * ((K + 15) >> 4) + 16 * KS + 16;
  const bool use_tab = !BF && p.ktab && nqt <= kIgTab;
  if (use_tab) {
    const int q4 = p.a_c4 >> 2;
    for (int k = threadIdx.x; k < nqt; k += 256) {
      int4 e;
      if (k < nq) {
        const int t = k / q4, q = k - t * q4;
        const int th = t / p.ntw, tw = t - th * p.ntw;
        const int dh = p.dh0 + th * p.dhs, dw = p.dw0 + tw * p.dws;
        const int tlin = (p.kh0 + th * p.khs) * p.ksz + (p.kw0 + tw * p.kws);
        e = make_int4(dh, (dw & 0xffff) | (4 * q) << 16, (int)((uint32_t)(tlin * p.a_c4 + 4 * q) * 4u),
                      (dh * p.a_w + dw) * p.a_ps + 4 * q);
      } else {
        e = make_int4(1 << 20, 0, (int)kOOB, 0);
      }
      ktab[k] = e;
    }
  }
  __syncthreads();
  int kq = g + (KS == 1 ? 0 : 4 * wave);  // this lane's next quad step (as c0 / tt above)
  int rbase[TM];  // rpix * a_ps: the row's pixel in elements
#pragma unroll
  for (int i = 0; i < TM; ++i) rbase[i] = rpix[i] * p.a_ps;

  f4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
  f4 fr0[NR > 0 ? NR : 1], fr1[NR > 0 ? NR : 1];  // remainder weights of the chunk
  f4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  auto load = [&](f4* fa, f4* fb, f4* fr, int& mk) {
    if (use_tab) {
      const int4 e = ktab[kq];
      kq += 4 * KS;
      const int dh = e.x, dw = (int)(short)(e.y & 0xffff), cq = e.y >> 16;
      const uint32_t woff = (uint32_t)e.z;
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = load4(wrsrc, wrow[j] + woff);
#pragma unroll
      for (int q = 0; q < NR; ++q) fr[q] = load4(wrsrc, woff == kOOB ? kOOB : wrowr[q] + woff);
      const bool m1 = cq + 1 < p.a_c, m2 = cq + 2 < p.a_c, m3 = cq + 3 < p.a_c;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int ih = ri[i] + dh, iw = rj[i] + dw;
        const bool ok = rok[i] && (unsigned)ih < (unsigned)p.a_h && (unsigned)iw < (unsigned)p.a_w;
        const uint32_t off = ok ? (uint32_t)(rbase[i] + e.w) * 4u : kOOB;
        f4 v;
        if (VEC) {
          v = load4(arsrc, off);
        } else {
          v[0] = load1(arsrc, off);
          v[1] = load1(arsrc, m1 ? off + 4u : kOOB);
          v[2] = load1(arsrc, m2 ? off + 8u : kOOB);
          v[3] = load1(arsrc, m3 ? off + 12u : kOOB);
        }
        fa[i] = v;
      }
      mk = (m1 ? 2 : 0) | (m2 ? 4 : 0) | (m3 ? 8 : 0);
      return;
    }
    const bool tv = tt < ntaps;
    const int tc = tv ? tt : 0;
    const int th = tc / p.ntw;
    const int tw = tc - th * p.ntw;
    const int dh = p.dh0 + th * p.dhs, dw = p.dw0 + tw * p.dws;
    const int tlin = (p.kh0 + th * p.khs) * p.ksz + (p.kw0 + tw * p.kws);
    const uint32_t woff = tv ? (uint32_t)(tlin * p.a_c4 + c0) * 4u : kOOB;
#pragma unroll
    for (int j = 0; j < TN; ++j) fb[j] = load4(wrsrc, wrow[j] + woff);
#pragma unroll
    for (int q = 0; q < NR; ++q) fr[q] = load4(wrsrc, tv ? wrowr[q] + woff : kOOB);
    const int doff = dh * p.a_w + dw;
    const bool m1 = c0 + 1 < p.a_c, m2 = c0 + 2 < p.a_c, m3 = c0 + 3 < p.a_c;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int ih = ri[i] + dh, iw = rj[i] + dw;
      const bool ok = tv && rok[i] && (unsigned)ih < (unsigned)p.a_h &&
                      (unsigned)iw < (unsigned)p.a_w;
      const uint32_t off = ok ? (uint32_t)((rpix[i] + doff) * p.a_ps + c0) * 4u : kOOB;
      f4 v;
      if (VEC) {
        v = load4(arsrc, off);  // channel-pad lanes are masked where consumed (mma)
      } else {
        v[0] = load1(arsrc, off);
        v[1] = load1(arsrc, m1 ? off + 4u : kOOB);
        v[2] = load1(arsrc, m2 ? off + 8u : kOOB);
        v[3] = load1(arsrc, m3 ? off + 12u : kOOB);
      }
      fa[i] = v;
    }
    mk = (m1 ? 2 : 0) | (m2 ? 4 : 0) | (m3 ? 8 : 0);
    c0 += 16 * KS;
    while (c0 >= p.a_c4) { c0 -= p.a_c4; ++tt; }
  };
  // Masking the pad lanes here (not right after the loads) keeps the next chunk's
  // loads in flight across this chunk's MFMAs.
  auto mma = [&](f4* fa, const f4* fb, const f4* fr, int mk) {
    if (VEC && cpad) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        fa[i][1] = (mk & 2) ? fa[i][1] : 0.f;
        fa[i][2] = (mk & 4) ? fa[i][2] : 0.f;
        fa[i][3] = (mk & 8) ? fa[i][3] : 0.f;
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int q = 0; q < NR; ++q)
#pragma unroll
        for (int s = 0; s < 4; ++s) racc[i][q] = __builtin_fmaf(fa[i][s], fr[q][s], racc[i][q]);
  };

  // Chunk pairs; the (possibly) extra odd chunk loads zeros (tt >= ntaps).
  if (mw < M && !BF) {
    int mk0 = 0, mk1 = 0;
    load(fa0, fb0, fr0, mk0);
    for (int ch = 0; ch < nchunks; ch += 2) {
      load(fa1, fb1, fr1, mk1);
      mma(fa0, fb0, fr0, mk0);
      load(fa0, fb0, fr0, mk0);
      mma(fa1, fb1, fr1, mk1);
    }
  } else if (mw < M) {  // bf16 operands: one 16x16x32 MFMA per chunk pair
    int mk0 = 0, mk1 = 0;
    load(fa0, fb0, fr0, mk0);
    load(fa1, fb1, fr1, mk1);
    for (int ch = 0; ch < nchunks; ch += 2) {
      if (VEC && cpad) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          fa0[i][1] = (mk0 & 2) ? fa0[i][1] : 0.f;
          fa0[i][2] = (mk0 & 4) ? fa0[i][2] : 0.f;
          fa0[i][3] = (mk0 & 8) ? fa0[i][3] : 0.f;
          fa1[i][1] = (mk1 & 2) ? fa1[i][1] : 0.f;
          fa1[i][2] = (mk1 & 4) ? fa1[i][2] : 0.f;
          fa1[i][3] = (mk1 & 8) ? fa1[i][3] : 0.f;
        }
      }
      bf16x8 A[TM], B[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) A[i] = pack_bf16(fa0[i], fa1[i]);
#pragma unroll
      for (int j = 0; j < TN; ++j) B[j] = pack_bf16(fb0[j], fb1[j]);
      load(fa0, fb0, fr0, mk0);
      load(fa1, fb1, fr1, mk1);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[i], B[j], acc[i][j], 0, 0, 0);
    }
  }

  if constexpr (KS > 1) {
    __shared__ float kred[KS - 1][TM * TN * 4][64];
    if (wave > 0) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) kred[wave - 1][(i * TN + j) * 4 + e][lane] = acc[i][j][e];
    }
    __syncthreads();
    if (wave > 0) return;  // no barrier below on this path
#pragma unroll
    for (int w = 0; w < KS - 1; ++w)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][e] += kred[w][(i * TN + j) * 4 + e][lane];
  }

  // ---- epilogue ----
  float csum[TN], csq[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) { csum[j] = 0.f; csq[j] = 0.f; }
  // producer BatchNorm backward partials (data gradient, bx set): per-column mean, invstd,
  // scale, shift of that layer (bn_bwd_reduce_body's arithmetic, element by element)
  constexpr bool BP = ROLE == 1 && !BF;
  const bool bnp = BP && p.bx != nullptr;
  float bmn[BP ? TN : 1], bis[BP ? TN : 1], bsc[BP ? TN : 1], bsh[BP ? TN : 1];
  if constexpr (BP) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + j * 16 + r < p.n ? n0 + j * 16 + r : p.n - 1;
      bmn[j] = bnp ? p.bsave[n] : 0.f;
      bis[j] = bnp ? p.bsave[p.n + n] : 0.f;
      bsc[j] = bnp ? p.bsave[2 * p.n + n] : 0.f;
      bsh[j] = bnp ? p.bsave[3 * p.n + n] : 0.f;
    }
  }
  // output pixel of GEMM row m (m < M)
  auto pix_of = [&](int m) {
    const int gn = (int)p.hw_div.div((uint32_t)m);
    const int rem = m - gn * p.g_h * p.g_w;
    const int gi = (int)p.w_div.div((uint32_t)rem);
    const int gj = rem - gi * p.g_w;
    return (gn * p.y_h + gi * p.y_step + p.y_offh) * p.y_w + gj * p.y_step + p.y_offw;
  };
  if (p.vec_out && (KS == 1 || wave == 0)) {
    // statistics in the MFMA layout (beta = 0 whenever they are requested), then each
    // 16x16 tile transposed inside lane quads: one 16-byte store per lane and tile, and
    // one output-pixel address per lane and row tile instead of four
    const int k = r & 3, qc = 4 * (r >> 2);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      if (BP && bnp && p.stats) {
        // the row tile's 4 x TN pre-BN values, one batch of range-checked loads
        const __amdgpu_buffer_rsrc_t bxr = make_rsrc(p.bx, p.bx_bytes);
        float xv[4][TN];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int me = mw + i * 16 + g * 4 + e;
          const bool mok = me < M;
          const int pix = pix_of(mok ? me : 0);
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int n = n0 + j * 16 + r;
            xv[e][j] = load1(bxr, mok && n < p.n ? (uint32_t)(pix * p.bx_ps + n) * 4u : kOOB);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool mok = mw + i * 16 + g * 4 + e < M;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int n = n0 + j * 16 + r;
            const float v = acc[i][j][e];
            const float x = xv[e][j];
            const float gv = (p.brelu && !(__builtin_fmaf(x, bsc[j], bsh[j]) > 0.f)) ? 0.f : v;
            const bool ok = mok && n < p.n;
            csum[j] += ok ? gv : 0.f;
            csq[j] += ok ? gv * (x - bmn[j]) * bis[j] : 0.f;
          }
        }
      } else if (p.stats) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (mw + i * 16 + g * 4 + e >= M) continue;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int n = n0 + j * 16 + r;
            if (n >= p.n) continue;
            const float v = acc[i][j][e] + (p.bias ? p.bias[n] : 0.f);
            csum[j] += v;
            csq[j] += v * v;
          }
        }
      }
      const int m = mw + i * 16 + g * 4 + k;
      const bool mok = m < M;
      const int mm = mok ? m : 0;
      const int gn = (int)p.hw_div.div((uint32_t)mm);
      const int rem = mm - gn * p.g_h * p.g_w;
      const int gi = (int)p.w_div.div((uint32_t)rem);
      const int gj = rem - gi * p.g_w;
      float* yrow = p.y + ((gn * p.y_h + gi * p.y_step + p.y_offh) * p.y_w +
                           gj * p.y_step + p.y_offw) * p.y_ps;
      // beta: the row tile's old output quads all loaded before any store (one round trip
      // per row tile instead of one per quad: loads cannot pass the stores to y)
      f4 yold[TN];
      if (p.beta != 0.f) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int n = n0 + j * 16 + qc;
          yold[j] = (mok && n + 3 < p.n) ? *reinterpret_cast<const f4*>(yrow + n)
                                         : f4{0.f, 0.f, 0.f, 0.f};
        }
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        f4 v = acc[i][j];
        quad_transpose(v, k);
        const int n = n0 + j * 16 + qc;
        if (!mok || n >= p.n) continue;
        if (p.bias) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] += n + q < p.n ? p.bias[n + q] : 0.f;
        }
        if (n + 3 < p.n) {
          if (p.beta != 0.f) v += p.beta * yold[j];
          *reinterpret_cast<f4*>(yrow + n) = v;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (n + q < p.n) yrow[n + q] = p.beta != 0.f ? v[q] + p.beta * yrow[n + q] : v[q];
        }
      }
    }
  } else
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = mw + i * 16 + g * 4 + e;
      if (m >= M) continue;
      const int gn = (int)p.hw_div.div((uint32_t)m);
      const int rem = m - gn * p.g_h * p.g_w;
      const int gi = (int)p.w_div.div((uint32_t)rem);
      const int gj = rem - gi * p.g_w;
      const int oy = gi * p.y_step + p.y_offh;
      const int ox = gj * p.y_step + p.y_offw;
      float* yrow = p.y + ((gn * p.y_h + oy) * p.y_w + ox) * p.y_ps;
      const float* xrow = BP && bnp ? p.bx + ((gn * p.y_h + oy) * p.y_w + ox) * p.bx_ps : nullptr;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + j * 16 + r;
        if (n >= p.n) continue;
        float v = acc[i][j][e];
        if (p.bias) v += p.bias[n];
        if (p.beta != 0.f) v += p.beta * yrow[n];
        yrow[n] = v;
        if (BP && bnp) {
          const float x = xrow[n];
          const float gv = (p.brelu && !(__builtin_fmaf(x, bsc[j], bsh[j]) > 0.f)) ? 0.f : v;
          csum[j] += gv;
          csq[j] += gv * (x - bmn[j]) * bis[j];
        } else {
          csum[j] += v;
          csq[j] += v * v;
        }
      }
    }
  }
  // the VALU remainder's outputs: the 4 lane groups' K shares summed (every group then holds
  // pixel i*16 + r's sums); lane group g writes the channels q = g (mod 4)
  float rsum[NR > 0 ? NR : 1], rsq[NR > 0 ? NR : 1];
  if constexpr (NR > 0) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        racc[i][q] += __shfl_xor(racc[i][q], 16, 64);
        racc[i][q] += __shfl_xor(racc[i][q], 32, 64);
      }
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      rsum[q] = 0.f;
      rsq[q] = 0.f;
      if ((q & 3) != g) continue;
      const int n = n0 + BN + q;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int m = mw + i * 16 + r;
        const bool mok = m < M && n < p.n;
        const int mm = m < M ? m : 0;
        const int gn = (int)p.hw_div.div((uint32_t)mm);
        const int rem = mm - gn * p.g_h * p.g_w;
        const int gi = (int)p.w_div.div((uint32_t)rem);
        const int gj = rem - gi * p.g_w;
        float* yp = p.y + ((gn * p.y_h + gi * p.y_step + p.y_offh) * p.y_w + gj * p.y_step +
                           p.y_offw) * p.y_ps + n;
        float v = racc[i][q];
        if (p.bias) v += p.bias[n < p.n ? n : 0];
        if (p.beta != 0.f && mok) v += p.beta * *yp;
        if (mok) *yp = v;
        if (BP && bnp) {  // producer BatchNorm partials of remainder channel n
          const int nc = n < p.n ? n : p.n - 1;
          const __amdgpu_buffer_rsrc_t bxr = make_rsrc(p.bx, p.bx_bytes);
          const float x = load1(bxr, mok ? (uint32_t)(pix_of(mm) * p.bx_ps + n) * 4u : kOOB);
          const float gv =
              (p.brelu && !(__builtin_fmaf(x, p.bsave[2 * p.n + nc], p.bsave[3 * p.n + nc]) > 0.f))
                  ? 0.f : v;
          rsum[q] += mok ? gv : 0.f;
          rsq[q] += mok ? gv * (x - p.bsave[nc]) * p.bsave[p.n + nc] : 0.f;
        } else {
          rsum[q] += mok ? v : 0.f;
          rsq[q] += mok ? v * v : 0.f;
        }
      }
    }
  }
  if (p.stats) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      csum[j] += __shfl_xor(csum[j], 16, 64);
      csum[j] += __shfl_xor(csum[j], 32, 64);
      csq[j] += __shfl_xor(csq[j], 16, 64);
      csq[j] += __shfl_xor(csq[j], 32, 64);
    }
    if constexpr (NR > 0) {  // sum over the wave's pixels (the 16 lanes r of group g)
#pragma unroll
      for (int q = 0; q < NR; ++q) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          rsum[q] += __shfl_xor(rsum[q], o, 64);
          rsq[q] += __shfl_xor(rsq[q], o, 64);
        }
      }
      if (r == 0) {
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          if ((q & 3) != g) continue;
          red[wave][0][BN + q] = rsum[q];
          red[wave][1][BN + q] = rsq[q];
        }
      }
    }
    // partial row of this workgroup: class-major over the stride-parity classes (z)
    const int rows = gridDim.x * gridDim.z;
    const int srow = blockIdx.z * gridDim.x + bm;
    if (KS > 1) {  // wave 0 holds the whole row tile
      if (g == 0) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int n = n0 + j * 16 + r;
          if (n >= p.n) continue;
          p.stats[srow * p.n + n] = csum[j];
          p.stats[(rows + srow) * p.n + n] = csq[j];
        }
      }
      return;
    }
    if (g == 0) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        red[wave][0][j * 16 + r] = csum[j];
        red[wave][1][j * 16 + r] = csq[j];
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < BN + NR; c += 256) {
      if (n0 + c >= p.n) continue;
      float s = red[0][0][c] + red[1][0][c] + red[2][0][c] + red[3][0][c];
      float s2 = red[0][1][c] + red[1][1][c] + red[2][1][c] + red[3][1][c];
      p.stats[srow * p.n + n0 + c] = s;
      p.stats[(rows + srow) * p.n + n0 + c] = s2;
    }
  }
}


// ----------------------------------------------------- 1x1 GEMM (persistent) ----
// Large-M 1x1 / stride-1 convs (the layer-1 64 <-> 256 expansions and the 256 -> 64
// reductions at full resolution) and their data gradients: Y[m][n] = sum_k X[m][k] W[n][k]
// with W packed [Npad][K4] (mode 0; mode 1 for the data gradient is the same form).
// The gather kernel gives each wave ONE 32-row tile with K = 64 (4 chunks): a full
// load-latency prologue and an epilogue per 256 MFMAs, weights re-read per wave
// (PMC: 52 % of wave cycles waiting, MFMA 36 % busy).  Here a workgroup stages its N block
// of W (BN x K, zero past K) in LDS once; its 4 waves then stream row tiles of 16*TM pixels
// (tile = blockIdx.x*4 + wave, + gridDim.x*4 per step) with the A fragments loaded two K
// chunks ahead ACROSS tile boundaries, so the next tile's loads are in flight during this
// tile's MFMAs and epilogue.  BN statistics accumulate over the wave's tiles: one partial
// row per workgroup.
struct Gemm1 {
  const float* a;
  int a_ps, a_c, a_c4, M;
  const float* w;       // packed rows of a_c4 floats
  int n;                // GEMM N (real)
  const float* bias;
  float* y;
  int y_ps;
  float beta;
  float* stats;         // [2][gridDim.x][n] or null
  uint32_t a_bytes, w_bytes;
  int vec;              // y 16-byte aligned with y_ps % 4 == 0 (else 4-byte stores)
  // data gradient with bx set (round 6): stats receives the producer BatchNorm's backward
  // partials (sum g, sum g*xhat; g = y masked by the ReLU recomputed from bx), as IGemm
  const float* bx;
  int bx_ps, brelu;
  const float* bsave;
  uint32_t bx_bytes;
};

template <int TM, int TN>
__global__ __launch_bounds__(256) void gemm1x1_kernel(Gemm1 p) {
  constexpr int BN = 16 * TN;
  extern __shared__ __attribute__((aligned(16))) float bsh[];  // [BN][KL]
  __shared__ float red[4][2][BN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, r = lane & 15;
  const int n0 = blockIdx.y * BN;
  const int nch = (p.a_c4 + 15) >> 4;   // K chunks of 16
  const int KL = nch * 16 + 4;          // LDS row stride (floats): conflict-free b128 reads
  {
    const __amdgpu_buffer_rsrc_t wr = make_rsrc(p.w, p.w_bytes);
    const int q4 = nch * 4;  // quads per staged row
    for (int i = threadIdx.x; i < BN * q4; i += 256) {
      const int nn = i / q4, q = i - nn * q4;
      const bool ok = 4 * q < p.a_c4;  // (rows past the packed Npad: range check -> 0)
      const f4 v = load4(wr, ok ? (uint32_t)((n0 + nn) * p.a_c4 + 4 * q) * 4u : kOOB);
      *reinterpret_cast<f4*>(&bsh[nn * KL + 4 * q]) = v;
    }
  }
  const __amdgpu_buffer_rsrc_t ar = make_rsrc(p.a, p.a_bytes);
  const int ntiles = (p.M + 16 * TM - 1) / (16 * TM);
  const int t0 = blockIdx.x * 4 + wave, tstep = gridDim.x * 4;
  const int iters = t0 < ntiles ? (ntiles - t0 + tstep - 1) / tstep : 0;
  const int S = iters * nch;  // (tile, chunk) steps of this wave
  const bool cpad = (p.a_c & 3) != 0;
  float bv[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + j * 16 + r;
    bv[j] = (p.bias && n < p.n) ? p.bias[n] : 0.f;
  }
  f4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  float csum[TN], csq[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) { csum[j] = 0.f; csq[j] = 0.f; }
  const bool bnp = p.bx != nullptr;
  float pmn[TN], pis[TN], psc[TN], psh[TN];  // the producer BatchNorm's coefficients
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + j * 16 + r < p.n ? n0 + j * 16 + r : p.n - 1;
    pmn[j] = bnp ? p.bsave[n] : 0.f;
    pis[j] = bnp ? p.bsave[p.n + n] : 0.f;
    psc[j] = bnp ? p.bsave[2 * p.n + n] : 0.f;
    psh[j] = bnp ? p.bsave[3 * p.n + n] : 0.f;
  }
  const __amdgpu_buffer_rsrc_t bxr = make_rsrc(p.bx, bnp ? p.bx_bytes : 0u);
  __syncthreads();  // W staged

  auto load = [&](f4* fa, int st) {
    const int it = st / nch, c = st - it * nch;
    const int t = t0 + it * tstep;
    const int q = 16 * c + 4 * g;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = t * 16 * TM + i * 16 + r;
      const bool ok = st < S && m < p.M && q < p.a_c4;
      fa[i] = load4(ar, ok ? (uint32_t)(m * p.a_ps + q) * 4u : kOOB);
    }
  };
  auto mma = [&](f4* fa, int st) {
    const int it = st / nch, c = st - it * nch;
    if (cpad && c == nch - 1) {  // channels past a_c in the last quad (a wider buffer's)
      const int q = 16 * c + 4 * g;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        fa[i][1] = q + 1 < p.a_c ? fa[i][1] : 0.f;
        fa[i][2] = q + 2 < p.a_c ? fa[i][2] : 0.f;
        fa[i][3] = q + 3 < p.a_c ? fa[i][3] : 0.f;
      }
    }
    f4 fb[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
      fb[j] = *reinterpret_cast<const f4*>(&bsh[(j * 16 + r) * KL + 16 * c + 4 * g]);
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][s2], fb[j][s2], acc[i][j], 0, 0, 0);
  };
  auto epi = [&](int st) {
    const int it = st / nch, c = st - it * nch;
    if (c != nch - 1) return;
    // the tile's epilogue, then a fresh accumulator.  BN partial sums in the MFMA layout
    // (lane = column r, rows 4g..4g+3; statistics only with beta = 0), then each 16x16
    // tile is transposed inside lane quads (DPP) so a lane holds 4 consecutive channels
    // of one pixel: one 16-byte store instead of four 4-byte ones.
    const int t = t0 + it * tstep;
    const int k = r & 3, qc = 4 * (r >> 2);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int mb = t * 16 * TM + i * 16 + 4 * g;
      if (p.stats && bnp) {  // producer BatchNorm partials: one batch of range-checked loads
        float xv[4][TN];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int n = n0 + j * 16 + r;
            xv[e][j] = load1(bxr, mb + e < p.M && n < p.n
                                      ? (uint32_t)((mb + e) * p.bx_ps + n) * 4u : kOOB);
          }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const bool ok = mb + e < p.M && n0 + j * 16 + r < p.n;
            const float v = acc[i][j][e];
            const float x = xv[e][j];
            const float gv = (p.brelu && !(__builtin_fmaf(x, psc[j], psh[j]) > 0.f)) ? 0.f : v;
            csum[j] += ok ? gv : 0.f;
            csq[j] += ok ? gv * (x - pmn[j]) * pis[j] : 0.f;
          }
        }
      } else if (p.stats) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            if (mb + e < p.M && n0 + j * 16 + r < p.n) {
              const float v = acc[i][j][e] + bv[j];
              csum[j] += v;
              csq[j] += v * v;
            }
          }
        }
      }
      const int m = mb + k;
      float* yrow = p.y + (int64_t)m * p.y_ps;
      f4 yold[TN];  // beta: loaded before any store (one round trip per row tile)
      if (p.beta != 0.f) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int n = n0 + j * 16 + qc;
          yold[j] = (p.vec && m < p.M && n + 3 < p.n) ? *reinterpret_cast<const f4*>(yrow + n)
                                                      : f4{0.f, 0.f, 0.f, 0.f};
        }
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        f4 v = acc[i][j];
        acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
        quad_transpose(v, k);
        const int n = n0 + j * 16 + qc;
        if (m >= p.M || n >= p.n) continue;
        if (p.bias) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] += n + q < p.n ? p.bias[n + q] : 0.f;
        }
        if (p.vec && n + 3 < p.n) {
          if (p.beta != 0.f) v += p.beta * yold[j];
          *reinterpret_cast<f4*>(yrow + n) = v;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (n + q < p.n) yrow[n + q] = p.beta != 0.f ? v[q] + p.beta * yrow[n + q] : v[q];
        }
      }
    }
  };
  // Two chunks' loads in flight; a tile's epilogue stores go out after the loads of the
  // next two chunks (vmcnt counts stores too: a load issued after them would wait for them)
  if (S > 0) {
    f4 fa0[TM], fa1[TM];
    load(fa0, 0);
    load(fa1, 1);
    for (int st = 0; st < S; st += 2) {
      mma(fa0, st);
      load(fa0, st + 2);
      epi(st);
      if (st + 1 < S) {
        mma(fa1, st + 1);
        load(fa1, st + 3);
        epi(st + 1);
      }
    }
  }
  if (p.stats) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      csum[j] += __shfl_xor(csum[j], 16, 64);
      csum[j] += __shfl_xor(csum[j], 32, 64);
      csq[j] += __shfl_xor(csq[j], 16, 64);
      csq[j] += __shfl_xor(csq[j], 32, 64);
    }
    if (g == 0) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        red[wave][0][j * 16 + r] = csum[j];
        red[wave][1][j * 16 + r] = csq[j];
      }
    }
    __syncthreads();
    const int rows = gridDim.x;
    for (int c = threadIdx.x; c < BN; c += 256) {
      if (n0 + c >= p.n) continue;
      p.stats[blockIdx.x * p.n + n0 + c] = red[0][0][c] + red[1][0][c] + red[2][0][c] + red[3][0][c];
      p.stats[(rows + blockIdx.x) * p.n + n0 + c] =
          red[0][1][c] + red[1][1][c] + red[2][1][c] + red[3][1][c];
    }
  }
}

// 1x1 convs with many output channels ("wide"): up to 9 column tiles per wave and
// 32 rows, so the activation rows are re-read by 2 column blocks instead of 5.
static bool wide_ok(int64_t M, int N, int taps) {
  return g_wide_tiles && taps == 1 && N > 64 && M >= 65536;
}

Tile pick_tile(int64_t M, int N, bool wide) {
  Tile t;
  int tiles = (N + 15) / 16;
  if (wide && tiles > 4) {
    t.nblk = (tiles + 8) / 9;
    t.tn = (tiles + t.nblk - 1) / t.nblk;
    t.tm = 2;
    return t;
  }
  if (tiles <= 4) {
    t.tn = tiles;
    t.nblk = 1;
  } else {
    t.nblk = (tiles + 3) / 4;
    t.tn = (tiles + t.nblk - 1) / t.nblk;
  }
  // 4 waves per block, 16*TM rows per wave; large TM once there are enough rows
  t.tm = (M >= 64 * 4 * 256) ? 4 : (M >= 32 * 4 * 128 ? 2 : 1);
  return t;
}


static Tile pick_igemm_tile(int64_t M, int N, int taps, int k4, int ncls) {
  const bool wide = wide_ok(M, N, taps);
  Tile t = pick_tile(M, N, wide);
  // smaller row tiles until the grid reaches g_igemm_minblk workgroups (more waves per
  // SIMD for layers whose 4-row-tile grid leaves one wave per SIMD)
  while (!wide && g_igemm_minblk > 0 && t.tm > 1 &&
         ceil_div(M, 64 * t.tm) * t.nblk * ncls < g_igemm_minblk)
    t.tm >>= 1;
  const int64_t blocks = ceil_div(M, 64 * t.tm) * t.nblk * ncls;
  const int chunks = (taps * k4 + 15) / 16;
  if (g_ksplit && !wide && blocks < 512 && chunks >= 16) t.ks = 4;
  // tune key 6: 18 / 36 output channels as 16 + 2 / 32 + 4 (VALU remainder, fp32, no K split);
  // 2: 18 channels only
  if (g_igemm_nr && !g_bf16 && t.ks == 1 && !wide && (N == 18 || (N == 36 && g_igemm_nr == 1))) {
    t.tn = N == 18 ? 1 : 2;
    t.nr = N == 18 ? 2 : 4;
    t.nblk = 1;
  }
  return t;
}

IGemmPlan igemm_plan(const IGemm& p, int ncls) {
  IGemmPlan pl;
  pl.M = (int64_t)p.g_n * p.g_h * p.g_w;
  pl.max_taps = p.nth * p.ntw;
  for (int c = 0; c < ncls && ncls > 1; ++c) {
    const IGemm::Cls& k = p.cls[c];
    const int64_t mc = (int64_t)p.g_n * k.g_h * k.g_w;
    if (c == 0 || mc > pl.M) pl.M = mc;
    if (k.nth * k.ntw > pl.max_taps) pl.max_taps = k.nth * k.ntw;
  }
  pl.t = pick_igemm_tile(pl.M, p.n, pl.max_taps, p.a_c4, ncls);
  // Rows per workgroup: layers whose row tiles would leave the chip with fewer than ~2 waves
  // per SIMD split K over the workgroup's 4 waves instead (when K has at least 16 chunks of
  // 16), giving 4x the workgroups.
  const int64_t rows_per_block = (pl.t.ks > 1 ? 16 : 64) * pl.t.tm;
  pl.grid = dim3((unsigned)ceil_div(pl.M, rows_per_block), (unsigned)pl.t.nblk, (unsigned)ncls);
  return pl;
}

static int gemm1_blocks_per_cu(int tm, int tn, size_t lds);

bool gemm1_pick(const vae2_act* ad, const vae2_act* yd, int k, int stride, int pad,
                const float* a, G1Tile* out) {
  if (!g_gemm1 || g_bf16 || g_conv_algo == 1) return false;
  if (k != 1 || stride != 1 || pad != 0 || ad->h != yd->h || ad->w != yd->w) return false;
  const int64_t M = act_pixels(yd);
  const int N = (int)yd->c;
  if (M < 65536 || N < 48 || !vec_ok(a, (int)ad->ps)) return false;
  const int k4 = round_up((int)ad->c, 4);
  const int tiles = (N + 15) / 16;
  G1Tile t;
  const int tn_max = g_gemm1_tn >= 3 && g_gemm1_tn <= 8 ? g_gemm1_tn : 4;
  t.nblk = (tiles + tn_max - 1) / tn_max;
  t.tn = (tiles + t.nblk - 1) / t.nblk;
  if (t.tn < 3) t.tn = 3;
  const int nch = (k4 + 15) / 16;
  t.lds = (size_t)16 * t.tn * (nch * 16 + 4) * sizeof(float);
  if (t.lds > 96 * 1024) return false;
  // resident workgroups per CU (registers and LDS; the TN = 8 instance holds 264 VGPRs:
  // one wave per SIMD) -- the persistent grid is exactly that many per CU
  t.tm = g_gemm1_tm == 1 ? 1 : 2;  // tune key 5: 16-row tiles (half the accumulators)
  const int per_cu = gemm1_blocks_per_cu(t.tm, t.tn, t.lds);
  const int64_t ntiles = ceil_div(M, 16 * t.tm);
  int64_t gx = 256 * per_cu / t.nblk;
  if (gx > ceil_div(ntiles, 4)) gx = ceil_div(ntiles, 4);
  t.grid_x = (int)(gx < 1 ? 1 : gx);
  if (out) *out = t;
  return true;
}

template <int TM, bool VEC, int ROLE, int KS = 1>
static void launch_tn(const IGemm& p, int tn, dim3 grid, hipStream_t s) {
  switch (tn) {
#define CASE(T) \
  case T:                                                                         \
    if (g_bf16) VAE2_LAUNCH((igemm_kernel<TM, T, VEC, ROLE, KS, true>), grid, dim3(256), 0, s, p); \
    else VAE2_LAUNCH((igemm_kernel<TM, T, VEC, ROLE, KS>), grid, dim3(256), 0, s, p);   \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4)
#undef CASE
  }
}

template <bool VEC, int ROLE>
static void launch_wide(const IGemm& p, int tn, dim3 grid, hipStream_t s) {
  switch (tn) {
#define CASE(T) \
  case T:                                                                         \
    if (g_bf16) VAE2_LAUNCH((igemm_kernel<2, T, VEC, ROLE, 1, true>), grid, dim3(256), 0, s, p); \
    else VAE2_LAUNCH((igemm_kernel<2, T, VEC, ROLE>), grid, dim3(256), 0, s, p);       \
    break;
    CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9)
#undef CASE
  }
}

template <bool VEC, int ROLE>
static void launch_nr(const IGemm& p, const Tile& t, dim3 grid, hipStream_t s) {
#define NRL(TM_)                                                                             \
  if (t.nr == 2) VAE2_LAUNCH((igemm_kernel<TM_, 1, VEC, ROLE, 1, false, 2>), grid, dim3(256), 0, s, p); \
  else VAE2_LAUNCH((igemm_kernel<TM_, 2, VEC, ROLE, 1, false, 4>), grid, dim3(256), 0, s, p);
  if (t.tm == 4) { NRL(4) }
  else if (t.tm == 2) { NRL(2) }
  else { NRL(1) }
#undef NRL
}
template <bool VEC, int ROLE>
static void launch_tm(const IGemm& p, const Tile& t, dim3 grid, hipStream_t s) {
  if (t.nr) {
    launch_nr<VEC, ROLE>(p, t, grid, s);
    return;
  }
  if (t.ks > 1) {  // (never with wide tiles: those need >= 65536 rows)
    if (t.tm == 4) launch_tn<4, VEC, ROLE, 4>(p, t.tn, grid, s);
    else if (t.tm == 2) launch_tn<2, VEC, ROLE, 4>(p, t.tn, grid, s);
    else launch_tn<1, VEC, ROLE, 4>(p, t.tn, grid, s);
    return;
  }
  if (t.tm == 2 && t.tn > 4) launch_wide<VEC, ROLE>(p, t.tn, grid, s);
  else if (t.tm == 4) launch_tn<4, VEC, ROLE>(p, t.tn, grid, s);
  else if (t.tm == 2) launch_tn<2, VEC, ROLE>(p, t.tn, grid, s);
  else launch_tn<1, VEC, ROLE>(p, t.tn, grid, s);
}

// ncls > 1: p.cls[0..ncls) hold the parity classes; the grid covers the largest one.
int launch_igemm(IGemm& p, int role, hipStream_t s, const char* fn, int ncls) {
  const IGemmPlan pl = igemm_plan(p, ncls);
  if (pl.M == 0) return 0;
  p.ktab = g_igemm_tab;
  for (int c = 0; c < ncls && ncls > 1; ++c) {
    IGemm::Cls& k = p.cls[c];
    k.hw_div = FastDiv((uint32_t)(k.g_h * k.g_w));
    k.w_div = FastDiv((uint32_t)k.g_w);
  }
  p.vec_out = g_vec_out && vec_ok(p.y, p.y_ps) && !(p.stats && p.beta != 0.f);
  p.hw_div = FastDiv((uint32_t)(p.g_h * p.g_w));
  p.w_div = FastDiv((uint32_t)p.g_w);
  bool vec = vec_ok(p.a, p.a_ps);
  if (role == 0) {
    if (vec) launch_tm<true, 0>(p, pl.t, pl.grid, s);
    else launch_tm<false, 0>(p, pl.t, pl.grid, s);
  } else {
    if (vec) launch_tm<true, 1>(p, pl.t, pl.grid, s);
    else launch_tm<false, 1>(p, pl.t, pl.grid, s);
  }
  return check_launch(fn);
}


// hipOccupancyMaxActiveBlocksPerMultiprocessor of gemm1x1_kernel<tm, tn> with `lds` bytes
// of dynamic LDS (cached per (tm, tn, lds)); at least 1.
static int gemm1_blocks_per_cu(int tm, int tn, size_t lds) {
  static int cache[3][9][4] = {};
  static size_t cache_lds[3][9][4] = {};
  if (tn < 3 || tn > 8 || tm < 1 || tm > 2) return 1;
  for (int i = 0; i < 4; ++i)
    if (cache[tm][tn][i] && cache_lds[tm][tn][i] == lds) return cache[tm][tn][i];
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
#define CASE(M, T)                                                                       \
  case T:                                                                                \
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(                                    \
        &n, reinterpret_cast<const void*>(gemm1x1_kernel<M, T>), 256, lds);              \
    break;
  if (tm == 1) {
    switch (tn) { CASE(1, 3) CASE(1, 4) CASE(1, 5) CASE(1, 6) CASE(1, 7) CASE(1, 8) }
  } else {
    switch (tn) { CASE(2, 3) CASE(2, 4) CASE(2, 5) CASE(2, 6) CASE(2, 7) CASE(2, 8) }
  }
#undef CASE
  if (e != hipSuccess || n < 1) {
    (void)hipGetLastError();
    n = 1;
  }
  for (int i = 0; i < 4; ++i)
    if (!cache[tm][tn][i]) {
      cache[tm][tn][i] = n;
      cache_lds[tm][tn][i] = lds;
      break;
    }
  return n;
}

int launch_gemm1(const float* a, const vae2_act* ad, const float* wp, uint32_t w_bytes,
                 const float* bias, float* y, const vae2_act* yd, float beta, float* stats,
                 const G1Tile& t, hipStream_t s, const char* fn, const float* bx, int bx_ps,
                 int brelu, const float* bsave, uint32_t bx_bytes) {
  // (16-byte stores of whole channel quads where y is aligned, 4-byte stores otherwise, so
  // the statistics rows vae2_conv2d_fwd_stats_rows reports do not depend on y's alignment;
  // statistics are of the fresh output only)
  if (stats && beta != 0.f) return -1;
  Gemm1 p{};
  p.bx = bx; p.bx_ps = bx_ps; p.brelu = brelu; p.bsave = bsave; p.bx_bytes = bx_bytes;
  p.vec = vec_ok(y, (int)yd->ps) ? 1 : 0;
  p.a = a; p.a_ps = (int)ad->ps; p.a_c = (int)ad->c; p.a_c4 = round_up((int)ad->c, 4);
  p.M = (int)act_pixels(yd);
  p.w = wp; p.n = (int)yd->c; p.bias = bias; p.y = y; p.y_ps = (int)yd->ps; p.beta = beta;
  p.stats = stats; p.a_bytes = act_bytes(ad); p.w_bytes = w_bytes;
  const dim3 grid((unsigned)t.grid_x, (unsigned)t.nblk);
#define CASE(M, T) \
  case T: VAE2_LAUNCH((gemm1x1_kernel<M, T>), grid, dim3(256), t.lds, s, p); break;
  if (t.tm == 1) {
    switch (t.tn) {
      CASE(1, 3) CASE(1, 4) CASE(1, 5) CASE(1, 6) CASE(1, 7) CASE(1, 8)
      default: return fail(fn, "gemm1x1: unsupported N block");
    }
  } else {
    switch (t.tn) {
      CASE(2, 3) CASE(2, 4) CASE(2, 5) CASE(2, 6) CASE(2, 7) CASE(2, 8)
      default: return fail(fn, "gemm1x1: unsupported N block");
    }
  }
#undef CASE
  return check_launch(fn);
}


}  // namespace vae2

// Direct 3x3 / stride-1 convolutions (LDS-tiled halo): dconv3_kernel, its grouped form,
// the rules that choose it over the gather kernel, its launchers and vae2_conv2d_multi.
#include "conv.h"

// Diagnostic builds only (never the shipped library): -DVAE2_ABLATE=1 stages zeros
// instead of loading the direct kernel's halo tile, 2 drops its output stores, 4 skips its
// MFMA main loop (bits combine).
#ifndef VAE2_ABLATE
#define VAE2_ABLATE 0
#endif

namespace vae2 {

// ------------------------------------------------------ direct 3x3 (LDS) ----
// 3x3 / stride-1 / pad-1 convolutions (the HRNet branch convs) — forward, and the
// data gradient with flipped taps and mode-1 weights.  A workgroup owns an output
// tile of (2*TM) rows x 32 columns of one image; per slab of <= 32 input channels it
// stages the (2*TM+2) x 34 halo tile in LDS once (zero halo, zero channel padding),
// then builds every tap's A fragment from LDS with one ds_read_b128 per lane.  The
// gather kernel re-reads each input element once per tap through L1/L2; here it is
// read once (+ halo).  K order inside a slab is (tap, quad), lane group g taking quad
// 4c+g of chunk c (as igemm_kernel), so B comes from the same packed weights.
struct DConv {
  const float* a;
  int a_ps, a_c, a_c4, img_h, img_w;
  int tiles_h, tiles_w;  // output tiles per image
  int cs4;               // channel quads per slab
  const float* w;        // packed [Npad][9][a_c4]
  uint32_t a_bytes, w_bytes;
  int n;
  const float* bias;
  float* y;
  int y_ps;
  float beta;
  float* stats;  // [2][gridDim.x][n] or null
  // Forward (FLIP = false): the input is the pre-BN output of a BatchNorm(+ReLU) layer
  // whose normalised activation is never stored: staging applies relu?(a*scale + shift)
  // (isave = that layer's (mean, invstd, scale, shift) [4][a_c]) to in-image pixels, the
  // zero halo stays zero.
  const float* isave;
  int irelu;
  // Data gradient (FLIP = true): this output is the gradient of such a layer's (never
  // stored) output; the epilogue writes that layer's BatchNorm backward partials (sum g,
  // sum g*xhat; g = the gradient masked by its ReLU) into stats instead of (sum, sum^2).
  // bx = the layer's pre-BN tensor (same pixels and channels as y), bsave its [4][n].
  const float* bx;
  int bx_ps, brelu;
  const float* bsave;
  uint32_t bx_bytes;  // bx extent for the range-checked epilogue loads
  int vec_out;  // y 16-byte aligned, y_ps % 4 == 0, no statistics with beta != 0
};

constexpr int kDcBW = 32;     // tile columns
constexpr int kDcMaxCs4 = 8;  // quads per slab
// (A offset, weight offset) of every K step of a slab (chunks of 4 (tap, quad) steps, an
// even number of chunks, + the 2 chunks the loop prefetches past the end), in LDS after
// the tile and the remainder weights
constexpr int kDcTab = ((9 * kDcMaxCs4 + 7) / 8) * 8 + 32;  // (+ 8 KS, KS <= 4)

// One output tile: bm = tile index (image-major), by = N block, nrows = tiles of the
// layer (rows of its BN partial statistics).
//
// NR > 0 (fp32 operands, one N block): the layer's last NR output channels (N = 16*TN +
// NR, NR in {2, 4, 8}: the 18 / 36 / 72-channel branches) are computed on the VALU
// beside the MFMAs instead of in a further 16-wide MFMA tile that would be mostly
// padding: lane = one output pixel of the wave's 16*TM (and, at TM = 2, one half of the
// NR channels), v_fma_f32 chains over the same (tap, channel) K order the chunks walk,
// with the remainder weights of the slab staged in LDS (broadcast reads).  The MFMA work
// of an 18-channel layer halves (32 -> 16 columns), of a 36-channel one drops by 1/3.
// BNX (compile time, so the plain instances carry none of it): 1 = input BatchNorm in the
// staging (DConv::isave, forward), 2 = producer BatchNorm backward partials in the
// epilogue (DConv::bx, data gradient).
// NW = waves per workgroup (4, or 8 with TM = 2: the same 8-row tile as TM = 4, each wave
// owning one row -- twice the waves per SIMD for the same LDS tile)
// KS > 1 (NW = 4 KS, NR = 0, fp32 operands): the 4 row waves' tile of the NW = 4 form with
// the K chunk pairs split between KS wave sets (set s: pairs s, s + KS, s + 2 KS, ...), sets
// 1 .. KS-1's accumulators added to set 0's through LDS in a fixed order before the epilogue
// -- KS waves per SIMD for layers whose tiles give one workgroup per CU (set_tune key 15)
template <int TM, int TN, bool FLIP, bool BF, int NR = 0, int BNX = 0, int NW = 4,
          int KS = 1>
__device__ __forceinline__ void dconv3_body(const DConv& p, const int bm, const int by,
                                            const int nrows, float* __restrict__ tile) {
  constexpr int NT = 64 * NW;
  constexpr int NWR = NW / KS;  // waves per K share: the tile's row waves
  static_assert(KS == 1 || (NW == 4 * KS && NR == 0 && !BF), "K split form");
  constexpr int BH = NWR * TM / 2, LH = BH + 2, LW = kDcBW + 2;
  constexpr int BN = 16 * TN;
  constexpr int BNT = BN + NR;             // channels of this block (MFMA + VALU)
  static_assert(NR == 0 || (!BF && NR <= 8), "remainder shape");
  __shared__ float red[NW][2][BNT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave % NWR, kp = wave / NWR;  // row wave, K share
  const int g = lane >> 4, r = lane & 15;
  const int per_img = p.tiles_h * p.tiles_w;
  const int img = bm / per_img;
  const int trem = bm - img * per_img;
  const int th = trem / p.tiles_w;
  const int oh0 = th * BH, ow0 = (trem - th * p.tiles_w) * kDcBW;
  // first output row of this wave (K shares > 0 of the KS form: past the image, so their
  // epilogue stores, loads and statistics are all masked off)
  const int ohw = kp ? (1 << 24) : oh0 + wr * (TM / 2);
  const int n0 = by * BNT;  // (NR > 0 with two N blocks: 72 = 2 x (32 + 4), set_tune key 14)
  const int kk4 = 9 * p.a_c4;
  const int csp = p.cs4 * 4 + 4;  // LDS floats per pixel (+4: bank spread)
  const int Q = p.a_c4 >> 2;

  int abase[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int trow = wr * (TM / 2) + (i >> 1), tcol = (i & 1) * 16 + r;
    abase[i] = ((trow + 1) * LW + tcol + 1) * csp;
  }
  const __amdgpu_buffer_rsrc_t arsrc = make_rsrc(p.a, p.a_bytes);
  const __amdgpu_buffer_rsrc_t wrsrc = make_rsrc(p.w, p.w_bytes);
  uint32_t wrow[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) wrow[j] = (uint32_t)((n0 + j * 16 + r) * kk4) * 4u;

  f4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
  f4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  auto mma = [&](const f4* fa, const f4* fb) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);
  };
  // VALU remainder: lane (g, r) multiplies the A fragments it already holds (pixels
  // i*16 + r of its TM row tiles, the 4 channels of K step 4c + g) with that K step's
  // remainder weights; the 4 lane groups' shares are summed at the end.  The slab's
  // remainder weights rw[NR][(tap, quad) step][4] live in LDS.
  float* const rw = tile + LH * LW * csp;
  // floats per remainder channel in rw: the K steps of an even number of chunks (the main
  // loop runs chunks in pairs), zero past the slab's 9 x qs steps
  const int rws = ((9 * p.cs4 + 7) >> 3) * 32;
  int2* const tab = reinterpret_cast<int2*>(rw + NR * rws);
  float racc[TM][NR > 0 ? NR : 1];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) racc[i][j] = 0.f;

  const int img_base = img * p.img_h;
  for (int q0 = 0; q0 < Q; q0 += p.cs4) {
    const int qs = Q - q0 < p.cs4 ? Q - q0 : p.cs4;
    // ---- stage the halo tile of this slab (zero outside the image / past a_c) ----
    __syncthreads();
    const int nch = (9 * qs + 3) >> 2;
    {  // the slab's K-step table: entry k = (tap, quad) step k of the chunk sequence
      const int k = threadIdx.x;
      // (steps past the 9 taps: zero weights; the KS form prefetches up to 2 (KS - 1)
      //  chunks further)
      if (k < ((nch + 1) >> 1) * 8 + 8 * KS) {
        const int t = k / qs, q = k - t * qs;
        const bool tv = t < 9;
        const int tt = tv ? t : 0;
        const int dh = tt / 3 - 1, dw = tt - 3 * (tt / 3) - 1;
        const int tl = FLIP ? 8 - tt : tt;
        tab[k] = make_int2((dh * LW + dw) * csp + 4 * q,
                           tv ? (int)((uint32_t)(tl * p.a_c4 + (q0 + q) * 4) * 4u) : (int)kOOB);
      }
    }
    if constexpr (NR > 0) {  // remainder weights of the slab [j][(tap, quad)][4], FLIP
      const int per = ((9 * qs + 7) >> 3) * 32;  // whole chunk pairs: zero tail
      for (int i = threadIdx.x; i < NR * per; i += NT) {
        const int j = i / per, rem = i - j * per;
        const int t = rem / (qs * 4), c = rem - t * (qs * 4);
        const int tl = FLIP ? 8 - t : t;
        rw[j * rws + rem] =
            t < 9 ? p.w[(int64_t)(n0 + BN + j) * kk4 + tl * p.a_c4 + q0 * 4 + c] : 0.f;
      }
    }
    // thread -> (channel quad q = tid % qs, pixels pb, pb + pstride, ...); SB loads in
    // flight per thread before their LDS stores (few round trips, few extra registers)
    constexpr int SB = 3;
    {
    const int sq = threadIdx.x % qs, pb = threadIdx.x / qs, pstride = NT / qs;
    const int c = (q0 + sq) * 4;
    const bool cpad = c + 4 > p.a_c;
    // input BatchNorm (FLIP = false only): this thread's channel quad's scale / shift
    f4 isc, ish;
    if (BNX == 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ch = c + k < p.a_c ? c + k : p.a_c - 1;
        isc[k] = p.isave[2 * p.a_c + ch];
        ish[k] = p.isave[3 * p.a_c + ch];
      }
    }
    if (pb < pstride) {
      for (int pix0 = pb; pix0 < LH * LW; pix0 += SB * pstride) {
        f4 v[SB];
        bool okv[SB];
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          const int pix = pix0 + u * pstride;
          const int lr = pix / LW, lc = pix - lr * LW;
          const int ih = oh0 - 1 + lr, iw = ow0 - 1 + lc;
          const bool ok = pix < LH * LW && (unsigned)ih < (unsigned)p.img_h &&
                          (unsigned)iw < (unsigned)p.img_w;
          okv[u] = ok;
          if (VAE2_ABLATE & 1) v[u] = f4{(float)pix, (float)ih, (float)iw, (float)c};
          else
          v[u] = load4(arsrc, ok ? (uint32_t)(((img_base + ih) * p.img_w + iw) * p.a_ps + c) * 4u
                                 : kOOB);
        }
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          const int pix = pix0 + u * pstride;
          if (pix >= LH * LW) break;
          if (BNX == 1 && okv[u]) {  // = bn_apply_body's arithmetic
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const float t = __builtin_fmaf(v[u][k], isc[k], ish[k]);
              v[u][k] = (p.irelu && t < 0.f) ? 0.f : t;
            }
          }
          if (cpad) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (c + k >= p.a_c) v[u][k] = 0.f;
          }
          *reinterpret_cast<f4*>(&tile[pix * csp + 4 * sq]) = v[u];
        }
      }
    }
    }
    __syncthreads();
    // ---- 9 taps x qs quads of K from LDS ----
    // chunk c, lane group g: K step 4c + g, its A / weight offsets from the table
    int kc = g + 8 * kp;  // (K share kp starts at chunk pair kp)
    auto load = [&](f4* fa, f4* fb) {
      const int2 e = tab[kc];
      kc += 4;
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const f4*>(&tile[abase[i] + e.x]);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = load4(wrsrc, wrow[j] + (uint32_t)e.y);
    };
    // the remainder's share of a chunk: this lane's K step (4c + g) against the A
    // fragments of the MFMAs (steps past the 9 taps meet the zeroed tail of rw)
    int rch = 0;
    auto rem = [&](const f4* fa) {
      if constexpr (NR > 0) {
        const int ks = 4 * rch + g;
        ++rch;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          const f4 wv = *reinterpret_cast<const f4*>(&rw[j * rws + 4 * ks]);
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            racc[i][j] = __builtin_fmaf(fa[i][0], wv[0], racc[i][j]);
            racc[i][j] = __builtin_fmaf(fa[i][1], wv[1], racc[i][j]);
            racc[i][j] = __builtin_fmaf(fa[i][2], wv[2], racc[i][j]);
            racc[i][j] = __builtin_fmaf(fa[i][3], wv[3], racc[i][j]);
          }
        }
      }
    };
    if (!BF) {
      load(fa0, fb0);
      for (int ch = 2 * kp; ch < ((VAE2_ABLATE & 4) ? 0 : nch); ch += 2 * KS) {
        load(fa1, fb1);
        if (KS > 1) kc += 8 * (KS - 1);  // (the other shares' pairs)
        mma(fa0, fb0);
        rem(fa0);
        load(fa0, fb0);
        mma(fa1, fb1);
        rem(fa1);
      }
    } else {  // bf16 operands: one 16x16x32 MFMA per chunk pair
      load(fa0, fb0);
      load(fa1, fb1);
      for (int ch = 0; ch < nch; ch += 2) {
        bf16x8 A[TM], B[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) A[i] = pack_bf16(fa0[i], fa1[i]);
#pragma unroll
        for (int j = 0; j < TN; ++j) B[j] = pack_bf16(fb0[j], fb1[j]);
        load(fa0, fb0);
        load(fa1, fb1);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[i], B[j], acc[i][j], 0, 0, 0);
      }
    }
  }

  if constexpr (KS > 1) {  // K shares 1 .. KS-1's accumulators onto share 0's (fixed order)
    __syncthreads();  // every wave's last reads of the tile are done
    f4* const kred = reinterpret_cast<f4*>(tile);  // [KS - 1][NWR][TM][TN][64]
    if (kp) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          kred[((((kp - 1) * NWR + wr) * TM + i) * TN + j) * 64 + lane] = acc[i][j];
    }
    __syncthreads();
    if (!kp) {
#pragma unroll
      for (int sh = 0; sh < KS - 1; ++sh)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] += kred[(((sh * NWR + wr) * TM + i) * TN + j) * 64 + lane];
    }
  }

  // ---- epilogue (bias, beta*y, BN partial statistics) ----
  float csum[TN], csq[TN];
  // producer BatchNorm backward partials (FLIP with bx): per-column mean, invstd, scale,
  // shift of that layer (= bn_bwd_reduce_body's arithmetic, element by element)
  constexpr bool bnp = BNX == 2;
  float bmn[TN], bis[TN], bsc[TN], bsh[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    csum[j] = 0.f; csq[j] = 0.f;
    if (bnp) {
      const int n = n0 + j * 16 + r < p.n ? n0 + j * 16 + r : p.n - 1;
      bmn[j] = p.bsave[n]; bis[j] = p.bsave[p.n + n];
      bsc[j] = p.bsave[2 * p.n + n]; bsh[j] = p.bsave[3 * p.n + n];
    }
  }
  if (p.vec_out) {
    // statistics in the MFMA layout (beta = 0 whenever they are requested), then each
    // 16x16 tile transposed inside lane quads: one 16-byte store per lane and tile
    const int k = r & 3, qc = 4 * (r >> 2);
    // beta (a data gradient summed onto a GradLink buffer): every old output quad of the
    // tile loaded before any store (loads cannot pass the stores to y: one round trip
    // instead of one per quad)
    constexpr bool PFA = TM * TN <= 8;
    f4 yold[PFA ? TM : 1][TN];
    auto yrow_of = [&](int i) {
      const int oh = ohw + (i >> 1), ow = ow0 + (i & 1) * 16 + g * 4 + k;
      const bool pok = oh < p.img_h && ow < p.img_w;
      return pok ? p.y + ((int64_t)(img_base + oh) * p.img_w + ow) * p.y_ps : nullptr;
    };
    auto prefetch = [&](int i, f4* yo) {
      const float* yr = yrow_of(i);
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + j * 16 + qc;
        yo[j] = (yr && n + 3 < p.n) ? *reinterpret_cast<const f4*>(yr + n) : f4{0.f, 0.f, 0.f, 0.f};
      }
    };
    if (PFA && p.beta != 0.f) {
#pragma unroll
      for (int i = 0; i < (PFA ? TM : 1); ++i) prefetch(i, yold[i]);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int oh = ohw + (i >> 1);
      if (p.stats && bnp) {
        // the row tile's 4 x TN pre-BN values in one batch of range-checked loads (one
        // round trip; loads guarded by branches waited on each element in turn)
        const __amdgpu_buffer_rsrc_t bxr = make_rsrc(p.bx, p.bx_bytes);
        float xv[4][TN];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ow = ow0 + (i & 1) * 16 + g * 4 + e;
          const bool pin = oh < p.img_h && ow < p.img_w;
          const int64_t pix = pin ? (int64_t)(img_base + oh) * p.img_w + ow : 0;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int n = n0 + j * 16 + r;
            xv[e][j] = load1(bxr, pin && n < p.n ? (uint32_t)((pix * p.bx_ps + n) * 4) : kOOB);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ow = ow0 + (i & 1) * 16 + g * 4 + e;
          const bool pin = oh < p.img_h && ow < p.img_w;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int n = n0 + j * 16 + r;
            const float v = acc[i][j][e] + (p.bias && n < p.n ? p.bias[n] : 0.f);
            const float x = xv[e][j];
            const float gv = (p.brelu && !(__builtin_fmaf(x, bsc[j], bsh[j]) > 0.f)) ? 0.f : v;
            const bool ok = pin && n < p.n;
            csum[j] += ok ? gv : 0.f;
            csq[j] += ok ? gv * (x - bmn[j]) * bis[j] : 0.f;
          }
        }
      } else if (p.stats) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ow = ow0 + (i & 1) * 16 + g * 4 + e;
          if (oh >= p.img_h || ow >= p.img_w) continue;
          const int64_t pix = (int64_t)(img_base + oh) * p.img_w + ow;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int n = n0 + j * 16 + r;
            if (n >= p.n) continue;
            const float v = acc[i][j][e] + (p.bias ? p.bias[n] : 0.f);
            if (bnp) {
              const float xv = p.bx[pix * p.bx_ps + n];
              const float gv = (p.brelu && !(__builtin_fmaf(xv, bsc[j], bsh[j]) > 0.f)) ? 0.f : v;
              csum[j] += gv;
              csq[j] += gv * (xv - bmn[j]) * bis[j];
            } else {
              csum[j] += v;
              csq[j] += v * v;
            }
          }
        }
      }
      float* yrow = yrow_of(i);
      const bool pok = yrow != nullptr;
      f4 yrt[PFA ? 1 : TN];
      if (!PFA && p.beta != 0.f) prefetch(i, yrt);
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        f4 v = acc[i][j];
        quad_transpose(v, k);
        const int n = n0 + j * 16 + qc;
        if (!pok || n >= p.n) continue;
        if (p.bias) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] += n + q < p.n ? p.bias[n + q] : 0.f;
        }
        if (n + 3 < p.n) {
          if (p.beta != 0.f) v += p.beta * (PFA ? yold[PFA ? i : 0][j] : yrt[PFA ? 0 : j]);
          if (!(VAE2_ABLATE & 2) || v[0] == 1234.5f) *reinterpret_cast<f4*>(yrow + n) = v;
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
    const int oh = ohw + (i >> 1);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ow = ow0 + (i & 1) * 16 + g * 4 + e;
      if (oh >= p.img_h || ow >= p.img_w) continue;
      const int64_t pix = (int64_t)(img_base + oh) * p.img_w + ow;
      float* yrow = p.y + pix * p.y_ps;
      const float* xrow = bnp ? p.bx + pix * p.bx_ps : nullptr;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + j * 16 + r;
        if (n >= p.n) continue;
        float v = acc[i][j][e];
        if (p.bias) v += p.bias[n];
        if (p.beta != 0.f) v += p.beta * yrow[n];
        if (!(VAE2_ABLATE & 2) || v == 1234.5f) yrow[n] = v;
        if (bnp) {
          const float xv = xrow[n];
          const float gv = (p.brelu && !(__builtin_fmaf(xv, bsc[j], bsh[j]) > 0.f)) ? 0.f : v;
          csum[j] += gv;
          csq[j] += gv * (xv - bmn[j]) * bis[j];
        } else {
          csum[j] += v;
          csq[j] += v * v;
        }
      }
    }
  }
  // the VALU remainder's outputs: the 4 lane groups' K-step shares summed (every group
  // then holds pixel i*16 + r's sums); lane group g writes the channels j = g (mod 4)
  float rsum[NR > 0 ? NR : 1], rsq[NR > 0 ? NR : 1];
  if constexpr (NR > 0) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        racc[i][j] += __shfl_xor(racc[i][j], 16, 64);
        racc[i][j] += __shfl_xor(racc[i][j], 32, 64);
      }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      rsum[j] = 0.f;
      rsq[j] = 0.f;
      if ((j & 3) != g) continue;
      const int n = n0 + BN + j;
      float bxv[TM];  // the pre-BN values of the TM pixels, one batch of loads (bnp)
      if (bnp) {
        const __amdgpu_buffer_rsrc_t bxr = make_rsrc(p.bx, p.bx_bytes);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int oh = ohw + (i >> 1), ow = ow0 + (i & 1) * 16 + r;
          const bool in = oh < p.img_h && ow < p.img_w;
          const int64_t pix = (int64_t)(img_base + (in ? oh : 0)) * p.img_w + (in ? ow : 0);
          bxv[i] = load1(bxr, in ? (uint32_t)((pix * p.bx_ps + n) * 4) : kOOB);
        }
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int oh = ohw + (i >> 1), ow = ow0 + (i & 1) * 16 + r;
        const bool in = oh < p.img_h && ow < p.img_w;
        const int64_t pix = (int64_t)(img_base + (in ? oh : 0)) * p.img_w + (in ? ow : 0);
        float* yp = p.y + pix * p.y_ps + n;
        float v = racc[i][j];
        if (p.bias) v += p.bias[n];
        if (p.beta != 0.f && in) v += p.beta * *yp;
        if (in && (!(VAE2_ABLATE & 2) || v == 1234.5f)) *yp = v;
        if (bnp) {
          const float xv = bxv[i];
          const float gv = (p.brelu && !(__builtin_fmaf(xv, p.bsave[2 * p.n + n],
                                                        p.bsave[3 * p.n + n]) > 0.f)) ? 0.f : v;
          rsum[j] += in ? gv : 0.f;
          rsq[j] += in ? gv * (xv - p.bsave[n]) * p.bsave[p.n + n] : 0.f;
        } else {
          rsum[j] += in ? v : 0.f;
          rsq[j] += in ? v * v : 0.f;
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
    if (g == 0) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        red[wave][0][j * 16 + r] = csum[j];
        red[wave][1][j * 16 + r] = csq[j];
      }
    }
    if constexpr (NR > 0) {  // sum over the wave's pixels (the 16 lanes r of group g)
#pragma unroll
      for (int j = 0; j < NR; ++j) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          rsum[j] += __shfl_xor(rsum[j], o, 64);
          rsq[j] += __shfl_xor(rsq[j], o, 64);
        }
      }
      if (r == 0) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          if ((j & 3) != g) continue;
          red[wave][0][BN + j] = rsum[j];
          red[wave][1][BN + j] = rsq[j];
        }
      }
    }
    __syncthreads();
    const int rows = nrows;
    for (int c = threadIdx.x; c < BNT; c += NT) {
      if (n0 + c >= p.n) continue;
      float s = red[0][0][c], s2 = red[0][1][c];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        s += red[w][0][c];
        s2 += red[w][1][c];
      }
      p.stats[bm * p.n + n0 + c] = s;
      p.stats[(rows + bm) * p.n + n0 + c] = s2;
    }
  }
}

template <int TM, int TN, bool FLIP, bool BF = false, int NR = 0, int BNX = 0, int NW = 4,
          int KS = 1>
__global__ __launch_bounds__(64 * NW, (TM == 4 && TN == 4 && NR == 0 && NW == 4) ? 3 : 1) void dconv3_kernel(DConv p) {
  static_assert(BNX == 0 || (!BF && (BNX == 1) != FLIP), "input BN: forward; partials: dgrad");
  extern __shared__ __attribute__((aligned(16))) float tile[];
  dconv3_body<TM, TN, FLIP, BF, NR, BNX, NW, KS>(p, xcd_remap(blockIdx.x, gridDim.x),
                                                 blockIdx.y, gridDim.x, tile);
}

// Up to kDcGroup independent layers with the same tile shape in one launch (the lock-
// stepped HRNet branches of one depth level: the low-resolution ones alone leave most
// of the chip idle).  The 1-D grid is the concatenation of each layer's (tiles x N
// blocks); the XCD remap runs over the whole grid, then the block finds its layer.
constexpr int kDcGroup = 4;
struct DConvGroup {
  DConv p[kDcGroup];
  int start[kDcGroup + 1];
  int tiles[kDcGroup];
  int n;
};

template <int TM, int TN, bool FLIP, bool BF = false>
__global__ __launch_bounds__(256) void dconv3_group_kernel(DConvGroup gp) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int idx = xcd_remap(blockIdx.x, gridDim.x);
  int j = 0;
#pragma unroll
  for (int k = 1; k < kDcGroup; ++k) j += (k < gp.n && idx >= gp.start[k]) ? 1 : 0;
  const DConv p = j == 0 ? gp.p[0] : j == 1 ? gp.p[1] : j == 2 ? gp.p[2] : gp.p[3];
  const int t = j == 0 ? gp.tiles[0] : j == 1 ? gp.tiles[1] : j == 2 ? gp.tiles[2] : gp.tiles[3];
  const int st = j == 0 ? gp.start[0] : j == 1 ? gp.start[1] : j == 2 ? gp.start[2] : gp.start[3];
  const int local = idx - st;
  const int by = local / t;
  dconv3_body<TM, TN, FLIP, BF>(p, local - by * t, by, t, tile);
}

static bool dconv_legal(const vae2_act* ad, const vae2_act* yd, int k, int stride, int pad,
                        const float* a) {
  return k == 3 && stride == 1 && pad == 1 && ad->h == yd->h && ad->w == yd->w &&
         vec_ok(a, (int)ad->ps);
}

// remainder = true: an N of 16*TN + NR with (TN, NR) = (1, 2), (2, 4) or (4, 8) (the 18 /
// 36 / 72-channel branches) takes TN MFMA tiles plus NR VALU channels in one N block
// (fp32 operands only).
DTile pick_dtile(const vae2_act* ad, const vae2_act* yd, bool remainder) {
  DTile d;
  Tile t = pick_tile(act_pixels(yd), (int)yd->c);
  d.tn = t.tn;
  d.nblk = t.nblk;
  const int N = (int)yd->c, tn = N / 16, nr = N % 16;
  // (auto: all three where the single N block still fills the chip twice -- in the
  //  concurrent training step the 32 + 4 form is 0.4 % faster than the padded 48-column
  //  tiles; set_algo bit 128 restricts auto to 16 + 2; algo 2 takes all three wherever
  //  legal, for the tests)
  if (remainder && g_dconv_nr && !g_bf16 &&
      ((tn == 1 && nr == 2) ||
       ((g_conv_algo == 2 || g_dconv_nr_wide) && ((tn == 2 && nr == 4) || (tn == 4 && nr == 8))))) {
    d.tn = tn;
    d.nr = nr;
    d.nblk = 1;
  }
  const int Q = round_up((int)ad->c, 4) / 4;
  const int nsl = (Q + kDcMaxCs4 - 1) / kDcMaxCs4;
  d.cs4 = (Q + nsl - 1) / nsl;  // balanced slabs
  d.tiles_w = (int)ceil_div(yd->w, kDcBW);
  // 8-row tiles unless that leaves fewer than ~3 workgroups per CU
  d.tm = 4;
  // (from the all-MFMA N blocking, so the tile rows and the BN partial-statistics rows
  //  do not depend on the remainder switch or the grouped path)
  if (yd->h < 8 || ad->n * ceil_div(yd->h, 8) * d.tiles_w * t.nblk < 768) d.tm = 2;
  // tune key 2: the 8-row tiles as 8 waves of one row each (TM = 2, NW = 8) -- same tile
  // rows, so the same BN partial-statistics rows
  if (g_dconv_nw8 && d.tm == 4 && !g_bf16) {
    d.tm = 2;
    d.nw = 8;
  }
  d.tiles_h = (int)ceil_div(yd->h, d.nw * d.tm / 2);
  // the remainder form has one N block: only where the tiles alone fill the chip twice
  // (algo 2 forces it wherever legal, for the tests)
  if (d.nr && g_conv_algo != 2 && ad->n * d.tiles_h * d.tiles_w < 512) {
    d.tn = t.tn; d.nblk = t.nblk; d.nr = 0;
  }
  // tune key 13: a layer whose tiles leave fewer than 2 workgroups per CU (the 72-channel
  // branch at 32 x 64: 256 workgroups = one wave per SIMD) takes 16-channel N blocks --
  // more workgroups re-staging the same halo tile (L2-resident) for more waves per SIMD
  if (g_dconv_n16 && !g_bf16 && d.nr == 0 && d.tn > 1 && N > 16 &&
      ad->n * d.tiles_h * d.tiles_w * d.nblk < 512) {
    d.tn = 1;
    d.nblk = (N + 15) / 16;
  }
  // tune key 14: the 72-channel branch as two N blocks of 32 MFMA + 4 VALU channels
  // (block b: channels 36 b ..) -- the same workgroups as the two padded 48-column blocks
  // (24 of their 96 MFMA columns are padding), a third fewer MFMAs per block
  if (remainder && g_dconv_split72 && g_dconv_nr && !g_bf16 && d.nr == 0 && N == 72 &&
      d.nblk == 2 && d.tn == 3) {
    d.tn = 2;
    d.nr = 4;
  }
  // tune key 15: 4-row tiles (TM = 2) that leave at most 2 workgroups per CU run as 8-wave
  // workgroups splitting K in two -- the same tiles, rows and statistics rows, twice the
  // waves per SIMD (the 72-channel branch at 32 x 64: 256 workgroups, one wave per SIMD;
  // conv_bench 25.4 / 24.9 -> 25.0 / 24.6 us fwd / dgrad, step 902.1 / 900.7 -> 908.6 / 910.3
  // frames/s over 2 A/B pairs, scripts/gpu_r6_n.sh)
  if (g_dconv_ksp && !g_bf16 && d.nr == 0 && d.tm == 2 && d.nw == 4 && d.tn >= 2 &&
      ad->n * d.tiles_h * d.tiles_w * d.nblk < 512) {
    d.ks = g_dconv_ksp == 2 ? 4 : 2;
    d.nw = 4 * d.ks;
  }
  return d;
}

// The streaming kernel (dconv_stream.hip) takes the 18 -> 18 and 36 -> 36 direct convs
// (fp32 operands, the VALU-remainder form) wherever the direct kernel is legal: its
// partial-statistics rows are its workgroups, so dconv_rows asks the same predicate.
bool stream_use(const vae2_act* ad, const vae2_act* yd) {
  return g_dconv_stream && !g_bf16 && g_dconv_nr && g_conv_algo != 1 &&
         (g_conv_algo == 2 || ad->w >= 16) && dconv3s_shape(ad, yd);
}

bool dconv_use(const vae2_act* ad, const vae2_act* yd, int k, int stride, int pad,
               const float* a) {
  if (g_conv_algo == 1 || !dconv_legal(ad, yd, k, stride, pad, a)) return false;
  if (g_conv_algo == 2 || stream_use(ad, yd)) return true;
  // auto: enough workgroups to fill the chip (narrow images waste partial 32-column
  // tiles and low-resolution layers have too few tiles: the gather kernel wins there)
  DTile d = pick_dtile(ad, yd, false);
  return ad->w >= 16 && ad->n * d.tiles_h * d.tiles_w * d.nblk >= 256;
}

template <int TM, bool FLIP, int NW = 4>
static void dconv_launch_tn(const DConv& p, int tn, dim3 grid, size_t shm, hipStream_t s,
                            int nr = 0) {
  if (p.isave || p.bx) {  // fused BatchNorm (fp32 operands): forward input / dgrad partials
    constexpr int X = FLIP ? 2 : 1;
    if (nr) {
      if (tn == 1 && nr == 2) VAE2_LAUNCH((dconv3_kernel<TM, 1, FLIP, false, 2, X, NW>), grid, dim3(64 * NW), shm, s, p);
      else if (tn == 2 && nr == 4) VAE2_LAUNCH((dconv3_kernel<TM, 2, FLIP, false, 4, X, NW>), grid, dim3(64 * NW), shm, s, p);
      else VAE2_LAUNCH((dconv3_kernel<TM, 4, FLIP, false, 8, X, NW>), grid, dim3(64 * NW), shm, s, p);
      return;
    }
    switch (tn) {
#define CASE(T) \
  case T: VAE2_LAUNCH((dconv3_kernel<TM, T, FLIP, false, 0, X, NW>), grid, dim3(64 * NW), shm, s, p); break;
      CASE(1) CASE(2) CASE(3) CASE(4)
#undef CASE
    }
    return;
  }
  if (nr) {  // fp32 operands (pick_dtile)
    if (tn == 1 && nr == 2) VAE2_LAUNCH((dconv3_kernel<TM, 1, FLIP, false, 2, 0, NW>), grid, dim3(64 * NW), shm, s, p);
    else if (tn == 2 && nr == 4) VAE2_LAUNCH((dconv3_kernel<TM, 2, FLIP, false, 4, 0, NW>), grid, dim3(64 * NW), shm, s, p);
    else VAE2_LAUNCH((dconv3_kernel<TM, 4, FLIP, false, 8, 0, NW>), grid, dim3(64 * NW), shm, s, p);
    return;
  }
  switch (tn) {
#define CASE(T) \
  case T:                                                                         \
    if (g_bf16) VAE2_LAUNCH((dconv3_kernel<TM, T, FLIP, true, 0, 0, NW>), grid, dim3(64 * NW), shm, s, p); \
    else VAE2_LAUNCH((dconv3_kernel<TM, T, FLIP, false, 0, 0, NW>), grid, dim3(64 * NW), shm, s, p);        \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4)
#undef CASE
  }
}

// K-split form (pick_dtile, set_tune key 15): TM = 2, 4 KS waves, fp32 operands, no remainder
template <bool FLIP, int KS>
static void dconv_launch_ksp(const DConv& p, int tn, dim3 grid, size_t shm, hipStream_t s) {
  constexpr int X = FLIP ? 2 : 1, NW = 4 * KS;
  const bool bn = p.isave || p.bx;
  switch (tn) {
#define CASE(T)                                                                                        \
  case T:                                                                                              \
    if (bn) VAE2_LAUNCH((dconv3_kernel<2, T, FLIP, false, 0, X, NW, KS>), grid, dim3(64 * NW), shm, s, p); \
    else VAE2_LAUNCH((dconv3_kernel<2, T, FLIP, false, 0, 0, NW, KS>), grid, dim3(64 * NW), shm, s, p);    \
    break;
    CASE(2) CASE(3) CASE(4)
#undef CASE
  }
}


static DConv make_dconv(const DTile& d, const float* a, const vae2_act* ad, const float* wp,
                        uint32_t w_bytes, const float* bias, float* y, const vae2_act* yd,
                        float beta, float* stats) {
  DConv p{};
  p.a = a; p.a_ps = (int)ad->ps; p.a_c = (int)ad->c; p.a_c4 = round_up((int)ad->c, 4);
  p.img_h = (int)ad->h; p.img_w = (int)ad->w;
  p.tiles_h = d.tiles_h; p.tiles_w = d.tiles_w; p.cs4 = d.cs4;
  p.w = wp; p.a_bytes = act_bytes(ad); p.w_bytes = w_bytes;
  p.n = (int)yd->c; p.bias = bias; p.y = y; p.y_ps = (int)yd->ps; p.beta = beta;
  p.stats = stats;
  p.vec_out = g_vec_out && vec_ok(y, (int)yd->ps) && !(stats && beta != 0.f);
  return p;
}

static size_t dconv_shm(const DTile& d) {
  const int rows = (d.ks > 1 ? 4 : d.nw) * d.tm / 2;  // output rows of a tile (KS: 4 row waves)
  const size_t stage = ((size_t)(rows + 2) * (kDcBW + 2) * (d.cs4 * 4 + 4) +
                        (size_t)d.nr * ((9 * d.cs4 + 7) / 8) * 32 + 2 * kDcTab) * sizeof(float);
  // KS > 1: shares 1 .. KS-1's accumulators ([KS - 1][4 waves][TM][TN][64] f4) in the same
  // LDS after the K loop
  const size_t kred = (size_t)(d.ks - 1) * 4 * d.tm * d.tn * 64 * 16;
  return stage > kred ? stage : kred;
}

template <int TM, bool FLIP>
static void dconv_group_launch_tn(const DConvGroup& g, int tn, dim3 grid, size_t shm,
                                  hipStream_t s) {
  switch (tn) {
#define CASE(T)                                                                          \
  case T:                                                                                \
    if (g_bf16) VAE2_LAUNCH((dconv3_group_kernel<TM, T, FLIP, true>), grid, dim3(256), shm, s, g); \
    else VAE2_LAUNCH((dconv3_group_kernel<TM, T, FLIP>), grid, dim3(256), shm, s, g);    \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4)
#undef CASE
  }
}

int launch_dconv(const float* a, const vae2_act* ad, const float* wp, uint32_t w_bytes,
                 const float* bias, float* y, const vae2_act* yd, float beta,
                 float* stats, bool flip, hipStream_t s, const char* fn, const BnSide& bn) {
  if (stream_use(ad, yd)) {
    dconv3s_launch(a, ad, wp, w_bytes, bias, y, yd, beta, stats, flip, bn.isave, bn.irelu,
                   bn.bx, bn.bx_ps, bn.brelu, bn.bsave, bn.bx_bytes, act_bytes(ad), s);
    return check_launch(fn);
  }
  DTile d = pick_dtile(ad, yd);
  DConv p = make_dconv(d, a, ad, wp, w_bytes, bias, y, yd, beta, stats);
  p.isave = bn.isave; p.irelu = bn.irelu;
  p.bx = bn.bx; p.bx_ps = bn.bx_ps; p.brelu = bn.brelu; p.bsave = bn.bsave;
  p.bx_bytes = bn.bx_bytes;
  dim3 grid((unsigned)(ad->n * d.tiles_h * d.tiles_w), (unsigned)d.nblk);
  const size_t shm = dconv_shm(d);
  if (d.ks == 4) {
    if (flip) dconv_launch_ksp<true, 4>(p, d.tn, grid, shm, s);
    else dconv_launch_ksp<false, 4>(p, d.tn, grid, shm, s);
  } else if (d.ks == 2) {
    if (flip) dconv_launch_ksp<true, 2>(p, d.tn, grid, shm, s);
    else dconv_launch_ksp<false, 2>(p, d.tn, grid, shm, s);
  } else if (d.nw == 8) {
    if (flip) dconv_launch_tn<2, true, 8>(p, d.tn, grid, shm, s, d.nr);
    else dconv_launch_tn<2, false, 8>(p, d.tn, grid, shm, s, d.nr);
  } else if (d.tm == 4) {
    if (flip) dconv_launch_tn<4, true>(p, d.tn, grid, shm, s, d.nr);
    else dconv_launch_tn<4, false>(p, d.tn, grid, shm, s, d.nr);
  } else {
    if (flip) dconv_launch_tn<2, true>(p, d.tn, grid, shm, s, d.nr);
    else dconv_launch_tn<2, false>(p, d.tn, grid, shm, s, d.nr);
  }
  return check_launch(fn);
}


int64_t dconv_rows(const vae2_act* ad, const vae2_act* yd) {
  if (stream_use(ad, yd)) return dconv3s_rows(ad, yd);
  DTile d = pick_dtile(ad, yd);
  return ad->n * d.tiles_h * d.tiles_w;
}

}  // namespace vae2

using namespace vae2;

extern "C" {

// Independent convolutions in one call (one HRNet depth level): the jobs the direct 3x3
// kernel takes are launched together, up to kDcGroup per launch, grouped by tile shape
// and direction (jobs writing the same output never share a launch); the others go
// through vae2_conv2d_fwd / vae2_conv2d_bwd_data one by one.
static int g_conv_group = 0;  // measured slower in the full step: off by default

int vae2_conv2d_set_grouping(int on) {
  const int prev = g_conv_group;
  g_conv_group = on ? 1 : 0;
  return prev;
}

int vae2_conv2d_multi(int n, const vae2_conv_job* jobs, void* stream) {
  const char* fn = "vae2_conv2d_multi";
  VAE2_REQUIRE(n >= 0 && (n == 0 || jobs), fn, "bad arguments");
  hipStream_t s = as_stream(stream);
  struct Bucket {
    int tm, tn, flip, cnt, tot;
    DConvGroup g;
    size_t shm;
    const float* outs[kDcGroup];
  };
  Bucket b[8];
  int nb = 0;
  auto flush = [&](Bucket& k) -> int {
    if (k.cnt == 0) return 0;
    k.g.n = k.cnt;
    k.g.start[k.cnt] = k.tot;
    for (int q = k.cnt; q < kDcGroup; ++q) { k.g.start[q + 1] = k.tot; k.g.tiles[q] = 1; }
    const dim3 grid((unsigned)k.tot);
    if (k.tm == 4) {
      if (k.flip) dconv_group_launch_tn<4, true>(k.g, k.tn, grid, k.shm, s);
      else dconv_group_launch_tn<4, false>(k.g, k.tn, grid, k.shm, s);
    } else {
      if (k.flip) dconv_group_launch_tn<2, true>(k.g, k.tn, grid, k.shm, s);
      else dconv_group_launch_tn<2, false>(k.g, k.tn, grid, k.shm, s);
    }
    k.cnt = 0; k.tot = 0; k.shm = 0;
    return check_launch(fn);
  };
  // a job writing an output some queued job also writes runs after that job's launch
  auto flush_holding = [&](const float* out) -> int {
    for (int k = 0; k < nb; ++k)
      for (int q = 0; q < b[k].cnt; ++q)
        if (b[k].outs[q] == out) return flush(b[k]);
    return 0;
  };
  for (int i = 0; i < n; ++i) {
    const vae2_conv_job& J = jobs[i];
    VAE2_REQUIRE(J.kind == 0 || J.kind == 1, fn, "job kind must be 0 (forward) or 1 (data grad)");
    if (int rc = flush_holding(J.y)) return rc;
    const bool fwd = J.kind == 0;
    const vae2_act* ad = &J.xd;  // the kernel's input: x (forward) or dy (data gradient)
    const vae2_act* od = &J.yd;
    bool direct = g_conv_group && J.x && J.wp && J.y &&
                  (fwd ? conv_shapes_ok(ad, od, J.k, J.stride, J.pad)
                       : conv_shapes_ok(od, ad, J.k, J.stride, J.pad)) &&
                  fits32(ad) && fits32(od) && dconv_use(ad, od, J.k, J.stride, J.pad, J.x) &&
                  !stream_use(ad, od) &&         // (streaming layers: their own launch)
                  pick_dtile(ad, od).nr == 0 &&  // (remainder layers: their own launch)
                  pick_dtile(ad, od).nw == 4;    // (8-wave tiles: their own launch)
    if (!direct) {
      int rc = fwd ? vae2_conv2d_fwd(J.x, ad, J.wp, J.bias, J.y, od, J.k, J.stride, J.pad,
                                     J.beta, J.stats, stream)
                   : vae2_conv2d_bwd_data(J.x, ad, J.wp, J.y, od, J.k, J.stride, J.pad,
                                          J.beta, stream);
      if (rc) return rc;
      continue;
    }
    const DTile d = pick_dtile(ad, od, false);
    const uint32_t wb = fwd ? packed_bytes(od->c, ad->c, J.k, 0) : packed_bytes(ad->c, od->c, J.k, 1);
    int k = 0;
    while (k < nb && !(b[k].tm == d.tm && b[k].tn == d.tn && b[k].flip == (fwd ? 0 : 1))) ++k;
    if (k == nb) {
      VAE2_REQUIRE(nb < 8, fn, "too many tile shapes");
      b[nb] = Bucket{};
      b[nb].tm = d.tm; b[nb].tn = d.tn; b[nb].flip = fwd ? 0 : 1;
      ++nb;
    }
    Bucket& B = b[k];
    if (B.cnt == kDcGroup) {
      int rc = flush(B);
      if (rc) return rc;
    }
    const int tiles = (int)(ad->n * d.tiles_h * d.tiles_w);
    B.g.p[B.cnt] = make_dconv(d, J.x, ad, J.wp, wb, fwd ? J.bias : nullptr, J.y, od, J.beta,
                              fwd ? J.stats : nullptr);
    B.g.start[B.cnt] = B.tot;
    B.g.tiles[B.cnt] = tiles;
    B.outs[B.cnt] = J.y;
    B.tot += tiles * d.nblk;
    const size_t sh = dconv_shm(d);
    if (sh > B.shm) B.shm = sh;
    ++B.cnt;
  }
  for (int k = 0; k < nb; ++k) {
    int rc = flush(b[k]);
    if (rc) return rc;
  }
  return 0;
}


}  // extern "C"

// Convolutions of the HRNet stacks as implicit GEMMs on the fp32 matrix cores
// (v_mfma_f32_16x16x4_f32: exact fp32 FMA chains, 64 FLOP/clk/SIMD on gfx950).
//
//   forward     Y[m][n] = sum_k A[m][k] * B[k][n]
//               m = output pixel, n = Cout, k = (tap, Cin4); A = im2col(X) gathered
//               from NHWC on the fly, B = weights packed [Npad][k*k][Cin4].
//   bwd data    same kernel: m = input pixel of one stride-parity class per launch,
//               n = Cin, k = (valid tap, Cout4), A = dY gathered, B = weights packed
//               [Cin_pad][k*k][Cout4] (the transposed conv).
//   bwd weight  dW[co][(tap, ci)] = sum_p dY[p][co] * X[src(p, tap)][ci], split over
//               pixels into fp32 slabs (one per wave), then a fixed-order reduction
//               into the [Cout][Cin][kh][kw] gradient (deterministic).
//
// Fragment-direct loads: Cin is padded to a multiple of 4 (Cin4) inside K, and in
// each 16-deep K chunk lane group g = lane>>4 owns the 4 consecutive k = 4g..4g+3,
// i.e. 4 consecutive channels of ONE tap.  MFMA k-step s uses k = 4g+s for both
// operands (a permutation of the reduction order the sum does not see).  So a
// lane's A fragment for 4 k-steps is one 16-byte load of an NHWC pixel and its B
// fragment one 16-byte load of the packed weights: no LDS staging, no barriers in
// the main loop; fragments are double-buffered in registers.
//
// Replaces nn.Conv2d forward/backward for every conv of enc_hrnet.py (call sites
// in include/vae2_hip.h).
#include "conv.h"

namespace vae2 {

// ------------------------------------------------------------ weight pack ----
// mode 0: out[n][t][c4] = w[n][c][t]         n < round_up(cout,64), c4 < round_up(cin,4)
// mode 1: out[n][t][c4] = w[c][n][t]         n < round_up(cin,64),  c4 < round_up(cout,4)
// (rows padded to 64 = the widest N tile, so B loads never need a bounds check).
// w[co][ci][t] lives at w[co*ld + ci*kk + t]: ld = cin*kk for a whole weight, larger
// for an input-channel block of a wider one (the per-branch blocks of a head conv).
__global__ void pack_weight_kernel(const float* __restrict__ w, int cout, int cin, int kk,
                                   int mode, int ld, float* __restrict__ out) {
  const int rows = mode == 0 ? (cout + 63) / 64 * 64 : (cin + 63) / 64 * 64;
  const int cols4 = mode == 0 ? (cin + 3) / 4 * 4 : (cout + 3) / 4 * 4;
  const int total = rows * kk * cols4;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    int n = i / (kk * cols4);
    int rem = i - n * kk * cols4;
    int t = rem / cols4;
    int c = rem - t * cols4;
    float v = 0.f;
    if (mode == 0) {
      if (n < cout && c < cin) v = w[(int64_t)n * ld + c * kk + t];
    } else {
      if (n < cin && c < cout) v = w[(int64_t)c * ld + n * kk + t];
    }
    out[i] = v;
  }
}

// One block row (blockIdx.y) per packing job.
__global__ __launch_bounds__(256) void pack_weights_batched_kernel(const vae2_pack_job* jobs) {
  const vae2_pack_job j = jobs[blockIdx.y];
  const int kk = j.k * j.k;
  const int rows = j.mode == 0 ? (j.cout + 63) / 64 * 64 : (j.cin + 63) / 64 * 64;
  const int cols4 = j.mode == 0 ? (j.cin + 3) / 4 * 4 : (j.cout + 3) / 4 * 4;
  const int per_row = kk * cols4;
  const int total = rows * per_row;
  const int64_t ld = j.ld > 0 ? j.ld : (int64_t)j.cin * kk;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int n = i / per_row;
    const int rem = i - n * per_row;
    const int t = rem / cols4;
    const int c = rem - t * cols4;
    float v = 0.f;
    if (j.mode == 0) {
      if (n < j.cout && c < j.cin) v = j.w[(int64_t)n * ld + c * kk + t];
    } else {
      if (n < j.cin && c < j.cout) v = j.w[(int64_t)c * ld + n * kk + t];
    }
    j.out[i] = v;
  }
}


int g_wide_tiles = 1;
int g_ksplit = 1;    // vae2_conv2d_set_algo bit 8 disables the K split (A/B tests)
int g_bf16 = 0;      // vae2_conv2d_set_mfma_bf16: bf16 MFMA operands (fp32 accumulate)
int g_conv_algo = 0; // 0 auto, 1 gather kernel only, 2 direct wherever legal
int g_dconv_nr = 1;  // vae2_conv2d_set_algo: bit 16 clear enables the VALU remainder
int g_gemm1 = 1;     // vae2_conv2d_set_algo: bit 32 clear enables the persistent 1x1 GEMM
int g_vec_out = 1;   // vae2_conv2d_set_algo: bit 64 clear enables the quad-transposed stores
int g_dconv_nr_wide = 1;  // vae2_conv2d_set_algo: bit 128 clear enables the 32 + 4 / 64 + 8 forms
// The launch-shape knobs of vae2_conv2d_set_tune that this library's conv units read
// (documented in the table below; the other files' knobs are defined where they are read).
int g_igemm_minblk = 512, g_wgrad_cols = 1, g_dconv_nw8 = 0, g_wgrad_nw8 = 1, g_gemm1_tn = 4,
    g_gemm1_tm = 2, g_igemm_nr = 2, g_wgrad_narrow = 3, g_igemm_tab = 1, g_dconv_n16 = 0,
    g_dconv_split72 = 0, g_dconv_ksp = 1, g_wgrad_wgs = 1024;

// vae2_conv2d_set_tune: row index = key.  A value in lo..hi is stored; one outside stores
// `other`, or with other == kReject is refused (-1, setting unchanged).  A/B measurement
// switches: every setting computes the same result.
constexpr int kReject = INT32_MIN, kAny = INT32_MAX;
struct Knob {
  int* var;
  int lo, hi, other;
};
static const Knob kKnobs[] = {
    // 0 (512): the gather GEMM's row tiles shrink until the grid has this many workgroups,
    //    0 = the plain row-tile rule (512: step 909.3-910.7 -> 915.4-915.8 frames/s, 768 level)
    {&g_igemm_minblk, 0, kAny, 0},
    // 1 (on): gather weight gradient takes 64 columns as one 2-row-tile block (pick_wtile)
    {&g_wgrad_cols, 0, 1, 1},
    // 2 (off): direct 3x3 8-row tiles as 8 waves of one row each
    {&g_dconv_nw8, 0, 1, 1},
    // 3 (on): 3x3 weight gradients of the remainder layers over 8 waves
    //    (keys 1 / 3 on: 820.7 / 822.4 -> 824.2 / 823.1, 828.3 / 828.3 frames/s; key 2 825.1 / 823.8)
    {&g_wgrad_nw8, 0, 1, 1},
    // 4 (4): the 1x1 GEMM's N tiles per workgroup, 3..8 (TN = 8 holds 264 VGPRs, one wave per
    //    SIMD: step 845.1 / 845.4 vs 847.3 / 848.0 frames/s at 4)
    {&g_gemm1_tn, 3, 8, kReject},
    // 5 (2): the 1x1 GEMM's row tiles of 16 * TM pixels, TM = 1 or 2
    {&g_gemm1_tm, 1, 2, 2},
    // 6 (2): gather GEMM VALU remainder: 0 off, 1 for N = 18 and 36, 2 for N = 18 only
    //    (step 895.7 -> 899.8 frames/s)
    {&g_igemm_nr, 0, 2, kReject},
    // 7 (3): wgrad_narrow.hip for 18 / 36 / 72 channels: 0 off, 1 on, 2 with register
    //    prefetch, 3 with 8 waves (35.0 / 31.7 / 32.1 -> 33.0 / 31.4 / 31.2 us)
    {&g_wgrad_narrow, 0, 3, kReject},
    // 8 (on): bn.hip, buffer-resource BatchNorm bodies
    {&g_bn_v2, 0, 1, 1},
    // 9 (3): dconv_stream.hip, streaming direct 3x3: bit 0 for 18, bit 1 for 36 channels
    {&g_dconv_stream, 0, 3, 3},
    // 10 (0): dconv_stream.hip, target workgroups per CU, 0 = auto
    {&g_dconv_stream_wpc, 0, 8, 0},
    // 11 (off): dconv_stream.hip, 18-channel weights in LDS instead of global
    {&g_dconv_stream_bl, 0, 1, 1},
    // 12 (on): the gather GEMM's K-step table (0: per-chunk tap arithmetic)
    {&g_igemm_tab, 0, 1, 1},
    // 13 (off): direct 3x3 16-channel N blocks for layers short of workgroups
    {&g_dconv_n16, 0, 1, 1},
    // 14 (off): the 72-channel direct 3x3 as two 32 + 4 N blocks
    {&g_dconv_split72, 0, 1, 1},
    // 15 (1): direct 3x3 K split for layers short of workgroups: 0 off, 1 = 2 shares /
    //    8 waves, 2 = 4 shares / 16 waves
    {&g_dconv_ksp, 0, 2, kReject},
    // 16 (2): wgrad_narrow.hip, minimum tiles per split (partial slab), 1 or 2
    {&g_wgrad_narrow_tps, 1, 2, kReject},
    // 17 (1): dconv_stream.hip, minimum 4-row steps per band, 1 or 2
    {&g_dconv_stream_spb, 1, 2, kReject},
    // 18 (1024): gather weight gradient's target workgroups (split count), 256..8192
    {&g_wgrad_wgs, 256, 8192, kReject},
    // 19 (1024): bn.hip, BatchNorm blocks per layer at most, 256..8192
    {&g_bn_blocks, 256, 8192, kReject},
    // 20 (0): bn.hip, the apply kernels' resident-block budget, 0 = one block per chunk
    {&g_bn_apply_res, 0, 65536, kReject},
    // 21 (on): resample.hip, the fuse sum a channel quad per thread (0: per channel)
    {&g_fuse_quad, 0, 1, 1},
};

}  // namespace vae2

using namespace vae2;

extern "C" {

int64_t vae2_conv2d_packed_size(int64_t cout, int64_t cin, int k, int mode) {
  int rows = mode == 0 ? round_up((int)cout, 64) : round_up((int)cin, 64);
  int cols4 = mode == 0 ? round_up((int)cin, 4) : round_up((int)cout, 4);
  return (int64_t)rows * k * k * cols4;
}

int vae2_conv2d_pack_weight_ld(const float* w, int64_t cout, int64_t cin, int k, int mode,
                               int64_t ld, float* out, void* stream) {
  const char* fn = "vae2_conv2d_pack_weight";
  VAE2_REQUIRE(w && out && cout > 0 && cin > 0 && k > 0 && (mode == 0 || mode == 1), fn,
               "bad arguments");
  VAE2_REQUIRE(ld >= cin * k * k && ld < (int64_t(1) << 31), fn, "bad row stride");
  int64_t total = vae2_conv2d_packed_size(cout, cin, k, mode);
  VAE2_LAUNCH(pack_weight_kernel, dim3(ew_blocks(total, 256, 2048)), dim3(256), 0,
                     as_stream(stream), w, (int)cout, (int)cin, k * k, mode, (int)ld, out);
  return check_launch(fn);
}

int vae2_conv2d_pack_weight(const float* w, int64_t cout, int64_t cin, int k, int mode,
                            float* out, void* stream) {
  return vae2_conv2d_pack_weight_ld(w, cout, cin, k, mode, cin * k * k, out, stream);
}

int vae2_conv2d_pack_weights(const vae2_pack_job* jobs, int64_t njobs, void* stream) {
  const char* fn = "vae2_conv2d_pack_weights";
  VAE2_REQUIRE(jobs && njobs > 0 && njobs <= 65535, fn, "bad job table");
  VAE2_LAUNCH(pack_weights_batched_kernel, dim3(32, (unsigned)njobs), dim3(256), 0,
                     as_stream(stream), jobs);
  return check_launch(fn);
}

// Returns the previous value, or -1 for an unknown key or a refused value (kKnobs).
int vae2_conv2d_set_tune(int key, int value) {
  if (key < 0 || key >= (int)(sizeof(kKnobs) / sizeof(kKnobs[0]))) return -1;
  const Knob& k = kKnobs[key];
  if (value < k.lo || value > k.hi) {
    if (k.other == kReject) return -1;
    value = k.other;
  }
  const int prev = *k.var;
  *k.var = value;
  return prev;
}

int vae2_conv2d_set_mfma_bf16(int on) {
  const int prev = g_bf16;
  g_bf16 = on ? 1 : 0;
  return prev;
}


int vae2_conv2d_set_algo(int algo) {
  const int prev = g_conv_algo + (g_wide_tiles ? 0 : 4) + (g_ksplit ? 0 : 8) +
                   (g_dconv_nr ? 0 : 16) + (g_gemm1 ? 0 : 32) + (g_vec_out ? 0 : 64) +
                   (g_dconv_nr_wide ? 0 : 128);
  const int a = algo & 7;
  if (algo >= 0 && algo <= 255 && a <= 6 && a != 3) {
    g_dconv_nr_wide = (algo & 128) ? 0 : 1;
    g_conv_algo = a & 3;
    g_wide_tiles = a < 4;
    g_ksplit = !(algo & 8);
    g_dconv_nr = !(algo & 16);
    g_gemm1 = !(algo & 32);
    g_vec_out = !(algo & 64);
  }
  return prev;
}

// The gather kernel's forward setup (vae2_conv2d_fwd, its rows and kernel-name queries).
static void igemm_fwd_setup(IGemm& p, const float* x, const vae2_act* xd, const float* wp,
                            const float* bias, float* y, const vae2_act* yd, int k, int stride,
                            int pad, float beta, float* stats) {
  p.a = x; p.a_ps = (int)xd->ps; p.a_c = (int)xd->c; p.a_c4 = round_up((int)xd->c, 4);
  p.a_h = (int)xd->h; p.a_w = (int)xd->w;
  p.g_n = (int)yd->n; p.g_h = (int)yd->h; p.g_w = (int)yd->w;
  p.a_step = stride;
  p.nth = k; p.ntw = k;
  p.dh0 = -pad; p.dhs = 1; p.dw0 = -pad; p.dws = 1;
  p.kh0 = 0; p.khs = 1; p.kw0 = 0; p.kws = 1; p.ksz = k;
  p.w = wp; p.n = (int)yd->c;
  p.a_bytes = act_bytes(xd);
  p.w_bytes = packed_bytes(yd->c, xd->c, k, 0);
  p.bias = bias;
  p.y = y; p.y_ps = (int)yd->ps; p.y_h = (int)yd->h; p.y_w = (int)yd->w;
  p.y_step = 1; p.y_offh = 0; p.y_offw = 0;
  p.beta = beta;
  p.stats = stats;
}

int64_t vae2_conv2d_fwd_stats_rows(const float* x, const vae2_act* xd, const vae2_act* yd,
                                   int k, int stride, int pad) {
  if (!act_ok(xd) || !act_ok(yd)) return 0;
  if (dconv_use(xd, yd, k, stride, pad, x)) return dconv_rows(xd, yd);
  G1Tile g1;
  if (gemm1_pick(xd, yd, k, stride, pad, x, &g1)) return g1.grid_x;
  IGemm p{};
  igemm_fwd_setup(p, x, xd, nullptr, nullptr, nullptr, yd, k, stride, pad, 0.f, nullptr);
  return igemm_plan(p, 1).grid.x;
}

int vae2_conv2d_fwd_kernel_name(const vae2_act* xd, const vae2_act* yd, int k, int stride,
                                int pad, char* buf, int64_t len) {
  if (!xd || !yd || !buf || len <= 0) return -22;
  if (dconv_use(xd, yd, k, stride, pad, (const float*)16)) {
    if (stream_use(xd, yd)) {
      const int q = (int)((xd->c + 3) / 4);
      snprintf(buf, (size_t)len, "dconv3s_kernel<%d, %d, %d, false", q == 5 ? 1 : 2,
               q == 5 ? 2 : 4, q);
      return 0;
    }
    DTile d = pick_dtile(xd, yd);
    if (d.nr)
      snprintf(buf, (size_t)len, "dconv3_kernel<%d, %d, false, false, %d>", d.tm, d.tn, d.nr);
    else
      snprintf(buf, (size_t)len, "dconv3_kernel<%d, %d, false>", d.tm, d.tn);
    return 0;
  }
  G1Tile g1;
  if (gemm1_pick(xd, yd, k, stride, pad, (const float*)16, &g1)) {
    snprintf(buf, (size_t)len, "gemm1x1_kernel<%d, %d>", g1.tm, g1.tn);
    return 0;
  }
  IGemm p{};
  igemm_fwd_setup(p, nullptr, xd, nullptr, nullptr, nullptr, yd, k, stride, pad, 0.f, nullptr);
  const Tile t = igemm_plan(p, 1).t;
  if (t.ks > 1)
    snprintf(buf, (size_t)len, "igemm_kernel<%d, %d, true, 0, %d>", t.tm, t.tn, t.ks);
  else
    snprintf(buf, (size_t)len, "igemm_kernel<%d, %d, true, 0>", t.tm, t.tn);
  return 0;
}

int vae2_conv2d_fwd(const float* x, const vae2_act* xd, const float* wp,
                    const float* bias, float* y, const vae2_act* yd, int k,
                    int stride, int pad, float beta, float* stats,
                    void* stream) {
  const char* fn = "vae2_conv2d_fwd";
  VAE2_REQUIRE(x && wp && y, fn, "null pointer");
  VAE2_REQUIRE(conv_shapes_ok(xd, yd, k, stride, pad), fn, "inconsistent conv shapes");
  VAE2_REQUIRE(fits32(xd) && fits32(yd), fn, "tensor too large for 32-bit indexing");
  if (dconv_use(xd, yd, k, stride, pad, x))
    return launch_dconv(x, xd, wp, packed_bytes(yd->c, xd->c, k, 0), bias, y, yd, beta, stats,
                        false, as_stream(stream), fn);
  G1Tile g1;
  if (gemm1_pick(xd, yd, k, stride, pad, x, &g1)) {
    const int rc = launch_gemm1(x, xd, wp, packed_bytes(yd->c, xd->c, k, 0), bias, y, yd, beta,
                                stats, g1, as_stream(stream), fn);
    if (rc != -1) return rc;
    VAE2_REQUIRE(stats == nullptr, fn, "BN statistics need a 16-byte aligned output here");
  }
  IGemm p{};
  igemm_fwd_setup(p, x, xd, wp, bias, y, yd, k, stride, pad, beta, stats);
  return launch_igemm(p, 0, as_stream(stream), fn);
}

int vae2_conv2d_bnin_ok(const float* x, const vae2_act* xd, const vae2_act* yd, int k,
                        int stride, int pad) {
  if (!x || !conv_shapes_ok(xd, yd, k, stride, pad) || !fits32(xd) || !fits32(yd)) return 0;
  return !g_bf16 && dconv_use(xd, yd, k, stride, pad, x) && g_conv_algo != 1 &&
         wgrad3_shape_ok(xd, yd, k, stride, pad) && vec_ok(x, (int)xd->ps);
}

int vae2_conv2d_fwd_bnin(const float* x, const vae2_act* xd, const float* bn_save, int relu,
                         const float* wp, const float* bias, float* y, const vae2_act* yd,
                         int k, int stride, int pad, float beta, float* stats, void* stream) {
  const char* fn = "vae2_conv2d_fwd_bnin";
  VAE2_REQUIRE(x && wp && y && bn_save, fn, "null pointer");
  VAE2_REQUIRE(conv_shapes_ok(xd, yd, k, stride, pad), fn, "inconsistent conv shapes");
  VAE2_REQUIRE(vae2_conv2d_bnin_ok(x, xd, yd, k, stride, pad), fn,
               "input BatchNorm needs the direct 3x3 kernels (vae2_conv2d_bnin_ok)");
  BnSide bn;
  bn.isave = bn_save;
  bn.irelu = relu ? 1 : 0;
  return launch_dconv(x, xd, wp, packed_bytes(yd->c, xd->c, k, 0), bias, y, yd, beta, stats,
                      false, as_stream(stream), fn, bn);
}

// The gather kernel's data-gradient setup (vae2_conv2d_bwd_data, the _bnpart form and its
// rows query): returns the number of stride-parity classes (0: nothing to do, -1: stride > 2).
static int igemm_dgrad_setup(IGemm& p, const float* dy, const vae2_act* dyd, const float* wp,
                             float* dx, const vae2_act* dxd, int k, int stride, int pad,
                             float beta) {
  // Stride-parity classes (ph, pw) of the input pixels: input row ih = stride*i + ph
  // receives from output row oh = (ih + pad - kh)/stride for every kh with
  // (ph + pad - kh) % stride == 0.  All classes run in one launch (class = blockIdx.z);
  // each has only its valid taps.
  p.a = dy; p.a_ps = (int)dyd->ps; p.a_c = (int)dyd->c; p.a_c4 = round_up((int)dyd->c, 4);
  p.a_h = (int)dyd->h; p.a_w = (int)dyd->w;
  p.g_n = (int)dxd->n;
  p.a_step = 1;
  p.dhs = -1; p.dws = -1;
  p.khs = stride; p.kws = stride; p.ksz = k;
  p.w = wp; p.n = (int)dxd->c;
  p.a_bytes = act_bytes(dyd);
  p.w_bytes = packed_bytes(dyd->c, dxd->c, k, 1);
  p.bias = nullptr;
  p.y = dx; p.y_ps = (int)dxd->ps; p.y_h = (int)dxd->h; p.y_w = (int)dxd->w;
  p.y_step = stride;
  p.beta = beta;
  p.stats = nullptr;
  int ncls = 0;
  for (int ph = 0; ph < stride; ++ph) {
    for (int pw = 0; pw < stride; ++pw) {
      int gh = (int)((dxd->h - ph + stride - 1) / stride);
      int gw = (int)((dxd->w - pw + stride - 1) / stride);
      if (gh <= 0 || gw <= 0) continue;
      if (ncls >= 4) return -1;
      int kh0 = ((ph + pad) % stride + stride) % stride;
      int kw0 = ((pw + pad) % stride + stride) % stride;
      int nth = kh0 < k ? (k - 1 - kh0) / stride + 1 : 0;
      int ntw = kw0 < k ? (k - 1 - kw0) / stride + 1 : 0;
      IGemm::Cls& c = p.cls[ncls++];
      c.g_h = gh; c.g_w = gw;
      c.nth = nth; c.ntw = ntw;
      c.dh0 = (ph + pad - kh0) / stride;
      c.dw0 = (pw + pad - kw0) / stride;
      c.kh0 = kh0; c.kw0 = kw0;
      c.y_offh = ph; c.y_offw = pw;
      if (nth == 0 || ntw == 0) { c.nth = 0; c.ntw = 1; }
    }
  }
  if (ncls == 0) return 0;
  {
    const IGemm::Cls& c = p.cls[0];  // the single-class launch reads the plain fields
    p.g_h = c.g_h; p.g_w = c.g_w; p.nth = c.nth; p.ntw = c.ntw;
    p.dh0 = c.dh0; p.dw0 = c.dw0; p.kh0 = c.kh0; p.kw0 = c.kw0;
    p.y_offh = c.y_offh; p.y_offw = c.y_offw;
  }
  return ncls;
}

// Partial-statistics rows of a gather-kernel data gradient (gridDim.x * classes).
static int64_t igemm_dgrad_rows(const float* dy, const vae2_act* dyd, const vae2_act* dxd,
                                int k, int stride, int pad) {
  IGemm p{};
  const int ncls = igemm_dgrad_setup(p, dy, dyd, nullptr, nullptr, dxd, k, stride, pad, 0.f);
  if (ncls <= 0) return 0;
  const dim3 grid = igemm_plan(p, ncls).grid;
  return (int64_t)grid.x * grid.z;
}

// Round 6: every data-gradient kernel family writes the partials -- the direct 3x3 kernels
// (round 3), the persistent 1x1 GEMM and the gather kernel (every other conv, incl. the
// stride-2 classes) -- so the rows follow vae2_conv2d_bwd_data's own dispatch.
int64_t vae2_conv2d_bwd_data_bnpart_rows(const float* dy, const vae2_act* dyd,
                                         const vae2_act* dxd, int k, int stride, int pad) {
  if (!dy || !conv_shapes_ok(dxd, dyd, k, stride, pad) || !fits32(dxd) || !fits32(dyd))
    return 0;
  if (g_bf16) return 0;
  if (dconv_use(dyd, dxd, k, stride, pad, dy)) return dconv_rows(dyd, dxd);
  G1Tile g1;
  if (gemm1_pick(dyd, dxd, k, stride, pad, dy, &g1)) return g1.grid_x;
  return igemm_dgrad_rows(dy, dyd, dxd, k, stride, pad);
}

int vae2_conv2d_bwd_data_bnpart(const float* dy, const vae2_act* dyd, const float* wp,
                                float* dx, const vae2_act* dxd, int k, int stride, int pad,
                                const float* bn_x, const vae2_act* bn_xd, const float* bn_save,
                                int relu, float* partials, void* stream) {
  const char* fn = "vae2_conv2d_bwd_data_bnpart";
  VAE2_REQUIRE(dy && wp && dx && bn_x && bn_xd && bn_save && partials, fn, "null pointer");
  VAE2_REQUIRE(conv_shapes_ok(dxd, dyd, k, stride, pad), fn, "inconsistent conv shapes");
  VAE2_REQUIRE(bn_xd->n == dxd->n && bn_xd->h == dxd->h && bn_xd->w == dxd->w &&
               bn_xd->c == dxd->c && bn_xd->ps >= bn_xd->c && fits32(bn_xd), fn,
               "BatchNorm input shape must match dx");
  VAE2_REQUIRE(vae2_conv2d_bwd_data_bnpart_rows(dy, dyd, dxd, k, stride, pad) > 0, fn,
               "BatchNorm partials are not available for this geometry "
               "(vae2_conv2d_bwd_data_bnpart_rows)");
  const uint32_t wbytes = packed_bytes(dyd->c, dxd->c, k, 1);
  if (dconv_use(dyd, dxd, k, stride, pad, dy)) {
    BnSide bn;
    bn.bx = bn_x;
    bn.bx_ps = (int)bn_xd->ps;
    bn.bx_bytes = act_bytes(bn_xd);
    bn.bsave = bn_save;
    bn.brelu = relu ? 1 : 0;
    return launch_dconv(dy, dyd, wp, wbytes, nullptr, dx, dxd, 0.f, partials, true,
                        as_stream(stream), fn, bn);
  }
  G1Tile g1;
  if (gemm1_pick(dyd, dxd, k, stride, pad, dy, &g1)) {
    const int rc = launch_gemm1(dy, dyd, wp, wbytes, nullptr, dx, dxd, 0.f, partials, g1,
                                as_stream(stream), fn, bn_x, (int)bn_xd->ps, relu ? 1 : 0,
                                bn_save, act_bytes(bn_xd));
    VAE2_REQUIRE(rc != -1, fn, "1x1 GEMM refused the partials form");
    return rc;
  }
  IGemm p{};
  const int ncls = igemm_dgrad_setup(p, dy, dyd, wp, dx, dxd, k, stride, pad, 0.f);
  VAE2_REQUIRE(ncls > 0, fn, "stride > 2 is not supported");
  p.stats = partials;
  p.bx = bn_x;
  p.bx_ps = (int)bn_xd->ps;
  p.bx_bytes = act_bytes(bn_xd);
  p.bsave = bn_save;
  p.brelu = relu ? 1 : 0;
  return launch_igemm(p, 1, as_stream(stream), fn, ncls);
}

int vae2_conv2d_bwd_data(const float* dy, const vae2_act* dyd, const float* wp,
                         float* dx, const vae2_act* dxd, int k, int stride,
                         int pad, float beta, void* stream) {
  const char* fn = "vae2_conv2d_bwd_data";
  VAE2_REQUIRE(dy && wp && dx, fn, "null pointer");
  VAE2_REQUIRE(conv_shapes_ok(dxd, dyd, k, stride, pad), fn, "inconsistent conv shapes");
  VAE2_REQUIRE(fits32(dxd) && fits32(dyd), fn, "tensor too large for 32-bit indexing");
  if (dconv_use(dyd, dxd, k, stride, pad, dy))
    return launch_dconv(dy, dyd, wp, packed_bytes(dyd->c, dxd->c, k, 1), nullptr, dx, dxd, beta,
                        nullptr, true, as_stream(stream), fn);
  G1Tile g1;
  if (gemm1_pick(dyd, dxd, k, stride, pad, dy, &g1)) {
    const int rc = launch_gemm1(dy, dyd, wp, packed_bytes(dyd->c, dxd->c, k, 1), nullptr, dx,
                                dxd, beta, nullptr, g1, as_stream(stream), fn);
    if (rc != -1) return rc;
  }
  IGemm p{};
  const int ncls = igemm_dgrad_setup(p, dy, dyd, wp, dx, dxd, k, stride, pad, beta);
  VAE2_REQUIRE(ncls >= 0, fn, "stride > 2 is not supported");
  if (ncls == 0) return 0;
  return launch_igemm(p, 1, as_stream(stream), fn, ncls);
}

}  // extern "C"

// What the four convolution units share (conv.hip: weight packing, switches, forward and
// data-gradient C ABI; conv_gather.hip: gather implicit GEMM and persistent 1x1 GEMM;
// conv_direct.hip: direct 3x3; conv_wgrad.hip: weight gradients): the parameter and tile
// structs that cross a unit boundary, the switch declarations, and the prototypes of the
// pickers and launchers one unit calls in another.  Kernel templates and the structs only
// their own launchers fill live in the unit that instantiates them.
#pragma once

#include "common.h"

namespace vae2 {

static inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// ------------------------------------------------------------ igemm ----
struct IGemm {
  const float* a;  // gathered activation (NHWC)
  int a_ps, a_c, a_c4, a_h, a_w;
  int g_n, g_h, g_w;  // iteration grid, M = g_n*g_h*g_w
  int a_step;         // A source row = g*a_step + d(tap)
  int nth, ntw;       // taps: t = th*ntw + tw
  int dh0, dhs, dw0, dws;
  int kh0, khs, kw0, kws, ksz;  // weight tap (kh0 + th*khs, kw0 + tw*kws) of a ksz x ksz kernel
  const float* w;               // packed [Npad][ksz*ksz][a_c4]
  uint32_t a_bytes, w_bytes;    // buffer extents for the range-checked loads
  int n;                        // GEMM N (real)
  const float* bias;
  float* y;
  int y_ps, y_h, y_w, y_step, y_offh, y_offw;
  float beta;
  float* stats;  // [2][gridDim.x][n] or null
  int vec_out;   // y 16-byte aligned, y_ps % 4 == 0, no statistics with beta != 0
  FastDiv hw_div, w_div;  // divide by g_h*g_w, g_w
  int ktab;               // use the K-step table (set_tune key 12, default on)
  // Data gradient (ROLE 1) with bx set (round 6): y is the gradient of a BatchNorm(+ReLU)
  // layer's output whose only consumer is this conv; the epilogue writes that layer's
  // backward partials (sum g, sum g*xhat; g = y masked by the ReLU recomputed from bx)
  // into stats, [2][gridDim.x * gridDim.z][n] (row = class * gridDim.x + tile), instead of
  // the layer's own reduce pass.  bx = its pre-BN tensor (y's pixels and channels).
  const float* bx;
  int bx_ps, brelu;
  const float* bsave;
  uint32_t bx_bytes;
  // Strided data gradient: one launch covers every stride-parity class of the input
  // pixels, class = blockIdx.z (gridDim.z == 1: the fields above are used as they are).
  struct Cls {
    int g_h, g_w, nth, ntw, dh0, dw0, kh0, kw0, y_offh, y_offw;
    FastDiv hw_div, w_div;
  } cls[4];
};

// ------------------------------------------------------------ tiling ----
struct Tile {
  int tm, tn, nblk;
  int ks = 1;  // in-workgroup K split (igemm_kernel KS)
  int nr = 0;  // output channels on the VALU beside the MFMA columns (igemm_kernel NR)
};

// Launch geometry of the gather kernel for p and its ncls stride-parity classes (1: p's
// plain fields; > 1: p.cls[0..ncls), the grid covering the largest).  The launcher, both
// partial-statistics rows queries and the kernel-name query all take it from here.
struct IGemmPlan {
  Tile t;
  int64_t M;     // GEMM rows of the largest class
  int max_taps;  // taps of the class with the most
  dim3 grid;     // (row tiles, N blocks, classes); statistics rows = grid.x * grid.z
};
IGemmPlan igemm_plan(const IGemm& p, int ncls);

// --------------------------------------------------------- switches ----
// Process-global; vae2_conv2d_set_algo / _set_mfma_bf16 / _set_tune (the table in conv.hip
// documents every key) write them.  Each is defined in the file its comment names.
extern int g_wide_tiles, g_ksplit, g_bf16, g_conv_algo, g_dconv_nr, g_gemm1, g_vec_out,
    g_dconv_nr_wide, g_igemm_minblk, g_wgrad_cols, g_dconv_nw8, g_wgrad_nw8, g_gemm1_tn,
    g_gemm1_tm, g_igemm_nr, g_wgrad_narrow, g_igemm_tab, g_dconv_n16, g_dconv_split72,
    g_dconv_ksp, g_wgrad_wgs;                                               // conv.hip
extern int g_dconv_stream, g_dconv_stream_wpc, g_dconv_stream_bl, g_dconv_stream_spb;  // dconv_stream.hip
extern int g_wgrad_narrow_tps;                                              // wgrad_narrow.hip
extern int g_bn_v2, g_bn_blocks, g_bn_apply_res;                            // bn.hip
extern int g_fuse_quad;                                                     // resample.hip

// Bytes of a packed weight (vae2_conv2d_packed_size floats), for buffer descriptors.
inline uint32_t packed_bytes(int64_t cout, int64_t cin, int k, int mode) {
  return (uint32_t)(vae2_conv2d_packed_size(cout, cin, k, mode) * 4);
}

inline bool vec_ok(const float* a, int ps) {
  return ((uintptr_t)a % 16 == 0) && (ps % 4 == 0);
}

inline bool conv_shapes_ok(const vae2_act* xd, const vae2_act* yd, int k, int stride, int pad) {
  if (!act_ok(xd) || !act_ok(yd)) return false;
  if (xd->n != yd->n) return false;
  if (k < 1 || stride < 1 || pad < 0) return false;
  int64_t oh = (xd->h + 2 * pad - k) / stride + 1;
  int64_t ow = (xd->w + 2 * pad - k) / stride + 1;
  return oh == yd->h && ow == yd->w;
}

inline bool fits32(const vae2_act* d) {
  return d->n * d->h * d->w * d->ps < (int64_t(1) << 29);  // byte offsets < 2^31
}

// Bytes spanned by an activation view, for buffer descriptors.  With 16-byte
// aligned pixels (ps % 4 == 0) the last pixel's final 4-channel quad is included
// (it lies inside the pixel stride), so a whole-access range check never drops
// real channels of the last quad.
inline uint32_t act_bytes(const vae2_act* d) {
  int64_t tail = (d->ps % 4 == 0) ? ((d->c + 3) / 4 * 4) : d->c;
  int64_t last = ((d->n * d->h * d->w) - 1) * d->ps + tail;
  return (uint32_t)(last * 4);
}

struct G1Tile {
  int tm = 2, tn, nblk, grid_x;
  size_t lds;
};
int launch_igemm(IGemm& p, int role, hipStream_t s, const char* fn, int ncls = 1);
int launch_gemm1(const float* a, const vae2_act* ad, const float* wp, uint32_t w_bytes,
                 const float* bias, float* y, const vae2_act* yd, float beta, float* stats,
                 const G1Tile& t, hipStream_t s, const char* fn, const float* bx = nullptr,
                 int bx_ps = 0, int brelu = 0, const float* bsave = nullptr,
                 uint32_t bx_bytes = 0);

struct DTile {
  int tm, tn, nblk, cs4, tiles_h, tiles_w;
  int nr = 0;  // output channels on the VALU beside the MFMA tiles (dconv3_body NR)
  int nw = 4;  // waves per workgroup (dconv3_body NW); tile rows = nw * tm / 2
  int ks = 1;  // K shares over 4-wave sets (dconv3_body KS, nw = 4 ks, tile rows = 2 tm)
};

// BatchNorm fused at a direct-3x3 conv's input (DConv::isave / irelu) or, for its data
// gradient, that BatchNorm's backward partials in the epilogue (DConv::bx ...).
struct BnSide {
  const float* isave = nullptr;
  int irelu = 0;
  const float* bx = nullptr;
  int bx_ps = 0, brelu = 0;
  const float* bsave = nullptr;
  uint32_t bx_bytes = 0;
};

int launch_dconv(const float* a, const vae2_act* ad, const float* wp, uint32_t w_bytes,
                 const float* bias, float* y, const vae2_act* yd, float beta,
                 float* stats, bool flip, hipStream_t s, const char* fn,
                 const BnSide& bn = BnSide{});

// conv_gather.hip
Tile pick_tile(int64_t M, int N, bool wide = false);
bool gemm1_pick(const vae2_act* ad, const vae2_act* yd, int k, int stride, int pad,
                const float* a, G1Tile* out);
// conv_direct.hip: which convs the direct / streaming 3x3 kernels take, their tile and
// their partial-statistics rows
DTile pick_dtile(const vae2_act* ad, const vae2_act* yd, bool remainder = true);
bool stream_use(const vae2_act* ad, const vae2_act* yd);
bool dconv_use(const vae2_act* ad, const vae2_act* yd, int k, int stride, int pad,
               const float* a);
int64_t dconv_rows(const vae2_act* ad, const vae2_act* yd);
// conv_wgrad.hip: the direct weight-gradient kernel takes this geometry
bool wgrad3_shape_ok(const vae2_act* xd, const vae2_act* dyd, int k, int stride, int pad);

}  // namespace vae2

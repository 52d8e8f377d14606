// ELBO terms, reparameterisation sampler, anomaly check and the Adam / SGD steps.
//
//   L1Loss (criterion.py:61-69)            -> vae2_l1_fwd / vae2_l1_bwd
//   KLLoss (criterion.py:72-87) + reparam
//     z = mu + exp(0.5*logvar)*eps (utils.py:85-101) -> vae2_reparam_kl_fwd / _bwd
//   loss assembly (utils.py:150-152)       -> vae2_weighted_sum
//   _anomoly_detection (utils.py:63-65)    -> vae2_nonfinite_check
//   torch.optim.Adam (train.py:251-261)    -> vae2_adam_step
//   torch.optim.SGD (train.py:232-250)     -> vae2_sgd_step
//   weight EMA (swa_utils.AveragedModel + get_ema_multi_avg_fn; not in the reference)
//                                          -> vae2_ema_coeffs / vae2_ema_update_dev
//   lsgan_adversarial_loss (criterion.py:90-103): MSELoss(sum) vs ones / zeros / batch
//                                          -> vae2_lsgan_fwd / vae2_lsgan_bwd
#include "common.h"

namespace vae2 {

static unsigned reduce_blocks(int64_t n) {
  int64_t b = ceil_div(n, 256 * 4);
  if (b > 1024) b = 1024;
  if (b < 1) b = 1;
  return (unsigned)b;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float s = 0.f;
  if (tid == 0) s = red[0] + red[1] + red[2] + red[3];
  return s;  // valid in thread 0
}

__global__ __launch_bounds__(256) void l1_partials_kernel(const float* __restrict__ p, Act pd,
                                                          const float* __restrict__ t, Act td,
                                                          float* __restrict__ ws,
                                                          FastDiv cdiv) {
  __shared__ float red[4];
  const uint32_t C = (uint32_t)pd.c;
  const uint32_t total = (uint32_t)(pd.n * pd.h * pd.w) * C;
  float s = 0.f;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    uint32_t px = cdiv.div(i);
    uint32_t c = i - px * C;
    s += fabsf(p[(int64_t)px * pd.ps + c] - t[(int64_t)px * td.ps + c]);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// out[0] (+)= scale * sum(ws[0..n))   (single block, fixed order)
__global__ __launch_bounds__(256) void finish_sum_kernel(const float* __restrict__ ws, int n,
                                                         float scale, float* out,
                                                         int accumulate) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)ws[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = (float)(red[0] + red[1] + red[2] + red[3]) * scale;
    out[0] = accumulate ? out[0] + v : v;
  }
}

__global__ __launch_bounds__(256) void l1_bwd_kernel(const float* __restrict__ p, Act pd,
                                                     const float* __restrict__ t, Act td,
                                                     const float* __restrict__ gout, float scale,
                                                     float* __restrict__ dp, Act dpd, float beta,
                                                     FastDiv cdiv) {
  const uint32_t C = (uint32_t)pd.c;
  const uint32_t total = (uint32_t)(pd.n * pd.h * pd.w) * C;
  const float g = gout[0] * scale;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    uint32_t px = cdiv.div(i);
    uint32_t c = i - px * C;
    float d = p[(int64_t)px * pd.ps + c] - t[(int64_t)px * td.ps + c];
    float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    float* dst = dp + (int64_t)px * dpd.ps + c;
    float v = sg * g;
    *dst = (beta != 0.f) ? v + beta * *dst : v;
  }
}

// sum (x - target)^2 partials (target a constant: 1 for 'real', 0 for 'fake')
__global__ __launch_bounds__(256) void sqdiff_partials_kernel(const float* __restrict__ x, Act xd,
                                                              float target,
                                                              float* __restrict__ ws,
                                                              FastDiv cdiv) {
  __shared__ float red[4];
  const uint32_t C = (uint32_t)xd.c;
  const uint32_t total = (uint32_t)(xd.n * xd.h * xd.w) * C;
  float s = 0.f;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    uint32_t px = cdiv.div(i);
    uint32_t c = i - px * C;
    const float d = x[(int64_t)px * xd.ps + c] - target;
    s = __builtin_fmaf(d, d, s);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// dx (+)= 2 * scale * gout * (x - target)
__global__ __launch_bounds__(256) void sqdiff_bwd_kernel(const float* __restrict__ x, Act xd,
                                                         float target,
                                                         const float* __restrict__ gout,
                                                         float scale, float* __restrict__ dx,
                                                         Act dxd, float beta, FastDiv cdiv) {
  const uint32_t C = (uint32_t)xd.c;
  const uint32_t total = (uint32_t)(xd.n * xd.h * xd.w) * C;
  const float g = 2.f * gout[0] * scale;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    uint32_t px = cdiv.div(i);
    uint32_t c = i - px * C;
    const float v = g * (x[(int64_t)px * xd.ps + c] - target);
    float* dst = dx + (int64_t)px * dxd.ps + c;
    *dst = (beta != 0.f) ? v + beta * *dst : v;
  }
}

__global__ __launch_bounds__(256) void reparam_kl_kernel(const float* __restrict__ mv, Act md,
                                                         const float* __restrict__ eps, Act ed,
                                                         float* __restrict__ z, Act zd,
                                                         int prior, float* __restrict__ ws,
                                                         FastDiv cdiv) {
  __shared__ float red[4];
  const uint32_t Z = (uint32_t)zd.c;
  const uint32_t total = (uint32_t)(zd.n * zd.h * zd.w) * Z;
  float s = 0.f;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    uint32_t px = cdiv.div(i);
    uint32_t c = i - px * Z;
    float mu = mv[(int64_t)px * md.ps + c];
    float lv = mv[(int64_t)px * md.ps + Z + c];
    float e = eps[(int64_t)px * ed.ps + c];
    z[(int64_t)px * zd.ps + c] = prior ? e : mu + expf(lv * 0.5f) * e;
    s += 0.5f * (mu * mu + expf(lv) - lv - 1.f);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void reparam_kl_bwd_kernel(
    const float* __restrict__ mv, Act md, const float* __restrict__ eps, Act ed,
    const float* __restrict__ dz, Act dzd, const float* __restrict__ gkl, float scale,
    float* __restrict__ dmv, Act dmd, FastDiv cdiv) {
  const uint32_t Z = (uint32_t)ed.c;
  const uint32_t total = (uint32_t)(ed.n * ed.h * ed.w) * Z;
  const float gk = gkl ? gkl[0] * scale : 0.f;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    uint32_t px = cdiv.div(i);
    uint32_t c = i - px * Z;
    float mu = mv[(int64_t)px * md.ps + c];
    float lv = mv[(int64_t)px * md.ps + Z + c];
    float e = eps[(int64_t)px * ed.ps + c];
    float g = dz ? dz[(int64_t)px * dzd.ps + c] : 0.f;
    float dmu = g + gk * mu;
    float dlv = g * e * 0.5f * expf(lv * 0.5f) + gk * 0.5f * (expf(lv) - 1.f);
    dmv[(int64_t)px * dmd.ps + c] = dmu;
    dmv[(int64_t)px * dmd.ps + Z + c] = dlv;
  }
}

struct WSum {
  const float* t[8];
  float l[8];
  int n;
};

__global__ void weighted_sum_kernel(WSum w, float* total) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float s = 0.f;
  for (int i = 0; i < w.n; ++i) s += w.l[i] * w.t[i][0];
  total[0] = s;
}

__global__ __launch_bounds__(256) void nonfinite_kernel(const float* __restrict__ x, int64_t n,
                                                        int32_t* flag) {
  bool bad = false;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float v = x[i];
    bad |= !isfinite(v);
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p,
                                                   const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   int64_t n, float lr_corr, float b1,
                                                   float b2, float eps, float wd,
                                                   float bc2_sqrt) {
  const float w1 = 1.f - b1;
  const float w2 = 1.f - b2;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gi = g[i];
    float pi = p[i];
    if (wd != 0.f) gi = gi + wd * pi;
    float mi = m[i];
    mi = mi + w1 * (gi - mi);  // lerp(m, g, 1 - b1), weight < 0.5 branch
    float vi = v[i] * b2 + w2 * (gi * gi);
    float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi + (-lr_corr) * (mi / denom);
    m[i] = mi;
    v[i] = vi;
  }
}

// Device-resident step counter for graph replay: state = {step, lr} (double),
// coeffs = {lr / (1 - b1^step), sqrt(1 - b2^step)} (float), as vae2_adam_step's host math.
__global__ void adam_coeffs_kernel(double* state, float b1, float b2, float* coeffs) {
  const double step = state[0] + 1.0;
  state[0] = step;
  const double lr = (double)(float)state[1];
  coeffs[0] = (float)(lr / (1.0 - pow((double)b1, step)));
  coeffs[1] = (float)sqrt(1.0 - pow((double)b2, step));
}

// A product rounded to fp32 on its own: never contracted into a multiply-add that follows.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// CLIP: every gradient element is first multiplied by clip[1] (vae2_clip_coeffs), rounded on
// its own, so the step equals the unclipped one on a pre-scaled gradient bit for bit.
template <bool CLIP>
__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p,
                                                       const float* __restrict__ g,
                                                       float* __restrict__ m,
                                                       float* __restrict__ v, int64_t n,
                                                       const float* __restrict__ coeffs,
                                                       const float* __restrict__ clip,
                                                       float b1, float b2, float eps, float wd) {
  const float lr_corr = coeffs[0];
  const float bc2_sqrt = coeffs[1];
  const float w1 = 1.f - b1;
  const float w2 = 1.f - b2;
  float cc = 1.f;
  if (CLIP) cc = clip[1];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gi = g[i];
    if (CLIP) gi = mul_rn(gi, cc);
    float pi = p[i];
    // (hipcc contracts the unclipped form to this fused multiply-add; with the clip product
    //  in front it would pair the two multiplies instead and round wd * p on its own)
    if (wd != 0.f) gi = CLIP ? __builtin_fmaf(wd, pi, gi) : gi + wd * pi;
    float mi = m[i];
    mi = mi + w1 * (gi - mi);
    float vi = v[i] * b2 + w2 * (gi * gi);
    float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi + (-lr_corr) * (mi / denom);
    m[i] = mi;
    v[i] = vi;
  }
}

// torch.optim.SGD.  c = {lr, 1 - dampening, first step ? 1 : 0}: from device memory
// (sgd_coeffs_kernel, graph replay) or, with coeffs == nullptr, the host's copy.
struct SgdCoef {
  float lr, damp1, first;
};

__global__ void sgd_coeffs_kernel(double* state, float dampening, float* coeffs) {
  const double step = state[0] + 1.0;
  state[0] = step;
  coeffs[0] = (float)state[1];
  coeffs[1] = (float)(1.0 - (double)dampening);
  coeffs[2] = step == 1.0 ? 1.f : 0.f;
}

// One element of the step; b is the momentum buffer's value, read only when MOM and not the
// first step.  The multiply-adds are written out as fused ones, in torch's operand order, so
// the 16-byte body and the scalar path give the same bits whatever the compiler would contract.
template <bool MOM>
__device__ __forceinline__ void sgd_update(float& p, float g, float& b, const SgdCoef c,
                                           float momentum, float wd, bool nesterov) {
  if (wd != 0.f) g = __builtin_fmaf(wd, p, g);
  float d = g;
  if (MOM) {
    b = c.first != 0.f ? g : __builtin_fmaf(c.damp1, g, momentum * b);
    d = nesterov ? __builtin_fmaf(momentum, b, g) : b;
  }
  p = __builtin_fmaf(-c.lr, d, p);
}

// nq: quads taken with 16-byte accesses (0 when a pointer is not 16-byte aligned); the
// elements from 4 * nq on take the scalar loop.
// CLIP: the gradient is first multiplied by clip[1], as in adam_dev_kernel<true>.
template <bool MOM, bool CLIP>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p,
                                                  const float* __restrict__ g,
                                                  float* __restrict__ buf, int64_t n,
                                                  int64_t nq, const float* __restrict__ coeffs,
                                                  const float* __restrict__ clip,
                                                  SgdCoef c, float momentum, float wd,
                                                  int nesterov) {
  if (coeffs) c = SgdCoef{coeffs[0], coeffs[1], coeffs[2]};
  float cc = 1.f;
  if (CLIP) cc = clip[1];
  const bool nes = nesterov != 0;
  const bool first = c.first != 0.f;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  f4* p4 = reinterpret_cast<f4*>(p);
  const f4* g4 = reinterpret_cast<const f4*>(g);
  f4* b4 = reinterpret_cast<f4*>(buf);
  for (int64_t i = tid; i < nq; i += stride) {
    f4 pv = p4[i];
    const f4 gv = g4[i];
    f4 bv = {0.f, 0.f, 0.f, 0.f};
    if (MOM && !first) bv = b4[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pk = pv[k], bk = bv[k];
      sgd_update<MOM>(pk, CLIP ? mul_rn(gv[k], cc) : gv[k], bk, c, momentum, wd, nes);
      pv[k] = pk;
      bv[k] = bk;
    }
    p4[i] = pv;
    if (MOM) b4[i] = bv;
  }
  for (int64_t i = 4 * nq + tid; i < n; i += stride) {
    float pv = p[i];
    const float gv = g[i];
    float bv = 0.f;
    if (MOM && !first) bv = buf[i];
    sgd_update<MOM>(pv, CLIP ? mul_rn(gv, cc) : gv, bv, c, momentum, wd, nes);
    p[i] = pv;
    if (MOM) buf[i] = bv;
  }
}

// Argument rules shared by the three SGD entry points (torch.optim.SGD's own).
inline const char* sgd_args_error(float momentum, float dampening, float wd, int nesterov) {
  if (!(momentum >= 0.f)) return "momentum must be >= 0";
  if (!(wd >= 0.f)) return "weight_decay must be >= 0";
  if (nesterov && (!(momentum > 0.f) || dampening != 0.f))
    return "nesterov momentum requires a momentum and zero dampening";
  return nullptr;
}

template <bool CLIP>
inline int sgd_launch(const char* fn, float* p, const float* g, float* buf, int64_t n,
                      const float* coeffs, const float* clip, SgdCoef c, float momentum,
                      float wd, int nesterov, void* stream) {
  if (n == 0) return 0;
  const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)buf;
  const int64_t nq = (bits & 15) == 0 ? n / 4 : 0;
  const unsigned nb = ew_blocks(nq ? nq : n, 256, 4096);
  if (momentum != 0.f)
    VAE2_LAUNCH((sgd_kernel<true, CLIP>), dim3(nb), dim3(256), 0, as_stream(stream), p, g, buf,
                n, nq, coeffs, clip, c, momentum, wd, nesterov);
  else
    VAE2_LAUNCH((sgd_kernel<false, CLIP>), dim3(nb), dim3(256), 0, as_stream(stream), p, g, buf,
                n, nq, coeffs, clip, c, momentum, wd, nesterov);
  return check_launch(fn);
}

// Exponential moving average of the weights (torch.optim.swa_utils.AveragedModel with
// get_ema_multi_avg_fn(decay)).  c = {w = 1 - decay, first update ? 1 : 0}: from device memory
// (ema_coeffs_kernel, graph replay) or, with coeffs == nullptr, the host's copy.
struct EmaCoef {
  float w, first;
};

// state[0] counts the updates; the weight is rounded once, from the double 1 - decay.
__global__ void ema_coeffs_kernel(double* state, float decay, float* coeffs) {
  const double count = state[0] + 1.0;
  state[0] = count;
  coeffs[0] = (float)(1.0 - (double)decay);
  coeffs[1] = count == 1.0 ? 1.f : 0.f;
}

// lerp(ema, p, w) in torch's form for w < 0.5, used for every w: one explicit fused
// multiply-add, so the 16-byte body and the scalar path give the same bits.
__device__ __forceinline__ float ema_update(float e, float p, float w) {
  return __builtin_fmaf(w, p - e, e);
}

// First update: ema = p, moved as 32-bit words (the float's bits, whatever they are) and ema
// is not read.  Afterwards ema += w * (p - ema).  nq as in sgd_kernel; p is read only.
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema,
                                                         const float* __restrict__ p, int64_t n,
                                                         int64_t nq,
                                                         const float* __restrict__ coeffs,
                                                         EmaCoef c) {
  if (coeffs) c = EmaCoef{coeffs[0], coeffs[1]};
  const float w = c.w;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (c.first != 0.f) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    u4* e4 = reinterpret_cast<u4*>(ema);
    const u4* p4 = reinterpret_cast<const u4*>(p);
    uint32_t* e1 = reinterpret_cast<uint32_t*>(ema);
    const uint32_t* p1 = reinterpret_cast<const uint32_t*>(p);
    for (int64_t i = tid; i < nq; i += stride) e4[i] = p4[i];
    for (int64_t i = 4 * nq + tid; i < n; i += stride) e1[i] = p1[i];
    return;
  }
  f4* e4 = reinterpret_cast<f4*>(ema);
  const f4* p4 = reinterpret_cast<const f4*>(p);
  for (int64_t i = tid; i < nq; i += stride) {
    f4 ev = e4[i];
    const f4 pv = p4[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) ev[k] = ema_update(ev[k], pv[k], w);
    e4[i] = ev;
  }
  for (int64_t i = 4 * nq + tid; i < n; i += stride) ema[i] = ema_update(ema[i], p[i], w);
}

// Argument rules shared by the EMA entry points.
inline const char* ema_decay_error(float decay) {
  return decay >= 0.f && decay < 1.f ? nullptr : "decay must be in [0, 1) (and not NaN)";
}

inline int ema_launch(const char* fn, float* ema, const float* p, int64_t n,
                      const float* coeffs, EmaCoef c, void* stream) {
  if (n == 0) return 0;
  const uintptr_t bits = (uintptr_t)ema | (uintptr_t)p;
  const int64_t nq = (bits & 15) == 0 ? n / 4 : 0;
  VAE2_LAUNCH(ema_update_kernel, dim3(ew_blocks(nq ? nq : n, 256, 4096)), dim3(256), 0,
              as_stream(stream), ema, p, n, nq, coeffs, c);
  return check_launch(fn);
}

// Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, 2-norm).  The block count
// depends on n alone, so the summation order -- and the norm -- is the same in every run.
constexpr int64_t kNormBlocks = 2048;  // 8 blocks of 256 threads per CU
static unsigned norm_blocks(int64_t n) {
  int64_t b = ceil_div(n, 256 * 4);
  if (b > kNormBlocks) b = kNormBlocks;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// partials[block] = sum of g^2 over the block's grid-stride share, in fp64: the square of an
// fp32 value is exact there and the summation error stays far below half an fp32 ulp of the
// norm.  Every block writes its slot (no zeroing, no atomics).  nq as in sgd_kernel.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n,
                                                         int64_t nq,
                                                         double* __restrict__ partials) {
  __shared__ double red[4];
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const f4* g4 = reinterpret_cast<const f4*>(g);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 4
  for (int64_t i = tid; i < nq; i += stride) {
    const f4 v = g4[i];
    const double a = (double)v[0], b = (double)v[1], c = (double)v[2], d = (double)v[3];
    s0 = fma(a, a, s0);
    s1 = fma(b, b, s1);
    s2 = fma(c, c, s2);
    s3 = fma(d, d, s3);
  }
  for (int64_t i = 4 * nq + tid; i < n; i += stride) {
    const double a = (double)g[i];
    s0 = fma(a, a, s0);
  }
  double s = wave_sum_d((s0 + s1) + (s2 + s3));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// clip[0] = the total norm, clip[1] = torch's clip coefficient, both fp32 (single block, fixed
// order).  A NaN norm gives a NaN coefficient, an infinite one 0.
__global__ __launch_bounds__(256) void clip_coeffs_kernel(const double* __restrict__ partials,
                                                          int64_t count, float max_norm,
                                                          float* __restrict__ clip) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) s += partials[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
    const float c = max_norm / (t + 1e-6f);
    clip[0] = t;
    clip[1] = c > 1.f ? 1.f : c;
  }
}

// x *= clip[1] in place (the second pass of the stand-alone clip_grad_norm_).
__global__ __launch_bounds__(256) void clip_scale_kernel(float* __restrict__ x, int64_t n,
                                                         int64_t nq,
                                                         const float* __restrict__ clip) {
  const float cc = clip[1];
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  f4* x4 = reinterpret_cast<f4*>(x);
  for (int64_t i = tid; i < nq; i += stride) {
    f4 v = x4[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = mul_rn(v[k], cc);
    x4[i] = v;
  }
  for (int64_t i = 4 * nq + tid; i < n; i += stride) x[i] = mul_rn(x[i], cc);
}

inline const char* max_norm_error(float max_norm) {
  return max_norm > 0.f ? nullptr : "max_norm must be > 0 (and not NaN)";
}

__global__ void scale_kernel(float* dst, const float* src, int64_t n, float s) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = src[i] * s;
}

}  // namespace vae2

using namespace vae2;

extern "C" {

int64_t vae2_reduce_ws_size(int64_t n) { return reduce_blocks(n); }

int vae2_l1_fwd(const float* p, const vae2_act* pd, const float* t,
                const vae2_act* td, float scale, float* ws, float* out,
                void* stream) {
  const char* fn = "vae2_l1_fwd";
  VAE2_REQUIRE(p && t && ws && out && act_ok(pd) && act_ok(td), fn, "bad arguments");
  VAE2_REQUIRE(pd->n == td->n && pd->h == td->h && pd->w == td->w && pd->c == td->c, fn,
               "predict / target shape mismatch");
  VAE2_REQUIRE(idx32_ok(pd), fn, kTooLarge);
  int64_t total = act_elems(pd);
  unsigned nb = reduce_blocks(total);
  hipStream_t s = as_stream(stream);
  VAE2_LAUNCH(l1_partials_kernel, dim3(nb), dim3(256), 0, s, p, to_act(pd), t,
                     to_act(td), ws, FastDiv((uint32_t)pd->c));
  int rc = check_launch(fn);
  if (rc) return rc;
  VAE2_LAUNCH(finish_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, (int)nb,
                     scale, out, 0);
  return check_launch(fn);
}

int vae2_l1_bwd(const float* p, const vae2_act* pd, const float* t,
                const vae2_act* td, const float* gout, float scale, float* dp,
                const vae2_act* dpd, float beta, void* stream) {
  const char* fn = "vae2_l1_bwd";
  VAE2_REQUIRE(p && t && gout && dp && act_ok(pd) && act_ok(td) && act_ok(dpd), fn,
               "bad arguments");
  VAE2_REQUIRE(same_shape(td, pd), fn, "predict / target shape mismatch");
  VAE2_REQUIRE(same_shape(dpd, pd), fn, "dp shape mismatch");
  VAE2_REQUIRE(idx32_ok(pd), fn, kTooLarge);
  int64_t total = act_elems(pd);
  VAE2_LAUNCH(l1_bwd_kernel, dim3(ew_blocks(total)), dim3(256), 0, as_stream(stream), p,
                     to_act(pd), t, to_act(td), gout, scale, dp, to_act(dpd), beta,
                     FastDiv((uint32_t)pd->c));
  return check_launch(fn);
}

int vae2_lsgan_fwd(const float* x, const vae2_act* xd, float target, float scale, float* ws,
                   float* out, void* stream) {
  const char* fn = "vae2_lsgan_fwd";
  VAE2_REQUIRE(x && ws && out && act_ok(xd), fn, "bad arguments");
  VAE2_REQUIRE(idx32_ok(xd), fn, kTooLarge);
  const int64_t total = act_elems(xd);
  const unsigned nb = reduce_blocks(total);
  hipStream_t s = as_stream(stream);
  VAE2_LAUNCH(sqdiff_partials_kernel, dim3(nb), dim3(256), 0, s, x, to_act(xd), target,
                     ws, FastDiv((uint32_t)xd->c));
  int rc = check_launch(fn);
  if (rc) return rc;
  VAE2_LAUNCH(finish_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, (int)nb,
                     scale, out, 0);
  return check_launch(fn);
}

int vae2_lsgan_bwd(const float* x, const vae2_act* xd, float target, const float* gout,
                   float scale, float* dx, const vae2_act* dxd, float beta, void* stream) {
  const char* fn = "vae2_lsgan_bwd";
  VAE2_REQUIRE(x && gout && dx && act_ok(xd) && act_ok(dxd), fn, "bad arguments");
  VAE2_REQUIRE(dxd->n == xd->n && dxd->h == xd->h && dxd->w == xd->w && dxd->c == xd->c, fn,
               "dx shape mismatch");
  VAE2_REQUIRE(idx32_ok(xd), fn, kTooLarge);
  const int64_t total = act_elems(xd);
  VAE2_LAUNCH(sqdiff_bwd_kernel, dim3(ew_blocks(total)), dim3(256), 0, as_stream(stream),
                     x, to_act(xd), target, gout, scale, dx, to_act(dxd), beta,
                     FastDiv((uint32_t)xd->c));
  return check_launch(fn);
}

int vae2_reparam_kl_fwd(const float* muvar, const vae2_act* md,
                        const float* eps, const vae2_act* ed, float* z,
                        const vae2_act* zd, int prior, float scale,
                        float* kl_out, int accumulate, float* ws, void* stream) {
  const char* fn = "vae2_reparam_kl_fwd";
  VAE2_REQUIRE(muvar && eps && z && kl_out && ws && act_ok(md) && act_ok(ed) && act_ok(zd), fn,
               "bad arguments");
  VAE2_REQUIRE(md->c == 2 * zd->c && ed->c == zd->c, fn, "channel mismatch");
  VAE2_REQUIRE(same_nhw(md, zd) && same_nhw(ed, zd), fn, "muvar / eps / z n, h, w mismatch");
  VAE2_REQUIRE(idx32_ok(zd), fn, kTooLarge);
  int64_t total = act_elems(zd);
  unsigned nb = reduce_blocks(total);
  hipStream_t s = as_stream(stream);
  VAE2_LAUNCH(reparam_kl_kernel, dim3(nb), dim3(256), 0, s, muvar, to_act(md), eps,
                     to_act(ed), z, to_act(zd), prior, ws, FastDiv((uint32_t)zd->c));
  int rc = check_launch(fn);
  if (rc) return rc;
  VAE2_LAUNCH(finish_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, (int)nb,
                     scale, kl_out, accumulate);
  return check_launch(fn);
}

int vae2_reparam_kl_bwd(const float* muvar, const vae2_act* md,
                        const float* eps, const vae2_act* ed, const float* dz,
                        const vae2_act* dzd, const float* gkl, float scale,
                        float* dmuvar, const vae2_act* dmd, void* stream) {
  const char* fn = "vae2_reparam_kl_bwd";
  VAE2_REQUIRE(muvar && eps && dmuvar && act_ok(md) && act_ok(ed) && act_ok(dmd), fn,
               "bad arguments");
  VAE2_REQUIRE(!dz || act_ok(dzd), fn, "bad dz descriptor");
  VAE2_REQUIRE(md->c == 2 * ed->c, fn, "channel mismatch");
  VAE2_REQUIRE(same_nhw(md, ed), fn, "muvar / eps n, h, w mismatch");
  VAE2_REQUIRE(same_shape(dmd, md), fn, "dmuvar shape mismatch");
  VAE2_REQUIRE(!dz || same_shape(dzd, ed), fn, "dz shape mismatch");
  VAE2_REQUIRE(idx32_ok(ed), fn, kTooLarge);
  int64_t total = act_elems(ed);
  Act dza = dz ? to_act(dzd) : to_act(ed);
  VAE2_LAUNCH(reparam_kl_bwd_kernel, dim3(ew_blocks(total)), dim3(256), 0,
                     as_stream(stream), muvar, to_act(md), eps, to_act(ed), dz, dza, gkl, scale,
                     dmuvar, to_act(dmd), FastDiv((uint32_t)ed->c));
  return check_launch(fn);
}

int vae2_weighted_sum(int n, const float* const* terms, const float* lambdas,
                      float* total, void* stream) {
  const char* fn = "vae2_weighted_sum";
  VAE2_REQUIRE(n >= 1 && n <= 8 && terms && lambdas && total, fn, "bad arguments");
  WSum w{};
  w.n = n;
  for (int i = 0; i < n; ++i) {
    VAE2_REQUIRE(terms[i], fn, "null term");
    w.t[i] = terms[i];
    w.l[i] = lambdas[i];
  }
  VAE2_LAUNCH(weighted_sum_kernel, dim3(1), dim3(64), 0, as_stream(stream), w, total);
  return check_launch(fn);
}

int vae2_nonfinite_check(const float* x, int64_t n, int32_t* flag,
                         void* stream) {
  const char* fn = "vae2_nonfinite_check";
  VAE2_REQUIRE(x && flag && n >= 0, fn, "bad arguments");
  if (n == 0) return 0;
  VAE2_LAUNCH(nonfinite_kernel, dim3(ew_blocks(n, 256, 1024)), dim3(256), 0,
                     as_stream(stream), x, n, flag);
  return check_launch(fn);
}

int vae2_adam_step(float* p, const float* g, float* m, float* v, int64_t n,
                   float lr, float beta1, float beta2, float eps,
                   float weight_decay, int64_t step, void* stream) {
  const char* fn = "vae2_adam_step";
  VAE2_REQUIRE(p && g && m && v && n >= 0 && step >= 1, fn, "bad arguments");
  if (n == 0) return 0;
  double bc1 = 1.0 - pow((double)beta1, (double)step);
  double bc2 = 1.0 - pow((double)beta2, (double)step);
  float lr_corr = (float)((double)lr / bc1);
  float bc2s = (float)sqrt(bc2);
  VAE2_LAUNCH(adam_kernel, dim3(ew_blocks(n, 256, 4096)), dim3(256), 0,
                     as_stream(stream), p, g, m, v, n, lr_corr, beta1, beta2, eps,
                     weight_decay, bc2s);
  return check_launch(fn);
}

int vae2_adam_coeffs(double* state, float beta1, float beta2, float* coeffs,
                     void* stream) {
  const char* fn = "vae2_adam_coeffs";
  VAE2_REQUIRE(state && coeffs, fn, "null pointer");
  VAE2_LAUNCH(adam_coeffs_kernel, dim3(1), dim3(1), 0, as_stream(stream), state, beta1,
                     beta2, coeffs);
  return check_launch(fn);
}

int vae2_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n,
                       const float* coeffs, float beta1, float beta2, float eps,
                       float weight_decay, void* stream) {
  const char* fn = "vae2_adam_step_dev";
  VAE2_REQUIRE(p && g && m && v && coeffs && n >= 0, fn, "bad arguments");
  if (n == 0) return 0;
  VAE2_LAUNCH(adam_dev_kernel<false>, dim3(ew_blocks(n, 256, 4096)), dim3(256), 0,
              as_stream(stream), p, g, m, v, n, coeffs, (const float*)nullptr, beta1, beta2, eps,
              weight_decay);
  return check_launch(fn);
}

int vae2_adam_step_dev_clip(float* p, const float* g, float* m, float* v, int64_t n,
                            const float* coeffs, const float* clip, float beta1, float beta2,
                            float eps, float weight_decay, void* stream) {
  const char* fn = "vae2_adam_step_dev_clip";
  VAE2_REQUIRE(p && g && m && v && coeffs && clip && n >= 0, fn, "bad arguments");
  if (n == 0) return 0;
  VAE2_LAUNCH(adam_dev_kernel<true>, dim3(ew_blocks(n, 256, 4096)), dim3(256), 0,
              as_stream(stream), p, g, m, v, n, coeffs, clip, beta1, beta2, eps, weight_decay);
  return check_launch(fn);
}

int vae2_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum,
                  float dampening, float weight_decay, int nesterov, int first_step,
                  void* stream) {
  const char* fn = "vae2_sgd_step";
  VAE2_REQUIRE(p && g && n >= 0, fn, "bad arguments");
  const char* err = sgd_args_error(momentum, dampening, weight_decay, nesterov);
  VAE2_REQUIRE(!err, fn, err);
  VAE2_REQUIRE(buf || momentum == 0.f, fn, "momentum needs a momentum buffer");
  const SgdCoef c{lr, (float)(1.0 - (double)dampening), first_step ? 1.f : 0.f};
  return sgd_launch<false>(fn, p, g, buf, n, nullptr, nullptr, c, momentum, weight_decay,
                           nesterov, stream);
}

int vae2_sgd_coeffs(double* state, float momentum, float dampening, int nesterov,
                    float* coeffs, void* stream) {
  const char* fn = "vae2_sgd_coeffs";
  VAE2_REQUIRE(state && coeffs, fn, "null pointer");
  const char* err = sgd_args_error(momentum, dampening, 0.f, nesterov);
  VAE2_REQUIRE(!err, fn, err);
  VAE2_LAUNCH(sgd_coeffs_kernel, dim3(1), dim3(1), 0, as_stream(stream), state, dampening,
              coeffs);
  return check_launch(fn);
}

int vae2_sgd_step_dev(float* p, const float* g, float* buf, int64_t n, const float* coeffs,
                      float momentum, float weight_decay, int nesterov, void* stream) {
  const char* fn = "vae2_sgd_step_dev";
  VAE2_REQUIRE(p && g && coeffs && n >= 0, fn, "bad arguments");
  const char* err = sgd_args_error(momentum, 0.f, weight_decay, nesterov);
  VAE2_REQUIRE(!err, fn, err);
  VAE2_REQUIRE(buf || momentum == 0.f, fn, "momentum needs a momentum buffer");
  return sgd_launch<false>(fn, p, g, buf, n, coeffs, nullptr, SgdCoef{0.f, 1.f, 0.f}, momentum,
                           weight_decay, nesterov, stream);
}

int vae2_sgd_step_dev_clip(float* p, const float* g, float* buf, int64_t n, const float* coeffs,
                           const float* clip, float momentum, float weight_decay, int nesterov,
                           void* stream) {
  const char* fn = "vae2_sgd_step_dev_clip";
  VAE2_REQUIRE(p && g && coeffs && clip && n >= 0, fn, "bad arguments");
  const char* err = sgd_args_error(momentum, 0.f, weight_decay, nesterov);
  VAE2_REQUIRE(!err, fn, err);
  VAE2_REQUIRE(buf || momentum == 0.f, fn, "momentum needs a momentum buffer");
  return sgd_launch<true>(fn, p, g, buf, n, coeffs, clip, SgdCoef{0.f, 1.f, 0.f}, momentum,
                          weight_decay, nesterov, stream);
}

int vae2_ema_coeffs(double* state, float decay, float* coeffs, void* stream) {
  const char* fn = "vae2_ema_coeffs";
  VAE2_REQUIRE(state && coeffs, fn, "null pointer");
  const char* err = ema_decay_error(decay);
  VAE2_REQUIRE(!err, fn, err);
  VAE2_LAUNCH(ema_coeffs_kernel, dim3(1), dim3(1), 0, as_stream(stream), state, decay, coeffs);
  return check_launch(fn);
}

int vae2_ema_update_dev(float* ema, const float* p, int64_t n, const float* coeffs,
                        void* stream) {
  const char* fn = "vae2_ema_update_dev";
  VAE2_REQUIRE(ema && p && coeffs && n >= 0, fn, "bad arguments");
  VAE2_REQUIRE(ema != p, fn, "ema and p must be different buffers");
  return ema_launch(fn, ema, p, n, coeffs, EmaCoef{0.f, 0.f}, stream);
}

int vae2_ema_update(float* ema, const float* p, int64_t n, float decay, int first,
                    void* stream) {
  const char* fn = "vae2_ema_update";
  VAE2_REQUIRE(ema && p && n >= 0, fn, "bad arguments");
  VAE2_REQUIRE(ema != p, fn, "ema and p must be different buffers");
  const char* err = ema_decay_error(decay);
  VAE2_REQUIRE(!err, fn, err);
  const EmaCoef c{(float)(1.0 - (double)decay), first ? 1.f : 0.f};
  return ema_launch(fn, ema, p, n, nullptr, c, stream);
}

int64_t vae2_grad_norm_ws_size(int64_t n) { return norm_blocks(n); }

int vae2_grad_sumsq(const float* g, int64_t n, double* partials, void* stream) {
  const char* fn = "vae2_grad_sumsq";
  VAE2_REQUIRE(g && partials && n >= 0, fn, "bad arguments");
  const int64_t nq = ((uintptr_t)g & 15) == 0 ? n / 4 : 0;
  VAE2_LAUNCH(grad_sumsq_kernel, dim3(norm_blocks(n)), dim3(256), 0, as_stream(stream), g, n,
              nq, partials);
  return check_launch(fn);
}

int vae2_clip_coeffs(const double* partials, int64_t count, float max_norm, float* clip,
                     void* stream) {
  const char* fn = "vae2_clip_coeffs";
  VAE2_REQUIRE(partials && clip && count >= 1, fn, "bad arguments");
  const char* err = max_norm_error(max_norm);
  VAE2_REQUIRE(!err, fn, err);
  VAE2_LAUNCH(clip_coeffs_kernel, dim3(1), dim3(256), 0, as_stream(stream), partials, count,
              max_norm, clip);
  return check_launch(fn);
}

int vae2_scale_dev(float* x, int64_t n, const float* clip, void* stream) {
  const char* fn = "vae2_scale_dev";
  VAE2_REQUIRE(x && clip && n >= 0, fn, "bad arguments");
  if (n == 0) return 0;
  const int64_t nq = ((uintptr_t)x & 15) == 0 ? n / 4 : 0;
  VAE2_LAUNCH(clip_scale_kernel, dim3(ew_blocks(nq ? nq : n, 256, 4096)), dim3(256), 0,
              as_stream(stream), x, n, nq, clip);
  return check_launch(fn);
}

int vae2_scale(float* dst, const float* src, int64_t n, float scale,
               void* stream) {
  const char* fn = "vae2_scale";
  VAE2_REQUIRE(dst && src && n >= 0, fn, "bad arguments");
  if (n == 0) return 0;
  VAE2_LAUNCH(scale_kernel, dim3(ew_blocks(n, 256, 4096)), dim3(256), 0,
                     as_stream(stream), dst, src, n, scale);
  return check_launch(fn);
}

}  // extern "C"

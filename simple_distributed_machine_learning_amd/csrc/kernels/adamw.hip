// AdamW over the flat parameter buffer, with global-norm gradient clipping and the learning-rate schedule
// kept on the device:
//   grad_sqnorm     sum g^2 over the flat gradient buffer (fp32 or bf16) -> per-block fp32 partials
//   sqnorm_finish   the partials, summed in fixed order in fp64 -> one fp64 scalar
//   adamw_prep      (optionally the same finish, then) step counter + norm^2 -> the step's prep block
//                   {t, lr_t, c, lr_t / (1 - b1^t), 1 / sqrt(1 - b2^t), norm}; advances the counter
//   adamw / adamw_mixed   one pass over p, g, m, v (and the fp32 master weights): adamw_rule.h
// No atomics anywhere: two runs on the same input give the same bits. t and everything derived from it live on the
// device, so a captured step (hipGraph) replays with the right bias corrections, schedule and clip coefficient.
#include <hip/hip_runtime.h>

#include <hip/hip_bf16.h>

#include "adamw_rule.h"
#include "kernels.h"
#include "wave_ops.h"

namespace sdml {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float bf16_to_f32(unsigned short v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
  return __builtin_bit_cast(unsigned short, static_cast<__bf16>(f));
}

// ---- sum of squares -------------------------------------------------------------------------------------------------
// One 16-B vector (4 fp32 / 8 bf16) per lane per trip, grid-stride. The summation shape (what the tests' error bound
// counts): every thread folds its vectors, in trip order and element order, into ONE fp32 accumulator with an fma per
// element (g * g is exact inside the fma); then 6 fp32 additions across the wave (wave_ops.h sum64), then 3 across the
// block's 4 waves in wave order. The longest chain of fp32 roundings an element passes through is therefore
// trips * elements-per-vector + 9. The partials are summed in fp64 (sqnorm_finish / adamw_prep).
__device__ __forceinline__ float fold(float acc, f32x4 v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = __builtin_fmaf(v[j], v[j], acc);
  return acc;
}
__device__ __forceinline__ float fold(float acc, u16x8 v) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x = bf16_to_f32(v[j]);
    acc = __builtin_fmaf(x, x, acc);
  }
  return acc;
}

template <typename V>
__global__ void __launch_bounds__(256) grad_sqnorm_kernel(const V* __restrict__ g, int64_t nvec,
                                                          float* __restrict__ partials) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float acc = 0.f;
  // 4 loads in flight per lane; folded in trip order, so the sum is the plain loop's
  for (; i + 3 * stride < nvec; i += 4 * stride) {
    const V a = g[i], b = g[i + stride], c = g[i + 2 * stride], d = g[i + 3 * stride];
    acc = fold(fold(fold(fold(acc, a), b), c), d);
  }
  for (; i < nvec; i += stride) acc = fold(acc, g[i]);
  acc = wv::sum64(acc);
  __shared__ float ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// the partials in fp64, fixed order: thread t takes t, t + 256, ...; then a tree over the block. All threads return
// the total.
__device__ __forceinline__ double sum_partials(const float* __restrict__ partials, int n, double* sh) {
  double s = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) s += (double)partials[j];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

__global__ void __launch_bounds__(256) sqnorm_finish_kernel(const float* __restrict__ partials, int n,
                                                            double* __restrict__ out) {
  __shared__ double sh[256];
  const double total = sum_partials(partials, n, sh);
  if (threadIdx.x == 0) *out = total;
}

// partials != nullptr: finish the sum first (and store it in norm2); else norm2 holds the total (a cross-rank sum
// happened in between) or is nullptr (clipping off). One thread does the step's scalar math in double.
__global__ void __launch_bounds__(256) adamw_prep_kernel(const float* __restrict__ partials, int nparts,
                                                         double* __restrict__ norm2, int64_t* __restrict__ step_ctr,
                                                         float* __restrict__ prep, AdamwSchedule s) {
  __shared__ double sh[256];
  double n2 = 0.0;
  if (partials != nullptr) {
    n2 = sum_partials(partials, nparts, sh);
    if (threadIdx.x == 0 && norm2 != nullptr) *norm2 = n2;
  } else if (norm2 != nullptr) {
    n2 = *norm2;
  }
  if (threadIdx.x != 0) return;
  const int64_t ti = *step_ctr + 1;
  const double t = (double)ti;
  double lr = s.lr;
  if (ti <= s.warmup) {
    lr = s.lr * t / (double)s.warmup;
  } else if (s.cosine && s.decay_steps > s.warmup) {
    const double prog = fmin(1.0, (t - (double)s.warmup) / (double)(s.decay_steps - s.warmup));
    lr = s.min_lr + 0.5 * (s.lr - s.min_lr) * (1.0 + cos(M_PI * prog));
  }
  double c = 1.0, norm = 0.0;
  if (s.max_norm > 0.0) {
    norm = sqrt(n2);
    c = fmin(1.0, s.max_norm / (norm + 1e-6));  // a NaN norm gives a NaN c: it propagates, as in torch
    if (norm != norm) c = norm;
  }
  prep[ADAMW_T] = (float)t;
  prep[ADAMW_LR] = (float)lr;
  prep[ADAMW_CLIP] = (float)c;
  prep[ADAMW_STEP] = (float)(lr / (1.0 - pow(s.b1, t)));
  prep[ADAMW_RBC2] = (float)(1.0 / sqrt(1.0 - pow(s.b2, t)));
  prep[ADAMW_NORM] = (float)norm;
  prep[6] = 0.f;
  prep[7] = 0.f;
  *step_ctr = ti;
}

__device__ __forceinline__ AdamwRule load_rule(const float* __restrict__ prep, const AdamwHyper& h) {
  return AdamwRule{h, prep[ADAMW_LR], prep[ADAMW_CLIP], prep[ADAMW_STEP], prep[ADAMW_RBC2]};
}

// ---- the update -----------------------------------------------------------------------------------------------------
// decay: one byte per 64-element granule of the flat buffer (1: the granule belongs to a decayed parameter). Flat
// offsets are padded to 64 elements, so a granule never spans two parameters, and a lane's 4 (8) elements never
// span two granules.
__global__ void __launch_bounds__(256) adamw_kernel(float* __restrict__ p, float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    const unsigned char* __restrict__ decay,
                                                    const float* __restrict__ prep, int64_t n4, AdamwHyper h,
                                                    int zero_grad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const AdamwRule rule = load_rule(prep, h);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
    f32x4 mv = reinterpret_cast<const f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<const f32x4*>(v)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    const bool dec = decay[i >> 4] != 0;
    if (zero_grad) reinterpret_cast<f32x4*>(g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    adamw_update4(pv, mv, vv, gv, dec, rule);
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
  }
}

// bf16 weights and gradients, fp32 master / m / v: 8 elements per lane, every stream moves 16 B per access
// (as sgd_mixed_kernel); p = bf16(master), round to nearest even (the hardware cvt).
__global__ void __launch_bounds__(256) adamw_mixed_kernel(float* __restrict__ master, unsigned short* __restrict__ p,
                                                          unsigned short* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v,
                                                          const unsigned char* __restrict__ decay,
                                                          const float* __restrict__ prep, int64_t n8, AdamwHyper h,
                                                          int zero_grad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const AdamwRule rule = load_rule(prep, h);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    f32x4 pv[2], mv[2], vv[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      pv[h] = reinterpret_cast<const f32x4*>(master)[2 * i + h];
      mv[h] = reinterpret_cast<const f32x4*>(m)[2 * i + h];
      vv[h] = reinterpret_cast<const f32x4*>(v)[2 * i + h];
    }
    const u16x8 gr = reinterpret_cast<const u16x8*>(g)[i];
    const bool dec = decay[i >> 3] != 0;
    if (zero_grad) reinterpret_cast<u16x8*>(g)[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    u16x8 po;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 gv = {bf16_to_f32(gr[4 * h]), bf16_to_f32(gr[4 * h + 1]), bf16_to_f32(gr[4 * h + 2]),
                        bf16_to_f32(gr[4 * h + 3])};
      adamw_update4(pv[h], mv[h], vv[h], gv, dec, rule);
      reinterpret_cast<f32x4*>(master)[2 * i + h] = pv[h];
      reinterpret_cast<f32x4*>(m)[2 * i + h] = mv[h];
      reinterpret_cast<f32x4*>(v)[2 * i + h] = vv[h];
#pragma unroll
      for (int e = 0; e < 4; ++e) po[4 * h + e] = f32_to_bf16(pv[h][e]);
    }
    reinterpret_cast<u16x8*>(p)[i] = po;
  }
}

// grids are capped at 2048 blocks (8 resident blocks of 256 threads on each of the 256 CUs); the rest is the loop
int64_t grid_for(int64_t nvec, int64_t cap) {
  int64_t blocks = (nvec + 255) / 256;
  if (blocks > cap) blocks = cap;
  return blocks < 1 ? 1 : blocks;
}

AdamwHyper hyper(double b1, double b2, double eps, double wd) {
  return AdamwHyper{(float)b1, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)eps, (float)wd};
}

}  // namespace

int grad_sqnorm_blocks(int64_t n, bool bf16) {
  return (int)grid_for(n / (bf16 ? 8 : 4), kGradSqnormMaxBlocks);
}

int grad_sqnorm_partials(const void* g, int64_t n, bool bf16, float* partials, hipStream_t stream) {
  const int64_t nvec = n / (bf16 ? 8 : 4);
  const int blocks = grad_sqnorm_blocks(n, bf16);
  if (bf16)
    hipLaunchKernelGGL(grad_sqnorm_kernel<u16x8>, dim3((unsigned)blocks), dim3(256), 0, stream,
                       static_cast<const u16x8*>(g), nvec, partials);
  else
    hipLaunchKernelGGL(grad_sqnorm_kernel<f32x4>, dim3((unsigned)blocks), dim3(256), 0, stream,
                       static_cast<const f32x4*>(g), nvec, partials);
  return blocks;
}

void grad_sqnorm_finish(const float* partials, int nparts, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(sqnorm_finish_kernel, dim3(1), dim3(256), 0, stream, partials, nparts, out);
}

void adamw_prep(const float* partials, int nparts, double* norm2, int64_t* step_ctr, float* prep,
                const AdamwSchedule& sched, hipStream_t stream) {
  hipLaunchKernelGGL(adamw_prep_kernel, dim3(1), dim3(256), 0, stream, partials, nparts, norm2, step_ctr, prep, sched);
}

void adamw(float* p, float* g, float* m, float* v, const unsigned char* decay, const float* prep, int64_t n, double b1,
           double b2, double eps, double wd, bool zero_grad, hipStream_t stream) {
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)grid_for(n4, 2048)), dim3(256), 0, stream, p, g, m, v, decay, prep,
                     n4, hyper(b1, b2, eps, wd), zero_grad ? 1 : 0);
}

void adamw_mixed(float* master, void* p_bf16, void* g_bf16, float* m, float* v, const unsigned char* decay,
                 const float* prep, int64_t n, double b1, double b2, double eps, double wd, bool zero_grad,
                 hipStream_t stream) {
  const int64_t n8 = n / 8;
  hipLaunchKernelGGL(adamw_mixed_kernel, dim3((unsigned)grid_for(n8, 2048)), dim3(256), 0, stream, master,
                     static_cast<unsigned short*>(p_bf16), static_cast<unsigned short*>(g_bf16), m, v, decay, prep, n8,
                     hyper(b1, b2, eps, wd), zero_grad ? 1 : 0);
}

}  // namespace sdml

// torch.optim.AdamW's update for 4 consecutive parameters, shared by the fp32 kernel and the mixed-precision
// (bf16 weights, fp32 master) kernel of adamw.hip. For step t >= 1, c the step's clip coefficient:
//   g = c g;  p = p (1 - lr_t wd_e);  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;
//   p = p - (lr_t / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// Everything that depends on t (lr_t, the bias corrections, c) comes from the device prep block that
// adamw_prep writes each step (AdamwPrep below), so a captured step replays with fresh values.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace sdml {

typedef float adamw_f32x4 __attribute__((ext_vector_type(4)));

// the prep block's layout (kAdamwPrepFloats = 8 floats, kernels.h): written by adamw_prep_kernel, read once per
// thread by the update kernels
enum AdamwPrepSlot {
  ADAMW_T = 0,       // the step t this block is for (exact in fp32 up to 2^24 steps; the int64 counter is the truth)
  ADAMW_LR = 1,      // lr_t (schedule)
  ADAMW_CLIP = 2,    // c = min(1, max_norm / (norm + 1e-6)); 1 with clipping off
  ADAMW_STEP = 3,    // lr_t / (1 - b1^t)
  ADAMW_RBC2 = 4,    // 1 / sqrt(1 - b2^t)
  ADAMW_NORM = 5,    // the global gradient norm (0 with clipping off: it is not computed then)
};

// host constants; a1 = 1 - b1 and a2 = 1 - b2 are formed in double on the host and then rounded (1.f - 0.9f is off
// by 2.4e-7 relative, which would show in m)
struct AdamwHyper {
  float b1, a1, b2, a2, eps, wd;
};

struct AdamwRule {
  AdamwHyper h;
  float lr, c, step, rbc2;  // from the prep block
};

// pv / mv / vv: the 4 parameters (fp32 weights or master weights) and their moments, g the raw gradients;
// decay: whether these elements belong to a decayed parameter. Updates pv / mv / vv in place.
// Every multiply-add is an explicit fma and contraction is off (as in sgd_rule.h), so both kernels that inline
// this produce the same bits from the same inputs. sqrtf and / are the correctly rounded ones (no fast-math).
__device__ __forceinline__ void adamw_update4(adamw_f32x4& pv, adamw_f32x4& mv, adamw_f32x4& vv, adamw_f32x4 g,
                                              bool decay, const AdamwRule& r) {
#pragma clang fp contract(off)
  const float keep = decay ? __builtin_fmaf(-r.lr, r.h.wd, 1.f) : 1.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float gj = r.c * g[j];
    const float p = pv[j] * keep;
    const float m = __builtin_fmaf(r.h.b1, mv[j], r.h.a1 * gj);
    const float v = __builtin_fmaf(r.h.b2, vv[j], (r.h.a2 * gj) * gj);
    const float denom = sqrtf(v) * r.rbc2 + r.h.eps;
    pv[j] = __builtin_fmaf(-r.step, m / denom, p);
    mv[j] = m;
    vv[j] = v;
  }
}

}  // namespace sdml

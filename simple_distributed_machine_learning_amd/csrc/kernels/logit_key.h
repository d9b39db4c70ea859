// The bf16 logit helpers that the sampler (sample.hip) and the beam step (beam.hip) share: one copy of the
// order-preserving key, so both rank logits the same way.
#pragma once

#include <hip/hip_runtime.h>

namespace sdml {

typedef unsigned short u16;

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float(((unsigned)v) << 16); }

// order-preserving 16-bit key of a bf16 bit pattern (larger value <-> larger key); -0 -> the key of +0
__device__ __forceinline__ unsigned key16(u16 b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (unsigned)(u16)~b : (unsigned)b | 0x8000u;
}
__device__ __forceinline__ bool is_nan_bf16(u16 b) { return (b & 0x7FFFu) > 0x7F80u; }

}  // namespace sdml

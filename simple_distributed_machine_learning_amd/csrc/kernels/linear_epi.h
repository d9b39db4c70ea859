// The epilogue of the decode projections (linear_decode.hip, linear_rows.hip): none, bias, bias + GELU on one fp32
// sum; U = bf16(acc + b), y = bf16(gelu(U)), the unfused pair's bits (gelu.h). One copy, so both kernels round alike.
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "gelu.h"
#include "kernels.h"

namespace sdml {

__device__ __forceinline__ float epi_bf2f(unsigned short v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ unsigned short epi_f2bf(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<unsigned short*>(&h);
}

// epi: EPI_STORE, EPI_BIAS, EPI_BIAS_GELU; bias [N] bf16 bit patterns (not read by EPI_STORE)
__device__ __forceinline__ unsigned short linear_epilogue(float acc, const unsigned short* bias, int n, int epi) {
  if (epi == EPI_STORE) return epi_f2bf(acc);
  const unsigned short u = epi_f2bf(acc + epi_bf2f(bias[n]));
  return epi == EPI_BIAS ? u : epi_f2bf(gelu_f(epi_bf2f(u)));
}

}  // namespace sdml

// The fp8 KV-cache row format on the device (ops/decode.py kv_quantize is the definition): a row of 64 channels is 64
// OCP e4m3 bytes and one int8 exponent e, value = e4m3(byte) * 2^e. e is the smallest integer with amax * 2^-e <= 448
// (amax = f 2^x, f in [1, 2): x - 8 if f <= 1.75, else x - 7), clamped to [-120, 120], 0 for an all-zero row, so the
// scaled row peaks in (224, 448]: e4m3's top binade, never beyond it. The scale is a power of two, so x * 2^-e is
// exact and the convert's round-to-nearest-even is the format's only rounding; e4m3 * 2^e is exact in fp32.
//
// Four lanes (a DPP quad) hold a row, 16 channels each: 32 B of bf16 or 16 B of e4m3 per lane. kv_quantize.hip
// (prefill) and attention_decode_fp8.hip (the new token's row) share quantize_quad, so both write the same bytes.
#pragma once

#include <hip/hip_runtime.h>

#include "wave_ops.h"

namespace sdml {
namespace kv_fp8 {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kExpMin = -120, kExpMax = 120;

// 2^e for e in [-126, 127], from the exponent field
__device__ __forceinline__ float pow2(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }

// this lane's 16 bf16 channels (two 16-byte pieces) as fp32
__device__ __forceinline__ void widen_bf16(const u32x4& a, const u32x4& b, float (&x)[16]) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    x[2 * w] = __uint_as_float(a[w] << 16);
    x[2 * w + 1] = __uint_as_float(a[w] & 0xffff0000u);
    x[8 + 2 * w] = __uint_as_float(b[w] << 16);
    x[8 + 2 * w + 1] = __uint_as_float(b[w] & 0xffff0000u);
  }
}

// this lane's 16 e4m3 bytes as fp32 (exact): eight v_cvt_pk_f32_fp8
__device__ __forceinline__ void widen_fp8(const u32x4& q, float (&x)[16]) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[w], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[w], true);
    x[4 * w] = lo[0], x[4 * w + 1] = lo[1], x[4 * w + 2] = hi[0], x[4 * w + 3] = hi[1];
  }
}

// The row's exponent from its amax (>= 0, the bits of a bf16 value): the float's own exponent and mantissa fields, no
// log2. A subnormal or zero amax has exponent field 0 and lands on the lower clamp; zero is then set to 0.
__device__ __forceinline__ int row_exponent(float amax) {
  const unsigned bits = __float_as_uint(amax);
  int e = (int)(bits >> 23) - 127 - ((bits & 0x7fffffu) <= 0x600000u ? 8 : 7);
  e = min(max(e, kExpMin), kExpMax);
  return amax == 0.f ? 0 : e;
}

// Quantise the row that this lane's quad holds (x: the lane's 16 channels): the quad's amax by two DPP steps, the
// exponent, eight v_cvt_pk_fp8_f32. q: the lane's 16 bytes; returns e (the same in the quad's four lanes). All four
// lanes of the quad must be active.
__device__ __forceinline__ int quantize_quad(const float (&x)[16], u32x4& q) {
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) a = fmaxf(a, fabsf(x[i]));
  a = fmaxf(a, wv::dpp<wv::XOR1>(a));
  a = fmaxf(a, wv::dpp<wv::XOR2>(a));
  const int e = row_exponent(a);
  const float s = pow2(-e);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w] * s, x[4 * w + 1] * s, 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w + 2] * s, x[4 * w + 3] * s, v, true);
    q[w] = (unsigned)v;
  }
  return e;
}

}  // namespace kv_fp8
}  // namespace sdml

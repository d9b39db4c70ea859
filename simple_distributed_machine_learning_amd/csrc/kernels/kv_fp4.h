// The fp4 KV-cache row format on the device (ops/decode.py kv_quantize_fp4 is the definition): OCP microscaling e2m1.
// A row of 64 channels is two blocks of 32; a block is 16 bytes of nibbles and one int8 exponent e, value =
// e2m1(nibble) * 2^e. Channel 2 i of a block is the low nibble of its byte i and channel 2 i + 1 the high nibble: the
// order in which the packed converts take and give a byte. A nibble is sign, two exponent bits, one mantissa bit:
// magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}. e is the smallest integer with amax * 2^-e <= 6 (amax = f 2^x, f in
// [1, 2): x - 2 if f <= 1.5, else x - 1), clamped to [-120, 120], 0 for an all-zero block, so the scaled block peaks
// in (3, 6] and never saturates. The scale is a power of two, so x * 2^-e is exact and the convert's
// round-to-nearest-even onto the e2m1 grid is the format's only rounding; e2m1 * 2^e is exact in fp32.
//
// Two lanes hold a row, one block each: 64 B of bf16 or 16 B of nibbles per lane, and the block's amax is taken
// in-lane. kv_quantize_fp4.hip (prefill) and attention_decode_fp4.hip (the new token's row) share quantize_block, so
// both write the same bytes.
#pragma once

#include <hip/hip_runtime.h>

#include "kv_fp8.h"

namespace sdml {
namespace kv_fp4 {

using kv_fp8::f32x2;
using kv_fp8::kExpMax;
using kv_fp8::kExpMin;
using kv_fp8::pow2;
using kv_fp8::u32x4;

// this lane's block of 32 bf16 channels: four 16-byte pieces, two channels a word
struct Bf16Block {
  u32x4 p[4];
};
__device__ __forceinline__ Bf16Block load_block_bf16(const unsigned short* src) {
  Bf16Block r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.p[i] = *reinterpret_cast<const u32x4*>(src + 8 * i);
  return r;
}
// the two channels of a word as fp32
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// channels 8 w + 2 t, 8 w + 2 t + 1 of a block (byte t of its word w) as fp32, times `scale` (a power of two, of which
// the instruction takes the exponent field): one v_cvt_scalef32_pk_f32_fp4, exact
template <int T>
__device__ __forceinline__ f32x2 widen_fp4(unsigned word, float scale) {
  return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, scale, T);
}

// The block's exponent from the bits of its amax (sign cleared): the float's own exponent and mantissa fields, no
// log2. A subnormal or zero amax has exponent field 0 and lands on the lower clamp; zero is then set to 0.
__device__ __forceinline__ int block_exponent(unsigned amax_bits) {
  int e = (int)(amax_bits >> 23) - 127 - ((amax_bits & 0x7fffffu) <= 0x400000u ? 2 : 1);
  e = min(max(e, kExpMin), kExpMax);
  return amax_bits == 0u ? 0 : e;
}

// Quantise the block this lane holds: the amax over the magnitudes' bit patterns (an integer max, in-lane: no
// cross-lane step and no dependence on the denormal mode), the exponent, sixteen v_cvt_scalef32_pk_fp4_f32 on
// x * 2^-e with scale 1, a word's two channels to a byte. q: the block's 16 bytes; returns e.
__device__ __forceinline__ int quantize_block(const Bf16Block& x, u32x4& q) {
  unsigned a = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) a = max(a, max((x.p[i][w] << 16) & 0x7fffffffu, x.p[i][w] & 0x7fff0000u));
  const int e = block_exponent(a);
  const float s = pow2(-e);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u32x4 w = x.p[i];
    unsigned v = 0u;
    v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, bf16_lo(w[0]) * s, bf16_hi(w[0]) * s, 1.0f, 0);
    v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, bf16_lo(w[1]) * s, bf16_hi(w[1]) * s, 1.0f, 1);
    v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, bf16_lo(w[2]) * s, bf16_hi(w[2]) * s, 1.0f, 2);
    v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, bf16_lo(w[3]) * s, bf16_hi(w[3]) * s, 1.0f, 3);
    q[i] = v;
  }
  return e;
}

}  // namespace kv_fp4
}  // namespace sdml

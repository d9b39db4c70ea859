// The arithmetic of the decode-attention family (attention_decode.hip, attention_append.hip), bf16,
// head width 64: one query against one chunk of kAttnDecodeChunk keys held in a wave's VGPRs, the chunk's workspace
// slot, and the combine of a query's slots in chunk order. This is the one definition: "a query's bits are
// attention_decode's at its own key count" holds because the kernels call these lines, each keeping only its own
// address selection, liveness, cache write and query loop. (attention_fork.hip still carries a copy of chunk_query
// and combine_chunks, kept for speed, profiles/decode_chunk_ab.jsonl: a change here must be repeated there.)
//
// Lane l of the wave holds piece l & 7 (channels 8 (l & 7) ..) of the rows of row group l >> 3; its keys are
// c * CH + 8 i + (l >> 3), i = 0 .. RPL - 1. Scores, exp2, sums and the combine are fp32; the output is rounded to
// bf16 once. A slot is (m, l) in ws_ml[2 slot ..] and the 64 partial outputs in ws_o[64 slot ..].
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "wave_ops.h"

namespace sdml {
namespace attn_chunk {

typedef unsigned short u16;
typedef u16 u16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CH = kAttnDecodeChunk;  // keys per wave
constexpr int RPL = CH / 8;           // rows per lane (8 lanes hold one row)
constexpr float kLog2e = 1.4426950408889634f;
constexpr int ROR8 = 0x128;  // DPP row_ror:8: lane i <- lane i ^ 8 inside a row of 16

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ u16 f2bf(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<u16*>(&h);
}

// sum / max over the 8 row groups of a wave (lane bits 3..5); lanes that differ only in those bits hold the addends
__device__ __forceinline__ float sum_groups(float x) { return wv::sum_rows(x + wv::dpp<ROR8>(x)); }
__device__ __forceinline__ float max_groups(float x) { return wv::max_rows(fmaxf(x, wv::dpp<ROR8>(x))); }

// chunk_query's per-row hook where the caller has nothing to do between the rows
struct NoRowHook {
  __device__ __forceinline__ void operator()(int, int) const {}
};

// One query (qrow: this lane's 8 channels of it) against chunk c's rows in VGPRs: the chunk's max m, sum l and partial
// output o (this lane's 8 channels, every row group holding the same sums). Keys past `last` never reach the result:
// their scores and probabilities are selected away, not multiplied by zero (a chunk that is wholly live passes its own
// last key, so every select takes the live operand). m is finite: the caller runs only chunks with c * CH <= last.
// on_row(i, j) runs ahead of row i's score, j its key index: where attention_decode.hip writes the new token's cache
// row. No contraction: the products and sums are the ones written.
template <class OnRow>
__device__ __forceinline__ void chunk_query(const u16x8 (&kv)[RPL], const u16x8 (&vv)[RPL], const u16* qrow, int c,
                                            int last, float scale, int lane, float& m, float& l, float (&o)[8],
                                            OnRow on_row) {
#pragma clang fp contract(off)
  const int rg = lane >> 3;
  const u16x8 qv = *reinterpret_cast<const u16x8*>(qrow);
  float q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) q[e] = bf2f(qv[e]);

  const float sl2 = scale * kLog2e;
  float s[RPL];
  m = -INFINITY;
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg;
    on_row(i, j);
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) a = fmaf(q[e], bf2f(kv[i][e]), a);
    a += wv::dpp<wv::XOR1>(a);
    a += wv::dpp<wv::XOR2>(a);
    a += wv::dpp<wv::HALF_MIRROR>(a);  // the row's 8 lanes hold the same sum
    s[i] = j <= last ? a * sl2 : -INFINITY;
    m = fmaxf(m, s[i]);
  }
  m = max_groups(m);

  l = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg;
    const float pr = j <= last ? __builtin_amdgcn_exp2f(s[i] - m) : 0.f;
    l += pr;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaf(pr, bf2f(vv[i][e]), o[e]);
  }
  l = sum_groups(l);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = sum_groups(o[e]);
}

// chunk_query's result to its slot: o as two 16-byte stores by lanes 0..7, (m, l) by lane 0
__device__ __forceinline__ void store_slot(float* ws_ml, float* ws_o, int64_t slot, int lane, float m, float l,
                                           const float (&o)[8]) {
  if (lane < 8) {
    f32x4* dst = reinterpret_cast<f32x4*>(ws_o + slot * 64 + 8 * lane);
    dst[0] = f32x4{o[0], o[1], o[2], o[3]};
    dst[1] = f32x4{o[4], o[5], o[6], o[7]};
  }
  if (lane == 0) {
    ws_ml[slot * 2] = m;
    ws_ml[slot * 2 + 1] = l;
  }
}

// lane = channel: slots slot .. slot + nc - 1 of one query in chunk order; the bf16 bits of O / L
__device__ __forceinline__ u16 combine_chunks(const float* ws_ml, const float* ws_o, int64_t slot, int nc, int lane) {
  float M = -INFINITY;
  for (int c = 0; c < nc; ++c) M = fmaxf(M, ws_ml[(slot + c) * 2]);
  float L = 0.f, O = 0.f;
  for (int c = 0; c < nc; ++c) {
    const float w = __builtin_amdgcn_exp2f(ws_ml[(slot + c) * 2] - M);
    L = fmaf(ws_ml[(slot + c) * 2 + 1], w, L);
    O = fmaf(ws_o[(slot + c) * 64 + lane], w, O);
  }
  return f2bf(O / L);
}

}  // namespace attn_chunk
}  // namespace sdml

// Pieces shared by the head-width-64 MFMA attention kernels (attention.hip, attention_extend.hip): the bf16 helpers,
// the 32x32x16 MFMA, the swizzled 64-wide LDS tile image with its two read kinds, and a tile's trip from global memory
// through registers to LDS. The layout conventions are those of attention.hip's header comment.
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "mma_prims.h"

namespace sdml {
namespace attn_tile {

typedef __attribute__((ext_vector_type(4))) short bf16x4;

constexpr int HD = 64;  // head dim
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ u16 f2bf(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<u16*>(&h);
}
__device__ __forceinline__ short f2bfs(float f) { return (short)f2bf(f); }

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// v_exp_f32 directly (exp2f adds denormal range fix-ups we do not need: arguments are <= 0 or
// -inf, and flushing tiny probabilities to 0 is harmless)
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// pack accumulator registers 8s..8s+7 to a bf16 B/A fragment
__device__ __forceinline__ bf16x8 pack8(const f32x16& x, int s) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = f2bfs(x[8 * s + j]);
  return r;
}

// ---- swizzled tile image ----------------------------------------------------------------------
constexpr int TR = 64;  // rows per staged tile (KB keys or BQ queries)
__device__ __forceinline__ int swz(int r, int ch) {
  return r * HD + 8 * (ch ^ ((((r >> 1) & 1) << 2) | ((r >> 2) & 3)));
}
// row fragment (A/B operand with k = d): element j = X[row][16t + 8h + j]
__device__ __forceinline__ bf16x8 rowf(const u16* X, int row, int t, int h) {
  return *reinterpret_cast<const bf16x8*>(X + swz(row, 2 * t + h));
}
// transposed fragment in the accumulator k-order: element j = X[k0 + 8(j>>2) + 4h + (j&3)][c0 + (lane&31)]
// (k0 % 8 == 0, c0 % 32 == 0). Two ds_read_b64_tr_b16: each 16-lane group g reads rows
// k0 + 4(g>>1) + q (q = 0..3) at columns c0 + 16(g&1) + 0..15; lane 4q+p supplies row q, cols 4p..4p+3.
// Must run with all 64 lanes active.
__device__ __forceinline__ bf16x8 trf(const u16* X, int k0, int c0, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int R = k0 + 4 * (g >> 1) + q;
  const int col = c0 + 16 * (g & 1) + 4 * p;
  const s16x4 lo = ds_tr16(X + swz(R, col >> 3) + (col & 7));
  const s16x4 hi = ds_tr16(X + swz(R + 8, col >> 3) + (col & 7));
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}
// a tile of ROWS rows in registers (ROWS * 8 / NTH x 16 B per thread of an NTH-thread block) on its way from global
// memory to LDS
template <int ROWS, int NTH = 256>
struct TileRegs {
  u16x8 v[ROWS * 8 / NTH];
};
template <int ROWS, int NTH>
__device__ __forceinline__ void tile_load(TileRegs<ROWS, NTH>& t, const u16* G, long srow, int r0, int S) {
#pragma unroll
  for (int u = 0; u < ROWS * 8 / NTH; ++u) {
    const int idx = threadIdx.x + NTH * u, r = idx >> 3, ch = idx & 7;
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r0 + r < S) v = *reinterpret_cast<const u16x8*>(G + (long)(r0 + r) * srow + 8 * ch);
    t.v[u] = v;
  }
}
// rows past S re-read row S - 1 (unconditional loads, no exec-masked branches): only for consumers that mask those
// keys themselves (the forward's edge tiles set their scores to -inf, so their V rows meet P = 0)
template <int ROWS, int NTH>
__device__ __forceinline__ void tile_load_clamped(TileRegs<ROWS, NTH>& t, const u16* G, long srow, int r0, int S) {
#pragma unroll
  for (int u = 0; u < ROWS * 8 / NTH; ++u) {
    const int idx = threadIdx.x + NTH * u, r = idx >> 3, ch = idx & 7;
    t.v[u] = *reinterpret_cast<const u16x8*>(G + (long)min(r0 + r, S - 1) * srow + 8 * ch);
  }
}
template <int ROWS, int NTH>
__device__ __forceinline__ void tile_store(u16* L, const TileRegs<ROWS, NTH>& t) {
#pragma unroll
  for (int u = 0; u < ROWS * 8 / NTH; ++u) {
    const int idx = threadIdx.x + NTH * u, r = idx >> 3, ch = idx & 7;
    *reinterpret_cast<u16x8*>(L + swz(r, ch)) = t.v[u];
  }
}

// XCD-aware block order: the dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs, so
// the blocks of one (batch, head) - which all read the same K/V (or Q/dO) tiles - would land on 8
// different L2s. Logical block L = (id % 8) * (n / 8) + id / 8 keeps consecutive L (same (b, h)) on one
// XCD (bijective when n % 8 == 0; otherwise the plain order).
__device__ __forceinline__ int xcd_block(int id, int n) { return (n % 8 == 0) ? (id % 8) * (n / 8) + id / 8 : id; }

}  // namespace attn_tile
}  // namespace sdml

// Tile geometry, LDS images and fragment reads shared by the dense weight gradients, gW[M][N] += sum_t A[t][m] B[t][n]:
// gemm_bf16_wgrad.hip (bf16) and gemm_f16x2.hip (fp16 planes). F is the MFMA fragment type (bf16x8 or f16x8), Ops the
// operand policy of mma_prims.h.
//
// Both operands are k-major (the token index t is the row of A and B), so their tiles are copied into LDS exactly as
// they sit in memory and the MFMA fragments come out of the hardware transpose read (ds_read_b64_tr_b16): no transpose
// pass, no extra copy.
//   block 512 threads = 8 waves (4 x 2), tile 256 (m) x 128 (n), K-step 64, wave tile 64 x 64 (2 x 2 32x32x16 MFMAs,
//   16 per wave per K-step); one stage = 48 KiB = [A cols m0..+127 | A cols m0+128..+255 | B cols n0..+127], each a
//   [64 k][128 cols] image with the km_off chunk swizzle (conflict-free transposed reads and 16-B writes).
// Two main loops fill the stages. They, the DMA stage issue and the finish stay in the kernels of each file: moved
// into templates over a K-step source, the fp16-plane kernels compiled to different instruction streams.
//   staged (any T): register-staged double buffer through KmTile, fragments by trfrag.
//   LDS-DMA (T % 64 == 0, 16-B aligned operands; the default): a ring of 3 stages filled by glds16 with the km_off
//     swizzle on the per-lane source address, so the images are the same; fragments by read_substep (ds_tr16_asm)
//     with explicit lgkm_wait (mma_prims.h says why).
#pragma once

#include "mma_prims.h"

namespace sdml {

constexpr int WNT = 512, WBM = 256, WBN = 128, WBK = 64;
constexpr int IMG = WBK * 128;  // u16 per 128-column image

// fragment of the 32-column block at c0 of a [64][128] image, k-substep s: element j = X[16s + 8h + j][c0 + lane&31]
template <typename F>
__device__ __forceinline__ F trfrag(const u16* P, int c0, int s, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int k = 16 * s + 8 * (g >> 1) + q;
  const int col = c0 + 16 * (g & 1) + 4 * p;
  const s16x4 lo = ds_tr16(P + km_off(k, col >> 3) + (col & 7));
  const s16x4 hi = ds_tr16(P + km_off(k + 4, col >> 3) + (col & 7));
  return cat<F>(lo, hi);
}

// a COLS-wide k-major tile (64 k x COLS) in registers: COLS/8 chunks of 16 B per k-row
template <int COLS>
struct KmTile {
  static constexpr int CPR = COLS / 8;         // chunks per k-row
  static constexpr int NV = WBK * CPR / WNT;   // chunks per thread
  u16x8 v[NV];
  // clamped loads (rows past T / cols past the end re-read valid memory; zeroed in store)
  __device__ __forceinline__ void load(const u16* __restrict__ P, int ld, int cols, int c0, int k0, int T) {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int id = threadIdx.x + WNT * u;
      const int k = min(k0 + id / CPR, T - 1);
      const int c = min(c0 + 8 * (id % CPR), cols - 8);
      v[u] = *reinterpret_cast<const u16x8*>(P + (size_t)k * ld + c);
    }
  }
  // rows k0 + k >= klim are stored as zeros. ROWSUM: when `sum`, colsum[e] += the 8 staged values of this thread's
  // column chunk (every u of a thread has the same chunk index: WNT is a multiple of CPR)
  template <bool ROWSUM, typename Ops>
  __device__ __forceinline__ void store(u16* L, int k0, int klim, bool sum, float (&colsum)[8]) const {
    const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int id = threadIdx.x + WNT * u;
      const int k = id / CPR, ch = id % CPR;
      const u16x8 val = (k0 + k < klim) ? v[u] : z;
      *reinterpret_cast<u16x8*>(L + (ch >> 4) * IMG + km_off(k, ch & 15)) = val;
      if constexpr (ROWSUM) {
        if (sum) {
#pragma unroll
          for (int e = 0; e < 8; ++e) colsum[e] += Ops::widen(val[e]);
        }
      }
    }
  }
};

// the 8 half-fragments of one 16-deep substep: A (2 x lo/hi) then B (2 x lo/hi), as trfrag reads them
__device__ __forceinline__ void read_substep(const u16* L, int wm, int wn, int s, int lane, s16x4 (&f)[8]) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, pp = i & 3;
  const int k = 16 * s + 8 * (g >> 1) + q;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const u16* P = x < 2 ? L + (wm >> 1) * IMG : L + 2 * IMG;
    const int c0 = x < 2 ? (wm & 1) * 64 + 32 * x : wn * 64 + 32 * (x - 2);
    const int col = c0 + 16 * (g & 1) + 4 * pp;
    f[2 * x] = ds_tr16_asm(P + km_off(k, col >> 3) + (col & 7));
    f[2 * x + 1] = ds_tr16_asm(P + km_off(k + 4, col >> 3) + (col & 7));
  }
}

}  // namespace sdml

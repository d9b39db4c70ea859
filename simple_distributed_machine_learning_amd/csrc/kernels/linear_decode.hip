// Decode-time projections: y[M][N] = x[M][K] . W[N][K]^T (+ bias) (then tanh-GELU), bf16 in and out, fp32
// accumulation, 1 <= M <= 64 (models/gpt2.py decode_step). W is the Linear's own [out][in] storage.
//
// The work is streaming W once: at M = 16 a 768 -> 768 projection reads 1.2 MB of weights for 19 MFLOP. gemm_bf16's
// 256 x 256 tiles put such a shape on 3 workgroups; here a wave owns 16 output columns and a slice of K.
//
//   * W goes straight to VGPRs, 32 contiguous bytes per lane and 64-wide k block: lane l reads W[n0 + (l & 15)]
//     [64 t + 16 (l >> 4) .. + 15], so the four lane groups of a row read one whole 128-B line. The two 16-B halves
//     feed the two v_mfma_f32_16x16x32_bf16 of the block; the k order inside the block is permuted, identically in
//     the x fragments (element j of group g in MFMA s is k = 64 t + 16 g + 8 s + j), which leaves the sum unchanged.
//   * x is tiny and L2-resident: its fragments are read from global with the same map, rows padded to 16 by clamping
//     the row index (a padded row only feeds padded outputs, which are not stored); M > 16 loops over 16-row groups
//     against the same W fragments.
//   * Decomposition: N / 16 column tiles x KS grid-level K splits, up to 4 waves per workgroup over the split's k
//     blocks. KS is the smallest divisor of K / 64 that gives at least kLinearDecodeMinBlocks workgroups (a function
//     of N and K only). The waves' accumulators are summed through LDS in wave order; with KS > 1 the fp32 partials
//     go to a workspace and a second launch sums them in split order. No atomics: the same bits on every run, and a
//     row's result does not depend on M.
//   * One-launch form (tickets): the splits of a column tile store their slabs write-through, each draws a ticket
//     on the tile's counter, and the block that draws the last one acquires at agent scope and runs the reduce for
//     its tile (handoff.h): the same additions in the same order, so the same bits, without the second launch. Nothing
//     waits on a counter.
//   * Epilogues: none, bias, bias + GELU; U = bf16(acc + b), y = bf16(gelu(U)), the unfused pair's bits (gelu.h).
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "gelu.h"
#include "handoff.h"
#include "kernels.h"

namespace sdml {
namespace {

typedef unsigned short u16;
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MAXW = 4;  // waves per workgroup

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ u16 f2bf(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<u16*>(&h);
}

struct LdParams {
  const u16* x;
  const u16* w;
  const u16* bias;
  u16* y;
  float* ws;  // [KS][M][N] fp32 (KS > 1)
  int* tickets;  // [N / 16] arrival counters of the one-launch form, zero between launches (nullptr: two launches)
  int M, N, K, ldx, ldw;
  int KS, kb_per_split, waves;
  int epi;  // EPI_STORE, EPI_BIAS, EPI_BIAS_GELU
};

__device__ __forceinline__ u16 epilogue(float acc, const u16* bias, int n, int epi) {
  if (epi == EPI_STORE) return f2bf(acc);
  const u16 u = f2bf(acc + bf2f(bias[n]));
  return epi == EPI_BIAS ? u : f2bf(gelu_f(bf2f(u)));
}

// grid (N / 16, KS); block 64 * waves. MG = ceil(M / 16) row groups. TK: the one-launch form (KS > 1 and tickets).
template <int MG, bool TK>
__global__ void __launch_bounds__(64 * MAXW) linear_decode_kernel(LdParams p) {
  __shared__ float red[MAXW][MG * 16][17];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  // this wave's k blocks inside the split: a contiguous range, the first `rem` waves take one more
  const int per = p.kb_per_split / p.waves, rem = p.kb_per_split % p.waves;
  const int kb0 = blockIdx.y * p.kb_per_split + wave * per + min(wave, rem);
  const int nkb = per + (wave < rem ? 1 : 0);

  const u16* wp = p.w + (int64_t)(n0 + r) * p.ldw + 16 * g;
  const u16* xp[MG];
#pragma unroll
  for (int mg = 0; mg < MG; ++mg) xp[mg] = p.x + (int64_t)min(mg * 16 + r, p.M - 1) * p.ldx + 16 * g;

  f32x4 acc[MG];
#pragma unroll
  for (int mg = 0; mg < MG; ++mg) acc[mg] = f32x4{0.f, 0.f, 0.f, 0.f};

  // (every GPT-2 shape gives a wave 1 to 3 k blocks; the loads in flight come from the 8 waves per SIMD. Issuing four
  // blocks' loads per trip with the surplus ones clamped was measured slower: lm_head 25.0 against 22.0 us)
#pragma unroll 4
  for (int t = 0; t < nkb; ++t) {
    const int k = (kb0 + t) * 64;
    const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(wp + k);
    const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(wp + k + 8);
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) {
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(xp[mg] + k);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(xp[mg] + k + 8);
      acc[mg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[mg], 0, 0, 0);
      acc[mg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[mg], 0, 0, 0);
    }
  }

  // accumulator element i of lane l: row 4 (l >> 4) + i of the group, column l & 15
#pragma unroll
  for (int mg = 0; mg < MG; ++mg)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][mg * 16 + 4 * g + i][r] = acc[mg][i];
  __syncthreads();

  for (int e = threadIdx.x; e < MG * 16 * 16; e += blockDim.x) {
    const int m = e >> 4, n = e & 15;
    if (m >= p.M) continue;
    float s = red[0][m][n];
    for (int w = 1; w < p.waves; ++w) s += red[w][m][n];
    if (TK)
      handoff::st_sc1(&p.ws[((int64_t)blockIdx.y * p.M + m) * p.N + n0 + n], s);
    else if (p.KS > 1)
      p.ws[((int64_t)blockIdx.y * p.M + m) * p.N + n0 + n] = s;
    else
      p.y[(int64_t)m * p.N + n0 + n] = epilogue(s, p.bias, n0 + n, p.epi);
  }
  if constexpr (TK) {
    // the slab went out write-through; draw a ticket on the tile (handoff.h). red is free after the barrier inside
    // draw_ticket and carries "this workgroup drew the last one" to every wave.
    const int t = handoff::draw_ticket(p.tickets + blockIdx.x);
    handoff::acquire_partials(t == p.KS - 1);
    if (threadIdx.x == 0) red[0][0][0] = t == p.KS - 1 ? 1.f : 0.f;
    __syncthreads();
    if (red[0][0][0] == 0.f) return;
    // linear_decode_reduce_kernel's sum for this tile, the splits in split order; 2 columns per thread
    const int64_t slab = (int64_t)p.M * p.N;
    for (int e = threadIdx.x; e < MG * 16 * 8; e += blockDim.x) {
      const int m = e >> 3, n = n0 + 2 * (e & 7);
      if (m >= p.M) continue;
      const int64_t i = (int64_t)m * p.N + n;
      float s0, s1;
      handoff::ld_sc1_x2(p.ws + i, s0, s1);
      for (int k = 1; k < p.KS; k += 4) {  // (four slabs' loads in flight: each is a round trip past the L1)
        float a0[4], a1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) handoff::ld_sc1_x2(p.ws + slab * min(k + j, p.KS - 1) + i, a0[j], a1[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < p.KS) s0 += a0[j], s1 += a1[j];
      }
      typedef u16 u16x2 __attribute__((ext_vector_type(2)));
      u16x2 o;
      o[0] = epilogue(s0, p.bias, n, p.epi), o[1] = epilogue(s1, p.bias, n + 1, p.epi);
      *reinterpret_cast<u16x2*>(p.y + i) = o;
    }
    if (threadIdx.x == 0) handoff::reset_ticket(p.tickets + blockIdx.x);
  }
}

// y = epilogue(sum over the splits in split order); 4 columns per thread
__global__ void __launch_bounds__(256) linear_decode_reduce_kernel(LdParams p) {
  const int64_t i4 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)p.M * p.N;
  if (i4 * 4 >= total) return;
  const f32x4* ws = reinterpret_cast<const f32x4*>(p.ws);
  f32x4 s = ws[i4];
  for (int k = 1; k < p.KS; ++k) s += ws[(total / 4) * k + i4];
  const int n = (int)((i4 * 4) % p.N);
  typedef u16 u16x4 __attribute__((ext_vector_type(4)));
  u16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = epilogue(s[e], p.bias, n + e, p.epi);
  reinterpret_cast<u16x4*>(p.y)[i4] = o;
}

}  // namespace

bool linear_decode_supported(int M, int N, int K, int ldx, int ldw) {
  return M >= 1 && M <= kLinearDecodeMaxM && N >= 16 && N % 16 == 0 && K >= 64 && K % 64 == 0 && ldx >= K &&
         ldw >= K && ldx % 8 == 0 && ldw % 8 == 0;
}

int linear_decode_splits(int N, int K) {
  const int tiles = N / 16, nkb = K / 64;
  for (int ks = 1; ks <= nkb; ++ks)
    if (nkb % ks == 0 && tiles * ks >= kLinearDecodeMinBlocks) return ks;
  return nkb;
}

size_t linear_decode_workspace_floats(int M, int N, int K) {
  const int ks = linear_decode_splits(N, K);
  return ks > 1 ? (size_t)ks * M * N : 0;
}

void linear_decode_bf16(const void* x, const void* w, const void* bias, void* y, float* ws, int M, int N, int K,
                        int ldx, int ldw, int epi, hipStream_t stream, int* tickets) {
  LdParams p;
  p.x = static_cast<const u16*>(x);
  p.w = static_cast<const u16*>(w);
  p.bias = static_cast<const u16*>(bias);
  p.y = static_cast<u16*>(y);
  p.ws = ws;
  p.M = M, p.N = N, p.K = K, p.ldx = ldx, p.ldw = ldw;
  p.KS = linear_decode_splits(N, K);
  p.kb_per_split = (K / 64) / p.KS;
  p.waves = p.kb_per_split < MAXW ? p.kb_per_split : MAXW;
  p.epi = epi;
  p.tickets = p.KS > 1 ? tickets : nullptr;
  const dim3 grid(N / 16, p.KS), block(64 * p.waves);
  if (p.tickets != nullptr) {  // one launch: the last split to arrive at a tile reduces it
    switch ((M + 15) / 16) {
      case 1: hipLaunchKernelGGL((linear_decode_kernel<1, true>), grid, block, 0, stream, p); break;
      case 2: hipLaunchKernelGGL((linear_decode_kernel<2, true>), grid, block, 0, stream, p); break;
      case 3: hipLaunchKernelGGL((linear_decode_kernel<3, true>), grid, block, 0, stream, p); break;
      default: hipLaunchKernelGGL((linear_decode_kernel<4, true>), grid, block, 0, stream, p); break;
    }
    return;
  }
  switch ((M + 15) / 16) {
    case 1: hipLaunchKernelGGL((linear_decode_kernel<1, false>), grid, block, 0, stream, p); break;
    case 2: hipLaunchKernelGGL((linear_decode_kernel<2, false>), grid, block, 0, stream, p); break;
    case 3: hipLaunchKernelGGL((linear_decode_kernel<3, false>), grid, block, 0, stream, p); break;
    default: hipLaunchKernelGGL((linear_decode_kernel<4, false>), grid, block, 0, stream, p); break;
  }
  if (p.KS > 1) {
    const int64_t n4 = (int64_t)M * N / 4;
    hipLaunchKernelGGL(linear_decode_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, p);
  }
}

}  // namespace sdml

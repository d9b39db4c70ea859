// Decode-time projections for 65 to 512 rows: y[M][N] = x[M][K] . W[N][K]^T (+ bias) (then tanh-GELU), bf16 in and
// out, fp32 accumulation, W in the Linear's own [out][in] storage. linear_decode.hip stops at 64 rows (it re-reads x
// from L2 for every 16 output columns) and gemm_bf16.hip's 256 x 256 tiles put a 768 -> 768 projection of 65..256 rows
// on 3 workgroups; this kernel serves the rows in between, and a row keeps linear_decode's bits.
//
//   * Bit contract. For a (row, column) linear_decode's result is a function of N and K only: KS =
//     linear_decode_splits(N, K) grid splits of kb_per_split 64-wide k blocks; inside a split min(kb_per_split, 4)
//     contiguous k ranges ("chains", the first `rem` one block longer), each one chain of v_mfma_f32_16x16x32_bf16 onto
//     a zero accumulator with element j of lane group g in MFMA s of block t at k = 64 t + 16 g + 8 s + j; the chains
//     summed in fp32 in chain order, the splits in split order, then linear_epi.h. All of that is kept here. What is
//     free is who runs a chain: one wave runs the split's chains one after the other and adds them in registers.
//   * Tile. A workgroup of NW waves (4, 2 or 1) owns a panel of 64 rows x 16 NW columns x one grid split of K. Wave w
//     owns 16 columns and runs every W fragment against the panel's four 16-row groups (linear_decode's reuse at
//     M = 64). NW drops to 2 or 1 at launch where 64-column tiles would leave CUs idle (or N % 64 != 0).
//   * x through LDS. The panel's slice of x, [64 rows][64 k] per k block (8 KiB), is staged by LDS-DMA
//     (lds_dma.h bdma16_asm), SB = 2, 4, 6 or 8 k blocks per stage (at most 64 KiB: two workgroups per CU), a template
//     parameter so that a stage is straight-line code; every GPT-2 projection is one stage, the lm_head two of 6.
//     16-B chunk c of row r lies at chunk c ^ rk_swz(r) (mma_prims.h; the swizzle is on the DMA's per-lane source
//     address), so the A fragment is one conflict-free ds_read_b128 per lane. Rows past M are clamped to row M - 1
//     on the source side (they only feed outputs that are not stored), and the buffer resource ends with row M - 1.
//     x is read from L2 once per column tile, N / 64 times, not N / 16 times.
//   * W to VGPRs with linear_decode's map: lane l reads 32 B of W[n0 + (l & 15)] at k = 64 t + 16 (l >> 4). A stage's
//     W loads (up to 8 blocks, 64 VGPRs) are all issued before its DMA, so a wave has up to 16 KiB of W and 16 KiB of
//     x in flight and waits once per stage; the 8 MFMAs of a k block could not cover a load anyway. The loads are
//     unconditional (a short last stage re-reads its last block): under a branch per block the compiler drained
//     vmcnt before each block's pair, one round trip after the other.
//   * Grid. panels x column tiles x KS workgroups, XCD-remapped (tile_order.h) with the panel index fastest, then the
//     column tile: the panels that share W lines and the column tiles that share an x slice meet in one XCD's L2.
//   * KS > 1: fp32 partials to the [KS][M][N] workspace, then linear_decode's reduce launch
//     (linear_splits_reduce_bf16). No atomics and no tickets: the same bits on every run.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lds_dma.h"
#include "linear_epi.h"
#include "mma_prims.h"
#include "tile_order.h"

namespace sdml {
namespace {

constexpr int PM = 64;               // rows of a panel
constexpr int BLK_BYTES = PM * 128;  // a panel's k block in LDS: [64 rows][64 k] bf16
constexpr int MAX_SB = 8;            // k blocks of an LDS stage
constexpr int MAX_CHAINS = 4;        // linear_decode's waves per workgroup: the chains of a split

struct LrParams {
  const u16* x;
  const u16* w;
  const u16* bias;
  u16* y;
  float* ws;  // [KS][M][N] fp32 (KS > 1)
  int M, N, K, ldx, ldw;
  int KS, kb_per_split, chains;
  int panels, ctiles;
  int epi;  // EPI_STORE, EPI_BIAS, EPI_BIAS_GELU
};

// grid panels * ctiles * KS; block 64 * NW; dynamic LDS SB * BLK_BYTES
template <int NW, int SB>
__global__ void __launch_bounds__(64 * NW) linear_rows_kernel(LrParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int panel = wg % p.panels;
  wg /= p.panels;
  const int ct = wg % p.ctiles, split = wg / p.ctiles;
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = panel * PM, n0 = (ct * NW + wave) * 16;
  const int kb0 = split * p.kb_per_split;

  // DMA pieces of a k block: 8 x 1 KiB, rows 8 q .. 8 q + 7; wave w issues q = w + NW u. Lane l of a piece writes
  // chunk l & 7 of row 8 q + (l >> 3), so it fetches chunk (l & 7) ^ rk_swz(row) of that row of x.
  constexpr int NU = 8 / NW;
  const dma_i32x4 rx = dma_rsrc4(p.x, (unsigned)(((size_t)(p.M - 1) * p.ldx + p.K) * 2));
  unsigned voff[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int lr = 8 * (wave + NW * u) + (lane >> 3);
    const int c = (lane & 7) ^ rk_swz(lr);
    voff[u] = (unsigned)(((size_t)min(m0 + lr, p.M - 1) * p.ldx + 8 * c) * 2);
  }
  // A fragment of row group mg, MFMA s: row 16 mg + r (rk_swz(16 mg + r) = rk_swz(r)), chunk 2 g + s
  const int abase = r * 128;
  const int xo0 = 16 * ((2 * g) ^ rk_swz(r)), xo1 = 16 * ((2 * g + 1) ^ rk_swz(r));
  const u16* wp = p.w + (int64_t)(n0 + r) * p.ldw + (int64_t)kb0 * 64 + 16 * g;

  f32x4 acc[4], tot[4];
#pragma unroll
  for (int mg = 0; mg < 4; ++mg) acc[mg] = tot[mg] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the chains of the split: chain c is linear_decode's wave c, per blocks and one more for the first rem
  const int per = p.kb_per_split / p.chains, rem = p.kb_per_split % p.chains;
  int chain = 0, chain_end = per + (rem > 0 ? 1 : 0);

  for (int j0 = 0; j0 < p.kb_per_split; j0 += SB) {
    const int nb = min(SB, p.kb_per_split - j0);
    bf16x8 wf[SB][2];
#pragma unroll
    for (int b = 0; b < SB; ++b) {
      const u16* wb = wp + min(j0 + b, p.kb_per_split - 1) * 64;
      wf[b][0] = *reinterpret_cast<const bf16x8*>(wb);
      wf[b][1] = *reinterpret_cast<const bf16x8*>(wb + 8);
    }
#pragma unroll
    for (int b = 0; b < SB; ++b)
      if (b < nb) {
#pragma unroll
        for (int u = 0; u < NU; ++u)
          bdma16_asm(rx, voff[u], (unsigned)(kb0 + j0 + b) * 128u, smem + b * BLK_BYTES + 1024 * (wave + NW * u));
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces landed (and its W fragments)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

#pragma unroll
    for (int b = 0; b < SB; ++b)
      if (b < nb) {
        if (j0 + b == chain_end) {  // the chain is complete: tot = chain 0, then tot += chain c in chain order
#pragma unroll
          for (int mg = 0; mg < 4; ++mg) {
            tot[mg] = chain == 0 ? acc[mg] : tot[mg] + acc[mg];
            acc[mg] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
          ++chain;
          chain_end += per + (chain < rem ? 1 : 0);
        }
        const unsigned char* blk = smem + b * BLK_BYTES + abase;
#pragma unroll
        for (int mg = 0; mg < 4; ++mg) {
          const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(blk + mg * 2048 + xo0);
          const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(blk + mg * 2048 + xo1);
          acc[mg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wf[b][0], acc[mg], 0, 0, 0);
          acc[mg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wf[b][1], acc[mg], 0, 0, 0);
        }
      }
    if (j0 + SB < p.kb_per_split) {  // every wave has read the stage before the next one's DMA overwrites it
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
  }
#pragma unroll
  for (int mg = 0; mg < 4; ++mg) tot[mg] = chain == 0 ? acc[mg] : tot[mg] + acc[mg];

  // accumulator element i of lane l: row 4 (l >> 4) + i of the group, column l & 15
  const int n = n0 + r;
  if (p.KS > 1) {
    float* ws = p.ws + (int64_t)split * p.M * p.N + n;
#pragma unroll
    for (int mg = 0; mg < 4; ++mg)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + 16 * mg + 4 * g + i;
        if (m < p.M) ws[(int64_t)m * p.N] = tot[mg][i];
      }
    return;
  }
  const u16 bn = p.epi == EPI_STORE ? (u16)0 : p.bias[n];  // the lane's one column: read once, not per element
#pragma unroll
  for (int mg = 0; mg < 4; ++mg)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + 16 * mg + 4 * g + i;
      if (m < p.M) p.y[(int64_t)m * p.N + n] = linear_epilogue(tot[mg][i], &bn, 0, p.epi);
    }
}

}  // namespace

bool linear_rows_supported(int M, int N, int K, int ldx, int ldw) {
  return M > kLinearDecodeMaxM && M <= kLinearRowsMaxM && N >= 16 && N % 16 == 0 && K >= 64 && K % 64 == 0 &&
         ldx >= K && ldw >= K && ldx % 8 == 0 && ldw % 8 == 0 && (int64_t)M * ldx * 2 < (int64_t)1 << 31;
}

size_t linear_rows_workspace_floats(int M, int N, int K) {
  const int ks = linear_decode_splits(N, K);
  return ks > 1 ? (size_t)ks * M * N : 0;
}

void linear_rows_bf16(const void* x, const void* w, const void* bias, void* y, float* ws, int M, int N, int K, int ldx,
                      int ldw, int epi, hipStream_t stream) {
  LrParams p;
  p.x = static_cast<const u16*>(x);
  p.w = static_cast<const u16*>(w);
  p.bias = static_cast<const u16*>(bias);
  p.y = static_cast<u16*>(y);
  p.ws = ws;
  p.M = M, p.N = N, p.K = K, p.ldx = ldx, p.ldw = ldw;
  p.KS = linear_decode_splits(N, K);
  p.kb_per_split = (K / 64) / p.KS;
  p.chains = p.kb_per_split < MAX_CHAINS ? p.kb_per_split : MAX_CHAINS;
  p.panels = (M + PM - 1) / PM;
  p.epi = epi;
  // 64 columns per workgroup, or 32 or 16 where that leaves CUs without one (a launch-time choice: not the chains')
  int nw = 4;
  while (nw > 1 && (N % (16 * nw) != 0 || (int64_t)(N / (16 * nw)) * p.KS * p.panels < kLinearDecodeMinBlocks)) nw >>= 1;
  p.ctiles = N / (16 * nw);
  // (stages of at most 4 k blocks, 4 workgroups per CU, for grids of several rounds: lm_head 102 against 110 us at
  // M = 512, but c_attn 20.2 against 17.9 and c_fc 22.6 against 20.8, and the step's sum 1034 against 999 us)
  const int stages = (p.kb_per_split + MAX_SB - 1) / MAX_SB;
  const int sb = ((p.kb_per_split + stages - 1) / stages + 1) & ~1;  // even stages: 2, 4, 6 or 8 k blocks
  const dim3 grid((unsigned)(p.panels * p.ctiles * p.KS)), block(64 * nw);
  const size_t lds = (size_t)sb * BLK_BYTES;
#define SDML_LR_LAUNCH(NW_)                                                                                  \
  switch (sb) {                                                                                              \
    case 2: hipLaunchKernelGGL((linear_rows_kernel<NW_, 2>), grid, block, lds, stream, p); break;            \
    case 4: hipLaunchKernelGGL((linear_rows_kernel<NW_, 4>), grid, block, lds, stream, p); break;            \
    case 6: hipLaunchKernelGGL((linear_rows_kernel<NW_, 6>), grid, block, lds, stream, p); break;            \
    default: hipLaunchKernelGGL((linear_rows_kernel<NW_, 8>), grid, block, lds, stream, p); break;           \
  }
  switch (nw) {
    case 4: SDML_LR_LAUNCH(4) break;
    case 2: SDML_LR_LAUNCH(2) break;
    default: SDML_LR_LAUNCH(1) break;
  }
#undef SDML_LR_LAUNCH
  if (p.KS > 1) linear_splits_reduce_bf16(ws, bias, y, M, N, p.KS, epi, stream);
}

}  // namespace sdml

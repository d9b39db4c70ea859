// Beam search's step on the device (parallel/generate.py num_beams=K; ops/reference.py beam_step is the definition).
// R = B K rows, row b K + j beam j of prompt b; per row a cumulative score (fp32), a finished flag and a length.
//
// beam_rows_kernel, one workgroup of 1024 threads per row:
//   * the row's logits, bf16 [ld] with columns < vocab taking part, are read ONCE in 16-byte pieces (8 logits) into
//     registers, piece p 1024 + tid in slot p of thread tid, and every later pass works on those registers. A NaN and a
//     column >= vocab become the pattern 0xFFFF on the way in, which no pass counts. 8 slots: vocab <= 65536. (A step
//     has at most 64 rows for 256 CUs, so occupancy sets no limit: docs/TUNING_NOTES.md "Beam step".)
//   * m = max_v z_v and S = sum_v exp(z_v - m) in fp32: a thread sums its slots in slot order, a wave reduces on DPP /
//     permlane swaps (wave_ops.h), the 16 wave sums are added in wave order. lse = m + log(S). The order is fixed, so
//     the bits are too; docs/NUMERICS.md "Beam step" bounds the error.
//   * the K-th largest logit VALUE, exactly, on the sampler's order-preserving 16-bit key by its two 256-bin counting
//     passes (high byte, then low byte inside the boundary bin; integer LDS atomics). Only logits >= t0 are counted,
//     t0 = the K-th largest of the 16 wave maxima: K different logits are >= t0, so the K-th largest value is too, and
//     a smaller logit cannot move the bin in which the count from the top reaches K. That leaves a few dozen atomics
//     where the unfiltered pass has 50,257 on a handful of bins.
//   * the winners in (logit descending, token ascending) order: every logit above the threshold, then the lowest token
//     ids at the threshold. Where the threshold bin holds exactly the tokens still needed they are simply taken; where
//     it holds more (ties at the boundary) the needed ones are found lowest id first, one block-wide minimum each. The
//     <= K (key, token) pairs are ranked by one wave and written in order with
//       c = score[r] + (float(z_v) - lse)        one fp32 subtract, then one fp32 add, not contracted
//     (-inf for a logit of -inf). A finished row writes its single candidate (pad, score[r]) and reads no logits.
// beam_merge_kernel, one wave per prompt (one workgroup, the waves take the prompts in turn): K <= 8 makes the <= 64
//   candidates one per lane, lane j K + i candidate i of row j. A lane's rank is the number of lanes that beat it under
//   (c descending, parent ascending, rank-in-row ascending), integer compares on an order-preserving key of c read
//   from the other lanes with v_readlane; lanes of rank < K write the prompt's new rows. all_done is one fixed-order
//   pass over the waves' flags after a barrier, as lookup_step_kernel's.
// beam_gather_kv_kernel: the suffix caches follow their parents, every layer's k and v in one launch, 16 bytes per
//   lane, vector stores. beam_backtrack_kernel: one thread per row walks the parents from the last step down.
#include <climits>
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "logit_key.h"
#include "wave_ops.h"

namespace sdml {
namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BT = 1024;            // threads per row
constexpr int kWaves = BT / 64;     // 16
constexpr int kSlots = 8;           // 16-byte pieces per thread
constexpr u16 kDead = 0xFFFFu;      // a NaN or a column >= vocab (a negative NaN pattern: never a logit's value)
static_assert(kSlots * 8 * BT == kBeamMaxVocab, "the row must fit the workgroup's registers");

// slot s, element e of the thread's logits (s, e compile-time after unrolling)
#define BEAM_EL(w, s, e) ((u16)((w)[s][(e) >> 1] >> (((e)&1) * 16)))
#define BEAM_FOR_EACH(s, e)              \
  _Pragma("unroll") for (int s = 0; s < kSlots; ++s) \
  _Pragma("unroll") for (int e = 0; e < 8; ++e)

// Between two passes: the compiler may carry nothing it derived from the row (64 floats, 64 keys) across this point,
// so a pass streams through the 32 registers that hold the row. Without it the kernel spills 71 of its 128 registers
// to scratch, with it 8 (in the exp pass).
__device__ __forceinline__ void pin_row(unsigned (&w)[kSlots][4]) {
#pragma unroll
  for (int s = 0; s < kSlots; ++s)
#pragma unroll
    for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(w[s][q]));
}

__device__ __forceinline__ u16 key16_to_bf16(unsigned k) { return (k & 0x8000u) ? (u16)(k & 0x7FFFu) : (u16)~k; }

// order-preserving 32-bit key of an fp32 score (NaN never reaches here; -0 -> +0); always > 0
__device__ __forceinline__ unsigned key32(float c) {
  unsigned u = c == 0.f ? 0u : __float_as_uint(c);
  return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}

// The bin of hist[256] in which the count from the top, starting at `above`, reaches K, by wave 0: lane l holds bins
// 4 l .. 4 l + 3. Writes sh[0] = the bin (UINT_MAX: the whole histogram holds fewer than K) and sh[1] = the count in
// the bins above it.
__device__ __forceinline__ void find_bin(const unsigned* hist, unsigned above, unsigned K, unsigned* sh) {
  const int lane = threadIdx.x;  // (wave 0)
  unsigned c[4], s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = hist[4 * lane + i], s += c[i];
  unsigned suf = s;  // inclusive suffix sum over the lanes: lanes above hold the higher bins
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = __shfl_down(suf, off);
    if (lane + off < 64) suf += o;
  }
  unsigned abv = above + suf - s;
  if (abv < K && abv + s >= K) {  // exactly one lane
    int b = 3;
    for (; b > 0; --b) {
      if (abv + c[b] >= K) break;
      abv += c[b];
    }
    sh[0] = 4 * lane + b, sh[1] = abv;
  }
  if (lane == 0 && above + suf < K) sh[0] = UINT_MAX, sh[1] = above + suf;
}

__global__ void __launch_bounds__(BT) beam_rows_kernel(BeamStepArgs p) {
  __shared__ float red_f[kWaves];
  __shared__ int red_i[kWaves];
  __shared__ unsigned hist[256];
  __shared__ unsigned sh[2], sh_n;
  __shared__ unsigned list_key[kBeamMaxK];
  __shared__ int list_tok[kBeamMaxK];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned K = (unsigned)p.K;
  int* ct = p.cand_tok + row * kBeamMaxK;
  float* cs = p.cand_score + row * kBeamMaxK;
  const float sc = p.score[row];
  if (p.fin[row]) {  // (uniform over the block)
    if (tid < kBeamMaxK) ct[tid] = tid == 0 ? (int)p.pad : -1, cs[tid] = tid == 0 ? sc : -INFINITY;
    return;
  }
  // ---- the row, once
  const u32x4* lg = reinterpret_cast<const u32x4*>(static_cast<const u16*>(p.logits) + (int64_t)row * p.ld);
  const int npieces = (p.vocab + 7) >> 3;  // (<= ld / 8: the host checks ld % 8 == 0 and vocab <= ld)
  unsigned w[kSlots][4];
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int piece = s * BT + tid;
    u32x4 v = {~0u, ~0u, ~0u, ~0u};
    if (piece < npieces) v = lg[piece];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      u16 lo = (u16)(v[q] & 0xFFFFu), hi = (u16)(v[q] >> 16);
      const int col = piece * 8 + q * 2;
      if (col >= p.vocab || is_nan_bf16(lo)) lo = kDead;
      if (col + 1 >= p.vocab || is_nan_bf16(hi)) hi = kDead;
      w[s][q] = (unsigned)lo | ((unsigned)hi << 16);
    }
  }
  if (tid == 0) sh_n = 0;
  // ---- m, and t0 = the K-th largest wave maximum
  float mx = -INFINITY;
  pin_row(w);
  BEAM_FOR_EACH(s, e) {
    const u16 b = BEAM_EL(w, s, e);
    if (b != kDead) mx = fmaxf(mx, bf2f(b));
  }
  mx = wv::max64(mx);
  if (lane == 0) red_f[wave] = mx;
  __syncthreads();
  float wm[kWaves], m = -INFINITY, t0 = -INFINITY;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) wm[i] = red_f[i], m = fmaxf(m, wm[i]);
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    unsigned rank = 0;
#pragma unroll
    for (int j = 0; j < kWaves; ++j) rank += (wm[j] > wm[i]) | ((wm[j] == wm[i]) & (j < i));
    if (rank == K - 1) t0 = wm[i];
  }
  __syncthreads();
  // ---- S and lse (a row without a finite logit: m0 = 0, S = 0, lse = -inf)
  const float m0 = m > -INFINITY ? m : 0.f;
  float sum = 0.f;
  pin_row(w);
  BEAM_FOR_EACH(s, e) {
    const u16 b = BEAM_EL(w, s, e);
    if (b != kDead) sum += expf(bf2f(b) - m0);
  }
  sum = wv::sum64(sum);
  if (lane == 0) red_f[wave] = sum;
  __syncthreads();
  float S = red_f[0];
#pragma unroll
  for (int i = 1; i < kWaves; ++i) S += red_f[i];
  const float lse = m0 + logf(S);
  // ---- the key of the K-th largest value: two counting passes over the logits >= t0
  unsigned hi = 0, above = 0, thr = 0, n_at = 0;
  bool few = false;  // fewer than K logits that are no NaN: all of them are candidates
  for (int pass = 0; pass < 2 && !few; ++pass) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    pin_row(w);
    BEAM_FOR_EACH(s, e) {
      const u16 b = BEAM_EL(w, s, e);
      if (b != kDead && bf2f(b) >= t0) {
        const unsigned k = key16(b);
        if (pass == 0)
          atomicAdd(&hist[k >> 8], 1u);
        else if ((k >> 8) == hi)
          atomicAdd(&hist[k & 255u], 1u);
      }
    }
    __syncthreads();
    if (wave == 0) find_bin(hist, above, K, sh);
    __syncthreads();
    if (sh[0] == UINT_MAX) {
      few = true;
    } else if (pass == 0) {
      hi = sh[0], above = sh[1];
    } else {
      thr = (hi << 8) | sh[0], above = sh[1], n_at = hist[sh[0]];
    }
    __syncthreads();
  }
  // ---- the winners: above the threshold, then the lowest ids at it
  const unsigned need = few ? 0 : K - above;  // tokens to take at the threshold, 1 .. n_at
  const bool take_all = n_at == need;
  pin_row(w);
  BEAM_FOR_EACH(s, e) {
    const u16 b = BEAM_EL(w, s, e);
    if (b != kDead && bf2f(b) >= t0) {
      const unsigned k = key16(b);
      if (k > thr || (k == thr && take_all && !few)) {
        const unsigned slot = atomicAdd(&sh_n, 1u);
        if (slot < (unsigned)kBeamMaxK) list_key[slot] = k, list_tok[slot] = ((s * BT + tid) << 3) + e;
      }
    }
  }
  if (!few && !take_all) {  // (uniform) ties at the boundary: `need` rounds of the lowest id above the last one taken
    int last = -1;
    for (unsigned r = 0; r < need; ++r) {
      int best = INT_MAX;
      pin_row(w);
      BEAM_FOR_EACH(s, e) {
        const u16 b = BEAM_EL(w, s, e);
        const int tok = ((s * BT + tid) << 3) + e;
        if (b != kDead && key16(b) == thr && tok > last) best = min(best, tok);
      }
      for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off));
      if (lane == 0) red_i[wave] = best;
      __syncthreads();
      last = red_i[0];
#pragma unroll
      for (int i = 1; i < kWaves; ++i) last = min(last, red_i[i]);
      if (tid == 0) list_key[above + r] = thr, list_tok[above + r] = last;
      __syncthreads();
    }
  }
  __syncthreads();
  // ---- rank the <= K pairs and write them in order
  if (tid < kBeamMaxK) {
    const unsigned n = few ? min(sh_n, K) : K;
    if ((unsigned)tid >= n) ct[tid] = -1, cs[tid] = -INFINITY;
    if ((unsigned)tid < n) {
      const unsigned k = list_key[tid];
      const int tok = list_tok[tid];
      int rank = 0;
      for (unsigned j = 0; j < n; ++j) rank += (list_key[j] > k) | ((list_key[j] == k) & (list_tok[j] < tok));
      const float z = bf2f(key16_to_bf16(k));
      float c = z == -INFINITY ? -INFINITY : __fadd_rn(sc, __fsub_rn(z, lse));
      if (!(c == c)) c = -INFINITY;
      ct[rank] = tok, cs[rank] = c;
    }
  }
}

constexpr int kMergeWaves = 16;

__global__ void __launch_bounds__(64 * kMergeWaves) beam_merge_kernel(BeamStepArgs p) {
  __shared__ int sh_alive[kMergeWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = p.K;
  int alive = 0;
  for (int b = wave; b < p.B; b += kMergeWaves) {  // (wave-uniform)
    const int j = lane / K, i = lane - j * K;
    const int prow = b * K + min(j, K - 1);
    int tok = -1;
    float c = -INFINITY;
    if (j < K) tok = p.cand_tok[prow * kBeamMaxK + i], c = p.cand_score[prow * kBeamMaxK + i];
    const bool valid = tok >= 0;
    const unsigned key = valid ? key32(c) : 0u;
    int rank = 0;
#pragma unroll
    for (int l = 0; l < 64; ++l) {
      const unsigned kl = (unsigned)__builtin_amdgcn_readlane((int)key, l);
      rank += (kl > key) | ((kl == key) & (l < lane));
    }
    if (rank < K) {
      const int r = b * K + rank;
      // (fewer than K candidates in all cannot happen with vocab >= K; such a row ends, finished, at -inf)
      const bool pf = valid ? p.fin[prow] != 0 : true;
      const int64_t t = valid ? (int64_t)tok : p.pad;
      const int fn = (pf || t == p.eos) ? 1 : 0;
      p.tok[r] = t;
      p.par[r] = valid ? j : 0;
      p.score_new[r] = valid ? c : -INFINITY;
      p.fin_new[r] = fn;
      p.glen_new[r] = p.glen[valid ? prow : b * K] + (pf ? 0 : 1);
      if (!fn) alive = 1;
    }
    alive = __any(alive);
  }
  if (lane == 0) sh_alive[wave] = alive;
  __syncthreads();
  if (threadIdx.x == 0) {
    int any = 0;
    for (int w = 0; w < kMergeWaves; ++w) any |= sh_alive[w];
    p.all_done[0] = any ? 0 : 1;
  }
}

__global__ void __launch_bounds__(256) beam_gather_kv_kernel(const u16* __restrict__ src, u16* __restrict__ dst,
                                                             const int* __restrict__ par, int R, int K, long row_elems,
                                                             long copy_pieces) {
  const int r = blockIdx.y, lk = blockIdx.z;
  const int pj = par[r];
  if (pj < 0 || pj >= K) return;
  const long from = (long)lk * R + (r / K) * K + pj, to = (long)lk * R + r;
  const u32x4* s = reinterpret_cast<const u32x4*>(src + from * row_elems);
  u32x4* d = reinterpret_cast<u32x4*>(dst + to * row_elems);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < copy_pieces; i += (long)gridDim.x * 256) d[i] = s[i];
}

__global__ void __launch_bounds__(64) beam_backtrack_kernel(const int64_t* __restrict__ tok_hist,
                                                            const int* __restrict__ par_hist,
                                                            const int* __restrict__ glen,
                                                            const int64_t* __restrict__ plen, int64_t* __restrict__ out,
                                                            long ld_out, int W, int R, int K, int steps, int64_t pad) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const int base = (r / K) * K, g = glen[r];
  const int64_t p0 = plen[r];
  int j = r - base;
  for (int t = steps - 1; t >= 0; --t) {
    if (j < 0 || j >= K) return;  // (a parent outside the prompt's rows: the histories are not the step's)
    const int64_t col = p0 + t;
    if (col >= 0 && col < W) out[(int64_t)r * ld_out + col] = t < g ? tok_hist[(int64_t)t * R + base + j] : pad;
    j = par_hist[(int64_t)t * R + base + j];
  }
}

}  // namespace

void beam_step_bf16(const BeamStepArgs& a, hipStream_t stream) {
  if (a.B <= 0) return;
  hipLaunchKernelGGL(beam_rows_kernel, dim3(a.B * a.K), dim3(BT), 0, stream, a);
  hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(64 * kMergeWaves), 0, stream, a);
}

void beam_gather_kv_bf16(const void* src, void* dst, const int* par, int LK, int R, int K, long row_elems,
                         long copy_elems, hipStream_t stream) {
  if (LK <= 0 || R <= 0 || copy_elems <= 0) return;
  const long pieces = copy_elems / 8;
  const int gx = (int)((pieces + 255) / 256 < 256 ? (pieces + 255) / 256 : 256);
  hipLaunchKernelGGL(beam_gather_kv_kernel, dim3(gx, R, LK), dim3(256), 0, stream, static_cast<const u16*>(src),
                     static_cast<u16*>(dst), par, R, K, row_elems, pieces);
}

void beam_backtrack(const int64_t* tok_hist, const int* par_hist, const int* glen, const int64_t* plen, int64_t* out,
                    long ld_out, int W, int R, int K, int steps, int64_t pad, hipStream_t stream) {
  if (R <= 0 || steps <= 0) return;
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3((R + 63) / 64), dim3(64), 0, stream, tok_hist, par_hist, glen, plen,
                     out, ld_out, W, R, K, steps, pad);
}

}  // namespace sdml

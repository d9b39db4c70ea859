// Generation's two small kernels (parallel/generate.py): the on-device sampler and the decode-time embedding.
//
// sample_logits: one workgroup per row of bf16 logits [B][ld]; only columns < vocab take part (the lm_head's padded
// columns hold zeros and must never win).
//   * temperature == 0 (inv_temp == 0 here): greedy, argmax with the lowest index on ties.
//   * top_k in 1 .. vocab - 1: the candidates are the tokens whose logit is >= the k-th largest logit VALUE (ties at
//     the boundary are all kept). bf16 has 65,536 bit patterns: two 256-bin histogram passes (high byte, then low
//     byte inside the boundary bin) over an order-preserving 16-bit key find that value exactly. -0 is keyed as +0.
//   * temperature > 0: Gumbel-max over the candidates, token = argmax_v (l_v * (1 / T) + g_v), lowest index on ties,
//     g_v = -log(-log u_v) with the accurate logf (-log u reaches 1.2e-7, where an absolute-error log is useless),
//     u_v = ((word >> 9) + 0.5) * 2^-23: exact in fp32, inside [2^-24, 1 - 2^-24]. One fp32 multiply and one add (no
//     contraction), so the torch twin (ops/reference.py) differs by the two logs' last ulps only.
//   * The word is dropout_hash.h's counter hash at site DROP_SITE_SAMPLE, layer 0, head 0:
//       rkey = drop_row_key(drop_site_key(seed, 5 << 16), sample0 + row, 0);  word = drop_word(rkey, position, v)
//     with the vocabulary id in the b4 slot (one word per candidate) and position = the index of the token being
//     drawn. No step counter: a token is a function of (seed, sample, position, logits) alone.
//   * rows_per_sample (default 1): row r is sample sample0 + r / rows_per_sample, so several positions of one sample
//     may be drawn in one launch (the verify step of prompt-lookup speculation).
//   NaN logits never win a comparison. Integer LDS atomics build the histograms; no float atomics anywhere.
//
// sample_step: sample_logits' token with two additions in the same launch (the device code above is shared).
//   * top_p in (0, 1), temperature > 0: the candidates shrink to the nucleus {v in C_k : l_v >= theta}, theta = the
//     largest logit value x with sum{w_v : l_v >= x} >= top_p * sum{w_v}, w_v = exp((l_v - l_max) / T) over the top-k
//     candidates C_k. Ties at theta are all kept. theta comes from the same two histogram passes, the bins holding
//     64-bit fixed-point masses (top_p_mass below); integer sums are order-independent, so theta is the same bits on
//     every run. With top_p off the token is sample_logits' token.
//   * the step's bookkeeping by thread 0 of the row (plain stores): a row whose done flag is set emits the pad token
//     and touches nothing; else the token goes to out[row][pos[row]], gen_len[row] grows by one and done[row] is set
//     when the token is the eos (-1: none). pos outside [0, W) writes none of the three.
//
// embedding_at: out[b] = bf16(wte[tok[b]] + wpe[pos[b]]) for one token per sample at a per-sample position read on
// the device (the cache length), where embedding_fwd_bf16 hard-wires position = column.
#include <hip/hip_bf16.h>
#include <climits>
#include <hip/hip_runtime.h>

#include "dropout_hash.h"
#include "kernels.h"

namespace sdml {
namespace {

typedef unsigned short u16;
typedef u16 u16x4 __attribute__((ext_vector_type(4)));

constexpr int ST = 1024;  // sampler threads per row

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ u16 f2bf(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<u16*>(&h);
}

// order-preserving 16-bit key of a bf16 bit pattern (larger value <-> larger key); -0 -> the key of +0
__device__ __forceinline__ unsigned key16(u16 b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (unsigned)(u16)~b : (unsigned)b | 0x8000u;
}
__device__ __forceinline__ bool is_nan_bf16(u16 b) { return (b & 0x7FFFu) > 0x7F80u; }

// better(a, b): does (sa, ia) beat (sb, ib)? larger score, then lower index; index < 0 = nothing yet
__device__ __forceinline__ bool better(float sa, int ia, float sb, int ib) {
  return ia >= 0 && (ib < 0 || sa > sb || (sa == sb && ia < ib));
}

struct SampleParams {
  const u16* logits;
  const int* pos;
  int64_t* out;
  int ld, vocab, top_k;
  float inv_temp;  // 0: greedy
  unsigned long long seed;
  unsigned sample0;
  int rps;  // logits rows per sample (>= 1): row r belongs to sample sample0 + r / rps
};

// sample_step's additions: the nucleus and the step's bookkeeping (all optional: a null pointer switches a part off)
struct StepParams {
  SampleParams s;  // s.out: the step's tokens [rows]
  double top_p;    // outside (0, 1): off
  double a_scale;  // log2(e) / T
  int64_t* seq;    // [rows][ld_seq] token matrix, W columns
  long ld_seq;
  int W;
  int* done;     // [rows] flags
  int* gen_len;  // [rows]
  int64_t eos, pad;
  u16* thr_out;  // test hook: write theta [rows] and return
};

// The top-k threshold: the key of the k-th largest logit value (0: every key), by two 256-bin counting passes. All
// threads return the same value.
__device__ __forceinline__ unsigned top_k_threshold(const u16* lg, int vocab, int top_k, unsigned* hist,
                                                    unsigned* sh_bin, unsigned* sh_above) {
  const int tid = threadIdx.x;
  unsigned thr = 0;  // candidates: key16 >= thr
  if (top_k > 0 && top_k < vocab) {
    unsigned hi = 0, above = 0;
    for (int pass = 0; pass < 2; ++pass) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int v = tid; v < vocab; v += ST) {
        const u16 b = lg[v];
        if (is_nan_bf16(b)) continue;
        const unsigned k = key16(b);
        if (pass == 0)
          atomicAdd(&hist[k >> 8], 1u);
        else if ((k >> 8) == hi)
          atomicAdd(&hist[k & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {  // from the top: the bin in which the count reaches top_k
        unsigned cum = above;
        int bin = 255;
        for (; bin > 0; --bin) {
          if (cum + hist[bin] >= (unsigned)top_k) break;
          cum += hist[bin];
        }
        *sh_bin = (unsigned)bin;
        *sh_above = cum;
      }
      __syncthreads();
      if (pass == 0) {
        hi = *sh_bin;
        above = *sh_above;
      } else {
        thr = (hi << 8) | *sh_bin;
      }
      __syncthreads();
    }
  }
  return thr;
}

// The row's token among the keys >= thr: greedy or Gumbel-max. Valid in thread 0 (a row of NaNs: -1).
__device__ __forceinline__ int draw_token(const SampleParams& p, const u16* lg, int row, unsigned thr, float* red_s,
                                          int* red_i) {
  const int tid = threadIdx.x;
  const bool greedy = p.inv_temp == 0.f;
  unsigned pk = 0;
  if (!greedy) {
    const unsigned rkey = drop_row_key(drop_site_key(p.seed, (unsigned)DROP_SITE_SAMPLE << 16), p.sample0 + (unsigned)(row / p.rps), 0);
    pk = rkey ^ ((unsigned)p.pos[row] * 0x9E3779B1u);  // drop_word(rkey, position, v) = fmix32(pk ^ v * 0x85EBCA77)
  }
  float best = 0.f;
  int bi = -1;
  for (int v = tid; v < p.vocab; v += ST) {
    const u16 b = lg[v];
    if (is_nan_bf16(b) || key16(b) < thr) continue;
    float s = bf2f(b);
    if (!greedy) {
      const unsigned word = drop_fmix32(pk ^ ((unsigned)v * 0x85EBCA77u));
      const float u = __fmul_rn((float)(word >> 9) + 0.5f, 1.1920928955078125e-07f);  // 2^-23, exact
      const float g = -logf(-logf(u));
      s = __fadd_rn(__fmul_rn(s, p.inv_temp), g);
    }
    if (better(s, v, best, bi)) best = s, bi = v;  // (v ascends: ties keep the earlier index)
  }
  // wave, then block: the same rule at every level
  for (int off = 32; off > 0; off >>= 1) {
    const float os = __shfl_xor(best, off);
    const int oi = __shfl_xor(bi, off);
    if (better(os, oi, best, bi)) best = os, bi = oi;
  }
  if ((tid & 63) == 0) red_s[tid >> 6] = best, red_i[tid >> 6] = bi;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < ST / 64; ++w)
      if (better(red_s[w], red_i[w], best, bi)) best = red_s[w], bi = red_i[w];
  return bi;
}

__global__ void __launch_bounds__(ST) sample_logits_kernel(SampleParams p) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_bin, sh_above;
  __shared__ float red_s[ST / 64];
  __shared__ int red_i[ST / 64];
  const int row = blockIdx.x;
  const u16* lg = p.logits + (int64_t)row * p.ld;
  const unsigned thr = top_k_threshold(lg, p.vocab, p.top_k, hist, &sh_bin, &sh_above);
  const int bi = draw_token(p, lg, row, thr, red_s, red_i);
  if (threadIdx.x == 0) p.out[row] = bi < 0 ? 0 : bi;  // (a row of NaNs: token 0)
}

// ---- top-p ---------------------------------------------------------------------------------------------------------
// The mass of a candidate in units of 2^-kMassBits of the largest candidate's: w = exp2(a), a = (l - l_max) * log2(e) / T
// <= 0. The difference of two bf16 values and the split a = n + f (n integer, f in [0, 1)) are exact in fp64 (the product
// rounds once, to 2^-53); f rounds to fp32 (2^-25 absolute), exp2f(f) in [1, 2] is good to an ulp, the scaling by
// 2^(kMassBits + n) is exact and the conversion truncates: docs/NUMERICS.md sums these up. A token at the maximum weighs
// exactly 2^kMassBits; one below 2^-kMassBits of it weighs 0. vocab <= 2^23 (the host checks): a sum stays below 2^63.
constexpr int kMassBits = 40;

__device__ __forceinline__ unsigned long long top_p_mass(u16 b, unsigned k, unsigned kmax, double lmax, double a_scale) {
  if (k == kmax) return 1ull << kMassBits;
  const double a = ((double)bf2f(b) - lmax) * a_scale;
  if (!(a >= -(double)kMassBits)) return 0;  // (-inf, and inf - inf, land here too)
  const double n = floor(a);
  const float w = exp2f((float)(a - n));
  return (unsigned long long)ldexpf(w, kMassBits + (int)n);
}

// The nucleus threshold: the largest key x whose tokens {key >= x} among the candidates {key >= thr_k} hold at least
// top_p of the candidates' mass. The same two passes as top-k with 64-bit integer masses in the bins (integer sums do
// not depend on the order of the atomics). All threads return the same value (>= thr_k).
__device__ __forceinline__ unsigned top_p_threshold(const u16* lg, int vocab, unsigned thr_k, double top_p,
                                                    double a_scale, unsigned long long* mass, unsigned* sh_bin,
                                                    unsigned long long* sh_above, unsigned long long* sh_target,
                                                    unsigned* sh_max) {
  const int tid = threadIdx.x;
  // the largest key (of a non-NaN logit): the reference point of the masses
  if (tid == 0) *sh_max = 0;
  __syncthreads();
  unsigned kmax = 0;
  for (int v = tid; v < vocab; v += ST) {
    const u16 b = lg[v];
    if (!is_nan_bf16(b)) kmax = max(kmax, key16(b));
  }
  for (int off = 32; off > 0; off >>= 1) kmax = max(kmax, __shfl_xor(kmax, off));
  if ((tid & 63) == 0) atomicMax(sh_max, kmax);
  __syncthreads();
  kmax = *sh_max;
  const u16 mb = (kmax & 0x8000u) ? (u16)(kmax & 0x7FFFu) : (u16)~kmax;
  const double lmax = (double)bf2f(mb);

  unsigned hi = 0, thr = thr_k;
  unsigned long long above = 0;
  for (int pass = 0; pass < 2; ++pass) {
    if (tid < 256) mass[tid] = 0;
    __syncthreads();
    for (int v = tid; v < vocab; v += ST) {
      const u16 b = lg[v];
      if (is_nan_bf16(b)) continue;
      const unsigned k = key16(b);
      if (k < thr_k || (pass == 1 && (k >> 8) != hi)) continue;
      const unsigned long long q = top_p_mass(b, k, kmax, lmax, a_scale);
      if (q) atomicAdd(&mass[pass == 0 ? (k >> 8) : (k & 255u)], q);
    }
    __syncthreads();
    if (tid == 0) {
      if (pass == 0) {  // the target: ceil(top_p * total), within [1, total]
        unsigned long long z = 0;
        for (int bin = 0; bin < 256; ++bin) z += mass[bin];
        unsigned long long t = (unsigned long long)ceil(top_p * (double)z);
        *sh_target = t < 1 ? 1 : (t > z ? z : t);
      }
      const unsigned long long target = *sh_target;
      unsigned long long cum = above;
      int bin = 255;
      for (; bin > 0; --bin) {  // from the top: the bin in which the mass reaches the target
        if (cum + mass[bin] >= target) break;
        cum += mass[bin];
      }
      *sh_bin = (unsigned)bin;
      *sh_above = cum;
    }
    __syncthreads();
    if (pass == 0) {
      hi = *sh_bin;
      above = *sh_above;
    } else {
      thr = max(thr_k, (hi << 8) | *sh_bin);
    }
    __syncthreads();
  }
  return thr;
}

__global__ void __launch_bounds__(ST) sample_step_kernel(StepParams q) {
  __shared__ unsigned long long mass[256];
  __shared__ unsigned long long sh_above64, sh_target;
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_bin, sh_above, sh_max;
  __shared__ float red_s[ST / 64];
  __shared__ int red_i[ST / 64];
  const SampleParams& p = q.s;
  const int row = blockIdx.x, tid = threadIdx.x;
  if (q.done && q.done[row]) {  // a finished row: the pad token, nothing else (uniform over the block)
    if (tid == 0) p.out[row] = q.pad;
    return;
  }
  const u16* lg = p.logits + (int64_t)row * p.ld;
  unsigned thr = top_k_threshold(lg, p.vocab, p.top_k, hist, &sh_bin, &sh_above);
  if (p.inv_temp != 0.f && q.top_p > 0.0 && q.top_p < 1.0)
    thr = top_p_threshold(lg, p.vocab, thr, q.top_p, q.a_scale, mass, &sh_bin, &sh_above64, &sh_target, &sh_max);
  if (q.thr_out) {  // the test hook: the threshold's value (no threshold: -inf)
    if (tid == 0) q.thr_out[row] = thr == 0 ? (u16)0xFF80u : ((thr & 0x8000u) ? (u16)(thr & 0x7FFFu) : (u16)~thr);
    return;
  }
  const int bi = draw_token(p, lg, row, thr, red_s, red_i);
  if (tid == 0) {
    const int64_t tok = bi < 0 ? 0 : bi;
    p.out[row] = tok;
    const int pos = p.pos[row];
    if (pos >= 0 && pos < q.W) {  // (the host API keeps positions inside the token matrix)
      if (q.seq) q.seq[(int64_t)row * q.ld_seq + pos] = tok;
      if (q.gen_len) q.gen_len[row] += 1;
      if (q.done && tok == q.eos) q.done[row] = 1;
    }
  }
}

// one wave per sample, 4 bf16 per lane per step
__global__ void __launch_bounds__(256) embed_at_kernel(const int64_t* __restrict__ tok, const int* __restrict__ pos,
                                                       const u16* __restrict__ wte, const u16* __restrict__ wpe,
                                                       u16* __restrict__ out, int rows, int C, int V, int P) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  int64_t t = tok[row];
  t = t < 0 ? 0 : (t >= V ? V - 1 : t);
  int q = pos[row];
  q = q < 0 ? 0 : (q >= P ? P - 1 : q);  // (the host API keeps positions below block_size)
  const u16x4* a = reinterpret_cast<const u16x4*>(wte + t * C);
  const u16x4* b = reinterpret_cast<const u16x4*>(wpe + (int64_t)q * C);
  u16x4* o = reinterpret_cast<u16x4*>(out + (int64_t)row * C);
  for (int c = lane; c < C / 4; c += 64) {
    const u16x4 va = a[c], vb = b[c];
    u16x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = f2bf(bf2f(va[e]) + bf2f(vb[e]));
    o[c] = r;
  }
}

}  // namespace

void sample_logits_bf16(const void* logits, int rows, int ld, int vocab, float inv_temp, int top_k,
                        unsigned long long seed, unsigned sample0, const int* pos, int64_t* out, hipStream_t stream,
                        int rows_per_sample) {
  if (rows <= 0) return;
  SampleParams p;
  p.logits = static_cast<const u16*>(logits);
  p.pos = pos;
  p.out = out;
  p.ld = ld, p.vocab = vocab, p.top_k = top_k;
  p.inv_temp = inv_temp;
  p.seed = seed;
  p.sample0 = sample0;
  p.rps = rows_per_sample > 0 ? rows_per_sample : 1;
  hipLaunchKernelGGL(sample_logits_kernel, dim3(rows), dim3(ST), 0, stream, p);
}

void sample_step_bf16(const SampleStepArgs& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  StepParams q;
  q.s.logits = static_cast<const u16*>(a.logits);
  q.s.pos = a.pos;
  q.s.out = a.tokens;
  q.s.ld = a.ld, q.s.vocab = a.vocab, q.s.top_k = a.top_k;
  q.s.inv_temp = a.temperature > 0.0 ? (float)(1.0 / a.temperature) : 0.f;
  q.s.seed = a.seed;
  q.s.sample0 = a.sample0;
  q.s.rps = a.rows_per_sample > 0 ? a.rows_per_sample : 1;
  q.top_p = a.top_p;
  q.a_scale = a.temperature > 0.0 ? 1.4426950408889634 / a.temperature : 0.0;
  q.seq = a.out;
  q.ld_seq = a.ld_out;
  q.W = a.out ? a.W : INT_MAX;  // (no token matrix: every position counts)
  q.done = a.done;
  q.gen_len = a.gen_len;
  q.eos = a.eos, q.pad = a.pad;
  q.thr_out = static_cast<u16*>(a.thr_out);
  hipLaunchKernelGGL(sample_step_kernel, dim3(a.rows), dim3(ST), 0, stream, q);
}

void embedding_at_bf16(const int64_t* tok, const int* pos, const void* wte, const void* wpe, void* out, int rows, int C,
                       int V, int P, hipStream_t stream) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(embed_at_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, tok, pos,
                     static_cast<const u16*>(wte), static_cast<const u16*>(wpe), static_cast<u16*>(out), rows, C, V, P);
}

}  // namespace sdml

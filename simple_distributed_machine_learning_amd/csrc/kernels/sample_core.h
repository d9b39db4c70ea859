// The sampler's device code, shared by sample.hip (sample_logits, sample_step) and sample_penalty.hip (sample_step
// with a repetition penalty, an n-gram ban and logprobs): the parameter blocks, the top-k and top-p thresholds and the
// draw. Every function reads the row through `lg[v]`, the bf16 bits of column v: a plain `const u16*` in sample.hip,
// sample_penalty.hip's processed row there, so all passes of one launch see one consistent row. Each file that
// includes this gets its own copy (an unnamed namespace): the kernels' names do not depend on who else includes it.
#pragma once

#include <climits>
#include <hip/hip_runtime.h>

#include "dropout_hash.h"
#include "kernels.h"
#include "logit_key.h"  // bf2f, key16, is_nan_bf16: shared with beam.hip

namespace sdml {
namespace {

constexpr int ST = 1024;  // sampler threads per row

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

inline StepParams step_params(const SampleStepArgs& a) {
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
  return q;
}

// The top-k threshold: the key of the k-th largest logit value (0: every key), by two 256-bin counting passes. All
// threads return the same value.
template <class Row>
__device__ __forceinline__ unsigned top_k_threshold(Row lg, int vocab, int top_k, unsigned* hist, unsigned* sh_bin,
                                                    unsigned* sh_above) {
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
template <class Row>
__device__ __forceinline__ int draw_token(const SampleParams& p, Row lg, int row, unsigned thr, float* red_s,
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
template <class Row>
__device__ __forceinline__ unsigned top_p_threshold(Row lg, int vocab, unsigned thr_k, double top_p, double a_scale,
                                                    unsigned long long* mass, unsigned* sh_bin,
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

}  // namespace
}  // namespace sdml

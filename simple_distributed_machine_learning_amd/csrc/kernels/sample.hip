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
// sample_step: sample_logits' token with two additions in the same launch (the device code, sample_core.h, is shared;
// sample_penalty.hip is the variant with a repetition penalty, an n-gram ban and logprobs).
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

#include "kernels.h"
#include "sample_core.h"  // the thresholds and the draw: shared with sample_penalty.hip

namespace sdml {
namespace {

typedef u16 u16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u16 f2bf(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<u16*>(&h);
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
  if (a.pen_neg != 1.f || a.pen_pos != 1.f || a.ngram > 0 || a.logp)  // the variant: sample_penalty.hip
    return sample_step_penalty_bf16(a, stream);
  const StepParams q = step_params(a);
  hipLaunchKernelGGL(sample_step_kernel, dim3(a.rows), dim3(ST), 0, stream, q);
}

void embedding_at_bf16(const int64_t* tok, const int* pos, const void* wte, const void* wpe, void* out, int rows, int C,
                       int V, int P, hipStream_t stream) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(embed_at_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, tok, pos,
                     static_cast<const u16*>(wte), static_cast<const u16*>(wpe), static_cast<u16*>(out), rows, C, V, P);
}

}  // namespace sdml

// sample_step with a repetition penalty, an n-gram ban and logprobs in the same launch (ops/reference.py
// process_logits and sample_step are the definition; kernels.h SampleStepArgs lists the arguments). The token is
// sample_step's token on the processed row; nothing else of the sampler changes, and with the three parts off
// sample_step_bf16 launches sample.hip's kernel, not this one.
//
// One workgroup of 1024 threads per row, as there. Before the threshold passes:
//   * two LDS bitmaps of vocab bits, `seen` and `banned` (kSamplePenaltyMaxVocab = 65536 bits = 8 KB each; GPT-2's
//     50257 uses 6.3 KB of each). The threads stride over the row's history hist = out[row][0 .. pos), one int64 read
//     per token: token hist[s] sets its bit of `seen` (integer LDS atomic OR: the bits do not depend on the order), and
//     with a ban of size n, m = n - 1, it sets its bit of `banned` where s >= m and hist[s - m .. s) equals the
//     history's last m tokens, which every thread holds in registers (<= 7). The start s - m of such a window obeys
//     (s - m) + m < pos because s < pos; with pos < n no s passes s >= m, so nothing is banned; n = 1 (m = 0) bans
//     every token of the history.
//   * one load function, ProcessedRow::operator[]: the bf16 bits of column v as every later pass sees them,
//       banned(v) ? -inf : seen(v) ? bf16_rn(fp32(l_v) * (l_v < 0 ? theta : 1 / theta)) : l_v
//     one fp32 multiply (__fmul_rn: never contracted) and one round-to-nearest-even. The top-k counting passes, the
//     top-p maximum and mass passes and the draw (sample_core.h) read the row through it, so they see one consistent
//     row and no second copy of the logits exists in memory. -0, NaN and +-inf follow from the multiply.
//   * logprobs: m = max and S = sum exp(l_v - m) over the RAW row in fp32, a thread over its columns v = tid, tid +
//     1024, .. in order, a wave on DPP / permlane swaps (wave_ops.h), the 16 wave sums in wave order, as beam.hip's row
//     pass reduces; a NaN counts as -inf. lse = m + log S, and thread 0 stores logp[row][pos] = l_tok - lse (one
//     __fsub_rn) next to out[row][pos]. No float atomics: the bits are the same on every run. docs/NUMERICS.md
//     "Sampler logprobs" bounds the error.
// The three parts are template parameters: a part that is off costs no instruction and no LDS.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "sample_core.h"
#include "wave_ops.h"

namespace sdml {
namespace {

constexpr int kWords = kSamplePenaltyMaxVocab / 32;  // of one bitmap
constexpr int kMaxM = kSampleMaxNgram - 1;
constexpr u16 kNegInf = 0xFF80u;

struct PenaltyParams {
  float f_neg, f_pos;  // theta, 1 / theta
  int ngram;
  float* logp;
  long ld_logp;
};

// fp32 -> bf16 bits, round to nearest even (a NaN stays a NaN; the sampler skips it whatever its payload)
__device__ __forceinline__ u16 bf16_rn(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u16)((u >> 16) | 0x0040u);
  return (u16)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

template <bool PEN, bool BAN>
struct ProcessedRow {
  const u16* lg;
  const unsigned* seen;
  const unsigned* banned;
  float f_neg, f_pos;
  __device__ __forceinline__ u16 operator[](int v) const {
    const unsigned bit = 1u << (v & 31);
    if (BAN && (banned[v >> 5] & bit)) return kNegInf;
    u16 b = lg[v];
    if (PEN && (seen[v >> 5] & bit)) {
      const float l = bf2f(b);
      b = bf16_rn(__fmul_rn(l, l < 0.f ? f_neg : f_pos));
    }
    return b;
  }
};

// `seen` and `banned` of the row's history hs[0 .. h); returns after a barrier
template <bool PEN, bool BAN>
__device__ __forceinline__ void build_bitmaps(const int64_t* hs, int h, int vocab, int ngram, unsigned* seen,
                                              unsigned* banned) {
  const int tid = threadIdx.x;
  for (int i = tid; i < (vocab + 31) >> 5; i += ST) {
    if (PEN) seen[i] = 0;
    if (BAN) banned[i] = 0;
  }
  __syncthreads();
  const int m = ngram - 1;
  int64_t suf[kMaxM] = {};
  if (BAN && h >= ngram) {
#pragma unroll
    for (int j = 0; j < kMaxM; ++j) suf[j] = j < m ? hs[h - m + j] : 0;
  }
  for (int s = tid; s < h; s += ST) {
    const int64_t t = hs[s];
    if ((unsigned long long)t >= (unsigned long long)vocab) continue;  // (no logit to change)
    const unsigned bit = 1u << ((unsigned)t & 31u);
    if (PEN) atomicOr(&seen[t >> 5], bit);
    if (BAN && s >= m) {  // (then h > m: suf is loaded)
      bool hit = true;
#pragma unroll
      for (int j = 0; j < kMaxM; ++j)
        if (j < m) hit = hit && hs[s - m + j] == suf[j];
      if (hit) atomicOr(&banned[t >> 5], bit);
    }
  }
  __syncthreads();
}

// log-sum-exp of the raw row in a fixed order (a row without a finite logit: -inf). All threads return the same bits.
__device__ __forceinline__ float row_lse(const u16* lg, int vocab, float* red_f) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float mx = -INFINITY;
  for (int v = tid; v < vocab; v += ST) {
    const u16 b = lg[v];
    if (!is_nan_bf16(b)) mx = fmaxf(mx, bf2f(b));
  }
  mx = wv::max64(mx);
  if (lane == 0) red_f[wave] = mx;
  __syncthreads();
  float m = red_f[0];
  for (int i = 1; i < ST / 64; ++i) m = fmaxf(m, red_f[i]);
  __syncthreads();
  const float m0 = m > -INFINITY ? m : 0.f;
  float sum = 0.f;
  for (int v = tid; v < vocab; v += ST) {
    const u16 b = lg[v];
    if (!is_nan_bf16(b)) sum += expf(__fsub_rn(bf2f(b), m0));
  }
  sum = wv::sum64(sum);
  if (lane == 0) red_f[wave] = sum;
  __syncthreads();
  float S = red_f[0];
  for (int i = 1; i < ST / 64; ++i) S += red_f[i];
  __syncthreads();
  return __fadd_rn(m0, logf(S));
}

template <bool PEN, bool BAN, bool LOGP>
__global__ void __launch_bounds__(ST) sample_step_penalty_kernel(StepParams q, PenaltyParams e) {
  __shared__ unsigned long long mass[256];
  __shared__ unsigned long long sh_above64, sh_target;
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_bin, sh_above, sh_max;
  __shared__ float red_s[ST / 64];
  __shared__ int red_i[ST / 64];
  __shared__ unsigned seen[PEN ? kWords : 1], banned[BAN ? kWords : 1];
  const SampleParams& p = q.s;
  const int row = blockIdx.x, tid = threadIdx.x;
  if (q.done && q.done[row]) {  // a finished row: the pad token, nothing else (uniform over the block)
    if (tid == 0) p.out[row] = q.pad;
    return;
  }
  const u16* raw = p.logits + (int64_t)row * p.ld;
  const int pos = p.pos[row];
  if (PEN || BAN)
    build_bitmaps<PEN, BAN>(q.seq + (int64_t)row * q.ld_seq, min(max(pos, 0), q.W), p.vocab, e.ngram, seen, banned);
  float lse = 0.f;
  if (LOGP) lse = row_lse(raw, p.vocab, red_s);
  const ProcessedRow<PEN, BAN> lg = {raw, seen, banned, e.f_neg, e.f_pos};
  unsigned thr = top_k_threshold(lg, p.vocab, p.top_k, hist, &sh_bin, &sh_above);
  if (p.inv_temp != 0.f && q.top_p > 0.0 && q.top_p < 1.0)
    thr = top_p_threshold(lg, p.vocab, thr, q.top_p, q.a_scale, mass, &sh_bin, &sh_above64, &sh_target, &sh_max);
  const int bi = draw_token(p, lg, row, thr, red_s, red_i);
  if (tid == 0) {
    const int64_t tok = bi < 0 ? 0 : bi;
    p.out[row] = tok;
    if (pos >= 0 && pos < q.W) {
      q.seq[(int64_t)row * q.ld_seq + pos] = tok;
      if (LOGP) e.logp[(int64_t)row * e.ld_logp + pos] = __fsub_rn(bf2f(raw[tok]), lse);
      if (q.gen_len) q.gen_len[row] += 1;
      if (q.done && tok == q.eos) q.done[row] = 1;
    }
  }
}

template <bool PEN, bool BAN, bool LOGP>
void launch(const StepParams& q, const PenaltyParams& e, int rows, hipStream_t stream) {
  hipLaunchKernelGGL((sample_step_penalty_kernel<PEN, BAN, LOGP>), dim3(rows), dim3(ST), 0, stream, q, e);
}

}  // namespace

void sample_step_penalty_bf16(const SampleStepArgs& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  const bool pen = a.pen_neg != 1.f || a.pen_pos != 1.f, ban = a.ngram > 0, logp = a.logp != nullptr;
  // (the binding refuses these with a message; here they only keep the kernel inside its bitmaps and its registers)
  if (!a.out || a.thr_out || a.ngram > kSampleMaxNgram || ((pen || ban) && a.vocab > kSamplePenaltyMaxVocab)) return;
  const StepParams q = step_params(a);
  const PenaltyParams e = {a.pen_neg, a.pen_pos, a.ngram, a.logp, a.ld_logp};
  switch ((int)pen | (int)ban << 1 | (int)logp << 2) {
    case 1: return launch<true, false, false>(q, e, a.rows, stream);
    case 2: return launch<false, true, false>(q, e, a.rows, stream);
    case 3: return launch<true, true, false>(q, e, a.rows, stream);
    case 4: return launch<false, false, true>(q, e, a.rows, stream);
    case 5: return launch<true, false, true>(q, e, a.rows, stream);
    case 6: return launch<false, true, true>(q, e, a.rows, stream);
    case 7: return launch<true, true, true>(q, e, a.rows, stream);
  }
}

}  // namespace sdml

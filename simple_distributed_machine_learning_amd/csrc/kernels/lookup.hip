// Prompt-lookup speculation's bookkeeping on the device (parallel/generate.py lookup=K): accept the drafts of the
// verify step that just ran, then draft the next step's tokens from the row's own history. ops/reference.py
// lookup_step is the definition; this kernel equals it cell for cell. Integer work only, no atomics: the same bits on
// every run.
//
// Per row b, T = K + 1: out [B][W] is the token matrix, lens[b] the cache length = the column of the row's newest
// token (not yet in the cache), limit[b] the row's final width (clamped to W).
//   accept (g != nullptr; skipped for a row that is done or full, lens[b] + 1 >= limit[b]): g[b][0..K] are the
//     sampler's tokens for the step's T positions, tok_in[b][1..] its n = nq_in[b] - 1 drafts. a = the number of
//     leading drafts that equal their g; the row emits g[b][0..a], cut to the columns below limit[b] and after the
//     first eos (kept): out[b][lens[b] + 1 + i] = g[b][i], gen_len[b] and lens[b] grow by the count, done[b] is set on
//     the eos, row_steps[b] grows by one.
//   draft: hist = out[b][0 .. lens[b]] (the new length). s = the largest start <= lens[b] - N whose N tokens equal the
//     last N of hist; n = min(K, lens[b] - s - N + 1, limit[b] - 2 - lens[b]) drafts hist[s + N + i] (none without a
//     match). tok_next[b] = the newest token, the drafts, the pad token; nq_next[b] = 1 + n, or 0 for a done or full
//     row (whose tok_next is the pad token throughout).
//   all_done[0] = 1 iff every nq_next is 0.
//
// One block of kLookupWaves waves, a wave per row in turn (a history has at most a few thousand tokens). The tokens a
// row emits in this launch are read back from the emitting lanes' registers, never from memory.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace sdml {
namespace {

constexpr int kLookupWaves = 16;

__global__ void __launch_bounds__(64 * kLookupWaves) lookup_step_kernel(LookupStepArgs p) {
  __shared__ int sh_alive[kLookupWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = p.K + 1;
  int alive = 0;
  for (int b = wave; b < p.B; b += kLookupWaves) {  // (wave-uniform)
    int64_t* row = p.out + (int64_t)b * p.ld_out;
    const int len0 = p.lens[b];
    const int lim = min(p.limit[b], p.W);
    int len = len0;
    bool dn = p.done[b] != 0 || len0 < 0 || len0 >= p.W;  // (a length outside the matrix: the row is left alone)
    // ---- accept: lane i holds g[b][i]
    int gi = 0, cnt = 0;
    if (p.g != nullptr && !dn && len0 + 1 < lim) {
      const int n = max(0, min(p.nq_in[b] - 1, p.K));
      if (lane < T) gi = (int)p.g[(int64_t)b * T + lane];
      const bool miss = lane < n && p.tok_in[(int64_t)b * T + 1 + lane] != (int64_t)gi;
      const unsigned long long mm = __ballot(miss);
      const int a = mm ? __ffsll((long long)mm) - 1 : n;
      cnt = min(a + 1, lim - 1 - len0);  // columns len0 + 1 + i < lim; >= 1: the row is not full
      const unsigned long long em = __ballot(lane < cnt && (int64_t)gi == p.eos);
      if (em) cnt = __ffsll((long long)em), dn = true;
      if (lane < cnt) row[len0 + 1 + lane] = gi;
      len = len0 + cnt;
      if (lane == 0) {
        p.lens[b] = len;
        p.gen_len[b] += cnt;
        p.row_steps[b] += 1;
        if (em) p.done[b] = 1;
      }
    }
    // hist(j), j <= len: columns <= len0 from memory (not written in this launch), later ones from lane j - len0 - 1.
    // Every lane of the wave calls it together (the shuffle).
    auto hist = [&](int j) -> int {
      const int fresh = __shfl(gi, min(max(j - len0 - 1, 0), 63));
      return j <= len0 ? (int)row[max(j, 0)] : fresh;
    };
    // ---- draft
    int n = 0, s_best = -1;
    const bool open = !dn && len + 1 < lim;
    if (open && len >= p.N) {
      int suf[kLookupMaxNgram];
#pragma unroll
      for (int k = 0; k < kLookupMaxNgram; ++k) {
        suf[k] = 0;
        if (k < p.N) suf[k] = hist(len - p.N + 1 + k);
      }
      const int n_starts = len - p.N + 1;  // s = 0 .. len - N
      for (int s0 = 0; s0 < n_starts; s0 += 64) {
        const int s = min(s0 + lane, n_starts - 1);
        bool hit = s0 + lane < n_starts;
#pragma unroll
        for (int k = 0; k < kLookupMaxNgram; ++k)
          if (k < p.N) hit = (hist(s + k) == suf[k]) && hit;
        if (hit) s_best = s;  // (s ascends with the rounds: the last hit of a lane is its largest)
      }
      for (int off = 32; off > 0; off >>= 1) s_best = max(s_best, __shfl_xor(s_best, off));
      if (s_best >= 0) n = max(0, min(min(p.K, len - s_best - p.N + 1), lim - 2 - len));
    }
    const int newest = hist(min(len, p.W - 1));
    const int draft = hist(min(max(s_best, 0) + p.N + max(lane - 1, 0), len));
    if (lane < T) {
      int64_t v = p.pad;
      if (open && lane == 0) v = newest;
      if (open && lane >= 1 && lane <= n) v = draft;
      p.tok_next[(int64_t)b * T + lane] = v;
    }
    if (lane == 0) p.nq_next[b] = open ? 1 + n : 0;
    alive |= open ? 1 : 0;
  }
  if (lane == 0) sh_alive[wave] = alive;
  __syncthreads();
  if (threadIdx.x == 0) {
    int any = 0;
    for (int w = 0; w < kLookupWaves; ++w) any |= sh_alive[w];
    p.all_done[0] = any ? 0 : 1;
  }
}

}  // namespace

void lookup_step(const LookupStepArgs& a, hipStream_t stream) {
  if (a.B <= 0) return;
  hipLaunchKernelGGL(lookup_step_kernel, dim3(1), dim3(64 * kLookupWaves), 0, stream, a);
}

}  // namespace sdml

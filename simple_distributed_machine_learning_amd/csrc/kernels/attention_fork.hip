// Shared-prefix (fork) decode attention, bf16, head width 64 (models/gpt2.py decode_step_forked): n continuations of
// one prompt, one new token each.
//
// R = G * n rows; row r = g * n + j is sibling j of group g. The group's prompt keys sit once in the prefix cache
// kp / vp [G][Pmax][H][64] (plens[g] of them; only read here), every row's own later keys in the suffix cache ks / vs
// [R][Nmax][H][64]; lens[r] = plens[g] + the row's suffix keys. Key i of row r is
//   kp[g][i]                    i < plens[g]
//   ks[r][i - plens[g]]         plens[g] <= i < lens[r]
//   the row's own qkv           i == lens[r]     (written to suffix row lens[r] - plens[g], bit for bit)
// and the row returns softmax(q . K[0..lens[r]]^T * scale) . V[0..lens[r]].
//
// Bit contract: row r gets the bits attention_decode.hip gives that token on a cache that holds the group's prompt
// rows followed by the row's suffix rows, with lens[r] keys cached. The arithmetic below is that kernel's, per query:
// the same kAttnDecodeChunk-key chunks at the absolute key index, one wave each, the same lane -> (row group, channel
// piece) mapping and fma chains, the same DPP reductions, one (m, l, o[64]) slot per (r, h, chunk), the same combine
// in chunk order in a second launch (tests/test_attention_fork_gpu.py compares the raw bits). That arithmetic is
// defined in attn_chunk.h, which attention_decode.hip and attention_append.hip call; this file keeps its own copy of
// chunk_query and the combine (on the header its chunk kernel was slower, profiles/decode_chunk_ab.jsonl), so a change
// to attn_chunk.h must be repeated here.
//
// The gain: a chunk c with (c + 1) * CH <= plens[g] lies wholly in the prompt and is the same for the n siblings. The
// block of sibling 0 loads its K and V rows to VGPRs once and runs the n queries against them in a wave-uniform loop,
// writing n slots; the other siblings' blocks of that chunk return. Every sibling sees all CH keys of such a chunk,
// so nothing is masked: decode's selects all take their first operand there. Every other live chunk, the one that
// straddles plens[g] included, is per sibling, each row's address selected between prefix, suffix and qkv as
// attention_decode.hip selects between cache and qkv.
//
// Keys past lens[r] never reach the result: their loads are redirected to the row's own qkv, their scores and
// probabilities are selected away. Nothing is read from prefix rows >= plens[g] or suffix rows >= lens[r] -
// plens[g] (they may hold anything). The chunk that contains index lens[r] owns the suffix write and takes that key
// from qkv, so no wave reads a row that another wave writes. A row whose lengths fall outside the caches or the
// host's bound n_keys is not indexed at all (row_ok); its output is not written.
//
// Two launches (chunks, combine), no atomics: a row's result depends on its own row of qkv, its group's prompt rows,
// its own suffix rows, plens[g] and lens[r] only; the same bits on every run, for a group alone or in any batch.
//
// Rounding: scores, exp2, sums and the combine are fp32; the output is rounded to bf16 once.
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "wave_ops.h"

namespace sdml {
namespace {

typedef unsigned short u16;
typedef u16 u16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CH = kAttnDecodeChunk;  // keys per wave
constexpr int RPL = CH / 8;           // rows per lane (8 lanes hold one row)
constexpr float kLog2e = 1.4426950408889634f;
constexpr int ROR8 = 0x128;  // DPP row_ror:8: lane i <- lane i ^ 8 inside a row of 16

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ u16 f2bf(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<u16*>(&h);
}

// sum / max over the 8 row groups of a wave (lane bits 3..5), as in attention_decode.hip
__device__ __forceinline__ float sum_groups(float x) { return wv::sum_rows(x + wv::dpp<ROR8>(x)); }
__device__ __forceinline__ float max_groups(float x) { return wv::max_rows(fmaxf(x, wv::dpp<ROR8>(x))); }

// the lengths the kernel may index with: the prompt inside the prefix cache, the suffix (the new row included) inside
// the suffix cache, the new key inside the host's bound (so inside the workspace's chunks)
__device__ __forceinline__ bool row_ok(const AttnForkArgs& p, int plen, int len) {
  return plen >= 0 && plen <= p.Pmax && len >= plen && len - plen < p.Nmax && len < p.n_keys;
}

// One query against a chunk's rows in VGPRs: attention_decode.hip's score, softmax and P.V lines. Keys past `last`
// are selected away (a shared chunk passes its own last key, so every select takes the live operand). No contraction:
// the products and sums are the ones written, as they are where decode's selects stand between them.
__device__ __forceinline__ void chunk_query(const AttnForkArgs& p, const u16x8 (&kv)[RPL], const u16x8 (&vv)[RPL],
                                            const u16* qrow, int c, int last, int64_t slot, int lane) {
#pragma clang fp contract(off)
  const int pc = lane & 7, rg = lane >> 3;
  const u16x8 qv = *reinterpret_cast<const u16x8*>(qrow);
  float q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) q[e] = bf2f(qv[e]);

  const float sl2 = p.scale * kLog2e;
  float s[RPL];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg;
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) a = fmaf(q[e], bf2f(kv[i][e]), a);
    a += wv::dpp<wv::XOR1>(a);
    a += wv::dpp<wv::XOR2>(a);
    a += wv::dpp<wv::HALF_MIRROR>(a);  // the row's 8 lanes hold the same sum
    s[i] = j <= last ? a * sl2 : -INFINITY;
    m = fmaxf(m, s[i]);
  }
  m = max_groups(m);  // finite: key c * CH <= last is in this chunk

  float l = 0.f, o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg;
    const float pr = j <= last ? __builtin_amdgcn_exp2f(s[i] - m) : 0.f;
    l += pr;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaf(pr, bf2f(vv[i][e]), o[e]);
  }
  l = sum_groups(l);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = sum_groups(o[e]);

  if (lane < 8) {
    f32x4* dst = reinterpret_cast<f32x4*>(p.ws_o + slot * 64 + 8 * pc);
    dst[0] = f32x4{o[0], o[1], o[2], o[3]};
    dst[1] = f32x4{o[4], o[5], o[6], o[7]};
  }
  if (lane == 0) {
    p.ws_ml[slot * 2] = m;
    p.ws_ml[slot * 2 + 1] = l;
  }
}

// grid (chunks, H, R), one wave per block. Lane l: piece l & 7 (channels 8 (l & 7) ..), row group l >> 3; its keys
// are chunk * CH + 8 i + (l >> 3), i = 0 .. RPL - 1.
__global__ void __launch_bounds__(64) attn_fork_chunk_kernel(AttnForkArgs p) {
  const int c = blockIdx.x, h = blockIdx.y, r = blockIdx.z, lane = threadIdx.x;
  const int g = r / p.n, sib = r - g * p.n;
  const int plen = p.plens[g];
  const int pc = lane & 7, rg = lane >> 3;
  const int C = p.H * 64;
  const int64_t pbase = (int64_t)g * p.psb + (int64_t)h * p.psh + 8 * pc;
  const u16* kpre = static_cast<const u16*>(p.k_prefix) + pbase;
  const u16* vpre = static_cast<const u16*>(p.v_prefix) + pbase;

  // a chunk that lies wholly in the prompt: sibling 0's wave loads it once and serves the group's n queries
  const bool shared = plen >= 0 && plen <= p.Pmax && (c + 1) * CH <= plen;
  int len = plen;  // (shared: every key of the chunk is a prefix key, none is the new one)
  if (shared) {
    if (sib != 0) return;
  } else {
    len = p.lens[r];
    if (!row_ok(p, plen, len)) return;  // (never index outside the caches)
    if (c * CH > len) return;
  }
  const u16* qrow = static_cast<const u16*>(p.qkv) + (int64_t)r * p.ldq + h * 64 + 8 * pc;
  const u16* knew = qrow + C;
  const u16* vnew = qrow + 2 * C;
  const int64_t sbase = (int64_t)r * p.ssb + (int64_t)h * p.ssh + 8 * pc;
  u16* ksuf = static_cast<u16*>(p.k_suffix) + sbase;
  u16* vsuf = static_cast<u16*>(p.v_suffix) + sbase;

  u16x8 kv[RPL], vv[RPL];
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg;
    const u16* src = j < plen ? kpre + (int64_t)j * p.pss : (j < len ? ksuf + (int64_t)(j - plen) * p.sss : knew);
    kv[i] = *reinterpret_cast<const u16x8*>(src);
  }
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg;
    const u16* src = j < plen ? vpre + (int64_t)j * p.pss : (j < len ? vsuf + (int64_t)(j - plen) * p.sss : vnew);
    vv[i] = *reinterpret_cast<const u16x8*>(src);
  }
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg;
    if (!shared && j == len) {  // the new token's row: bit for bit from qkv (len - plen < Nmax)
      *reinterpret_cast<u16x8*>(ksuf + (int64_t)(j - plen) * p.sss) = kv[i];
      *reinterpret_cast<u16x8*>(vsuf + (int64_t)(j - plen) * p.sss) = vv[i];
    }
  }
  // the queries of the chunk: the row's own, or in a shared chunk those of the n siblings (rows r .. r + n - 1),
  // each of which sees all of its keys
  const int nq = shared ? p.n : 1;
  const int last = shared ? c * CH + CH - 1 : len;
  for (int t = 0; t < nq; ++t) {  // (wave-uniform)
    const int rt = r + t;
    if (shared && !row_ok(p, plen, p.lens[rt])) continue;
    chunk_query(p, kv, vv, qrow + (int64_t)t * p.ldq, c, last, ((int64_t)rt * p.H + h) * p.max_chunks + c, lane);
  }
}

// grid (H, R), one wave per block, lane = channel: the chunks of one (r, h) in chunk order (attention_decode.hip
// combine_chunks)
__global__ void __launch_bounds__(64) attn_fork_combine_kernel(AttnForkArgs p) {
  const int h = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
  const int len = p.lens[r];
  if (!row_ok(p, p.plens[r / p.n], len)) return;
  const int nc = len / CH + 1;  // <= max_chunks: len < n_keys
  const int64_t slot = ((int64_t)r * p.H + h) * p.max_chunks;
  float M = -INFINITY;
  for (int c = 0; c < nc; ++c) M = fmaxf(M, p.ws_ml[(slot + c) * 2]);
  float L = 0.f, O = 0.f;
  for (int c = 0; c < nc; ++c) {
    const float w = __builtin_amdgcn_exp2f(p.ws_ml[(slot + c) * 2] - M);
    L = fmaf(p.ws_ml[(slot + c) * 2 + 1], w, L);
    O = fmaf(p.ws_o[(slot + c) * 64 + lane], w, O);
  }
  static_cast<u16*>(p.out)[(int64_t)r * p.H * 64 + h * 64 + lane] = f2bf(O / L);
}

}  // namespace

void attention_fork_bf16(const AttnForkArgs& a, hipStream_t stream) {
  if (a.G <= 0 || a.n <= 0 || a.H <= 0 || a.max_chunks <= 0) return;
  const int R = a.G * a.n;
  hipLaunchKernelGGL(attn_fork_chunk_kernel, dim3(a.max_chunks, a.H, R), dim3(64), 0, stream, a);
  hipLaunchKernelGGL(attn_fork_combine_kernel, dim3(a.H, R), dim3(64), 0, stream, a);
}

}  // namespace sdml

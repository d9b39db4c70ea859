// Multi-query (append) attention against a KV cache, bf16, head width 64 (models/gpt2.py decode_block).
//
// T = 1 .. kAttnAppendMaxT new tokens per sample: qkv [B][T][3C] holds their fused projections, the cache holds
// lens[b] earlier keys, nq[b] in 0 .. T of the sample's queries are live. Live query t writes its k and v rows to
// cache row lens[b] + t, bit for bit from qkv, and returns
//   softmax(q_t . K[0..lens[b]+t]^T * scale) . V[0..lens[b]+t]        (lens[b] + t + 1 keys, its own included)
// A dead query (t >= nq[b], or a row lens[b] + t at or past the host's bound n_keys) writes no cache row and returns
// exact zeros. lens is not changed.
//
// Bit contract: query (b, t) gets the bits attention_decode.hip gives that token with lens[b] + t keys cached: both
// run attn_chunk.h's chunk_query per (query, chunk) with the same chunks and lane mapping, and its combine_chunks in
// chunk order (tests/test_attention_append_gpu.py compares the raw bits). The gain over T calls: a chunk's K and V rows
// go to VGPRs once and serve all T queries.
//
// Keys: index j < lens[b] comes from the cache; j = lens[b] + r, r < nq[b], from row r of qkv; nothing is read from
// cache rows >= lens[b] (they may hold anything). Keys past a query's own index are selected away by chunk_query
// (their loads are redirected to a live row of qkv, so the unused operands are finite). A chunk
// is live for query t iff c * CH <= lens[b] + t. The chunk that contains index lens[b] + r owns that row's cache
// write, and takes the key from qkv, so no wave reads a row that another wave writes.
//
// Workspace: one (m, l, o[64]) slot per (b, t, h, chunk). Two launches (chunks, combine), no atomics: a sample's
// result depends on its own rows of qkv, its own cache rows, lens[b] and nq[b] only; the same bits on every run, in
// any batch.
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "attn_chunk.h"

namespace sdml {
namespace {

using namespace attn_chunk;

// live queries of sample b given its length: t < nq[b], and row len + t inside the host's bound (so inside the
// cache and the workspace's chunks). 0 for a length outside the cache.
__device__ __forceinline__ int live_queries(const AttnAppendArgs& p, int b, int len) {
  if (len < 0 || len >= p.n_keys) return 0;
  return max(0, min(min(p.nq[b], p.T), p.n_keys - len));
}

// grid (chunks, H, B), one wave per block. Lane l: piece l & 7 (channels 8 (l & 7) ..), row group l >> 3; its keys
// are chunk * CH + 8 i + (l >> 3), i = 0 .. RPL - 1.
__global__ void __launch_bounds__(64) attn_append_chunk_kernel(AttnAppendArgs p) {
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const int len = p.lens[b];
  const int n = live_queries(p, b, len);
  if (n <= 0 || c * CH > len + n - 1) return;
  const int pc = lane & 7, rg = lane >> 3;
  const int C = p.H * 64;
  const u16* qrow0 = static_cast<const u16*>(p.qkv) + (int64_t)b * p.T * p.ldq + h * 64 + 8 * pc;  // query 0
  const int64_t base = (int64_t)b * p.sb + (int64_t)h * p.sh + 8 * pc;
  u16* kc = static_cast<u16*>(p.k_cache) + base;
  u16* vc = static_cast<u16*>(p.v_cache) + base;

  // a chunk's rows, once for all queries: cached, or a live new row of qkv (index past the last one: row 0, unused)
  u16x8 kv[RPL], vv[RPL];
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg, r = j - len;
    const u16* src = r < 0 ? kc + (int64_t)j * p.ss : qrow0 + C + (int64_t)(r < n ? r : 0) * p.ldq;
    kv[i] = *reinterpret_cast<const u16x8*>(src);
  }
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg, r = j - len;
    const u16* src = r < 0 ? vc + (int64_t)j * p.ss : qrow0 + 2 * C + (int64_t)(r < n ? r : 0) * p.ldq;
    vv[i] = *reinterpret_cast<const u16x8*>(src);
  }
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg, r = j - len;
    if (r >= 0 && r < n) {  // the new tokens' rows: bit for bit from qkv (j = len + r < n_keys <= Smax)
      *reinterpret_cast<u16x8*>(kc + (int64_t)j * p.ss) = kv[i];
      *reinterpret_cast<u16x8*>(vc + (int64_t)j * p.ss) = vv[i];
    }
  }

  for (int t = 0; t < n; ++t) {  // (wave-uniform)
    const int lt = len + t;      // the query's own key index: keys 0 .. lt
    if (c * CH > lt) continue;
    float m, l, o[8];
    chunk_query(kv, vv, qrow0 + (int64_t)t * p.ldq, c, lt, p.scale, lane, m, l, o, NoRowHook{});
    store_slot(p.ws_ml, p.ws_o, (((int64_t)b * p.T + t) * p.H + h) * p.max_chunks + c, lane, m, l, o);
  }
}

// grid (H, T, B), one wave per block, lane = channel: the chunks of one (b, t, h) in chunk order; a dead
// query's row is zeros
__global__ void __launch_bounds__(64) attn_append_combine_kernel(AttnAppendArgs p) {
  const int h = blockIdx.x, t = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const int len = p.lens[b];
  u16* dst = static_cast<u16*>(p.out) + (((int64_t)b * p.T + t) * p.H + h) * 64 + lane;
  if (t >= live_queries(p, b, len)) {
    *dst = 0;
    return;
  }
  const int nc = (len + t) / CH + 1;  // <= max_chunks: len + t < n_keys
  *dst = combine_chunks(p.ws_ml, p.ws_o, (((int64_t)b * p.T + t) * p.H + h) * p.max_chunks, nc, lane);
}

}  // namespace

void attention_append_bf16(const AttnAppendArgs& a, hipStream_t stream) {
  if (a.B <= 0 || a.H <= 0 || a.T <= 0 || a.max_chunks <= 0) return;
  hipLaunchKernelGGL(attn_append_chunk_kernel, dim3(a.max_chunks, a.H, a.B), dim3(64), 0, stream, a);
  hipLaunchKernelGGL(attn_append_combine_kernel, dim3(a.H, a.T, a.B), dim3(64), 0, stream, a);
}

}  // namespace sdml

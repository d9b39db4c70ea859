// Single-token (decode) attention against a grouped KV cache (grouped-query attention; multi-query at Hkv = 1), bf16,
// head width 64 (models/gpt2.py decode_step with n_kv_head < n_head).
//
// H query heads share Hkv = H / G key/value heads: query head h reads kv head h / G. The new token's fused projection
// is qkv [B][64 H + 128 Hkv] = (q | k | v), the cache [B][Smax][Hkv][64] holds lens[b] earlier keys. The kernel writes
// the new k and v rows to cache index lens[b], once per (sample, kv head), and returns for every query head
//   softmax(q_h . K[0..lens[b]]^T * scale) . V[0..lens[b]]        over kv head h / G
//
// Work split: one wave per (sample, kv head, chunk of kAttnDecodeChunk keys). The chunk's K and V rows go to VGPRs
// once, with attention_decode.hip's lane map (16-byte pieces, eight lanes per row, all 8 + 8 loads issued ahead of
// the first use: 32 + 32 VGPRs), and then serve the group's G queries one after the other in a wave-uniform loop, the
// way attention_append.hip serves its T queries: attention_decode.hip would load every row G times. A query's row of
// qkv is read inside its iteration (2 VGPRs), not held for the whole group. One workspace slot per (sample, query
// head, chunk); the second launch is attention_decode.hip's chunk-order combine over the H query heads. No LDS, no
// atomics, no one-launch form.
//
// Bit contract: the output and the cache after the call are those of attention_decode.hip on the cache and qkv
// expanded to H heads. A (query head, chunk) runs attn_chunk.h's chunk_query on the same row registers with the same
// lane map and the same `last`, and the combine is the same kernel (tests/test_attention_gqa_gpu.py compares the
// raw bits).
//
// Keys past lens[b] never reach the result: their loads are redirected to the new token's own row, their scores and
// probabilities are selected away by chunk_query. Dead chunks (c * CH > lens[b]) return before any load. The chunk
// that holds index lens[b] owns the cache write and takes that key from qkv, through chunk_query's row hook in the
// group's first iteration, so no wave reads a row that another wave writes.
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "attn_chunk.h"

namespace sdml {
namespace {

using namespace attn_chunk;

// grid (chunks, Hkv, B), one wave per block. Lane l: piece l & 7 (channels 8 (l & 7) ..), row group l >> 3; its keys
// are chunk * CH + 8 i + (l >> 3), i = 0 .. RPL - 1. G: query heads per kv head (p.H = G Hkv).
template <int G>
__global__ void __launch_bounds__(64) attn_decode_gqa_chunk_kernel(AttnDecodeArgs p, int Hkv) {
  const int c = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const int len = p.lens[b];
  if (len < 0 || len >= p.Smax) return;  // (refused by the host API; never index outside the cache)
  if (c * CH > len) return;
  const int pc = lane & 7, rg = lane >> 3;
  const u16* row = static_cast<const u16*>(p.qkv) + (int64_t)b * p.ldq + 8 * pc;  // this lane's piece of head 0's q
  const u16* knew = row + (G + 0) * Hkv * 64 + kvh * 64;
  const u16* vnew = row + (G + 1) * Hkv * 64 + kvh * 64;
  const int64_t base = (int64_t)b * p.sb + (int64_t)kvh * p.sh + 8 * pc;
  u16* kc = static_cast<u16*>(p.k_cache) + base;
  u16* vc = static_cast<u16*>(p.v_cache) + base;

  // the chunk's rows, once for the group
  u16x8 kv[RPL], vv[RPL];
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg;
    kv[i] = *reinterpret_cast<const u16x8*>(j < len ? kc + (int64_t)j * p.ss : knew);
  }
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg;
    vv[i] = *reinterpret_cast<const u16x8*>(j < len ? vc + (int64_t)j * p.ss : vnew);
  }

  const int h0 = kvh * G;
#pragma unroll(G <= 4 ? G : 2)
  for (int g = 0; g < G; ++g) {  // (wave-uniform) the group's queries against the same registers
    float m, l, o[8];
    chunk_query(kv, vv, row + (h0 + g) * 64, c, len, p.scale, lane, m, l, o, [&](int i, int j) {
      if (g == 0 && j == len) {  // the new token's row, once per (sample, kv head): bit for bit from qkv
        *reinterpret_cast<u16x8*>(kc + (int64_t)j * p.ss) = kv[i];
        *reinterpret_cast<u16x8*>(vc + (int64_t)j * p.ss) = vv[i];
      }
    });
    store_slot(p.ws_ml, p.ws_o, ((int64_t)b * p.H + h0 + g) * p.max_chunks + c, lane, m, l, o);
  }
}

template <int G>
void launch(const AttnDecodeArgs& a, int Hkv, hipStream_t stream) {
  hipLaunchKernelGGL(attn_decode_gqa_chunk_kernel<G>, dim3(a.max_chunks, Hkv, a.B), dim3(64), 0, stream, a, Hkv);
}

}  // namespace

bool attention_decode_gqa_supported(int G) { return G == 2 || G == 3 || G == 4 || G == 6 || G == 12; }

void attention_decode_gqa_bf16(const AttnDecodeArgs& a, int Hkv, hipStream_t stream) {
  if (a.B <= 0 || a.H <= 0 || Hkv <= 0 || a.max_chunks <= 0 || a.H % Hkv) return;
  switch (a.H / Hkv) {  // (the binding refuses any other group size)
    case 2: launch<2>(a, Hkv, stream); break;
    case 3: launch<3>(a, Hkv, stream); break;
    case 4: launch<4>(a, Hkv, stream); break;
    case 6: launch<6>(a, Hkv, stream); break;
    case 12: launch<12>(a, Hkv, stream); break;
    default: return;
  }
  attention_decode_combine(a, stream);  // attention_decode.hip's: the H query heads' slots in chunk order
}

}  // namespace sdml

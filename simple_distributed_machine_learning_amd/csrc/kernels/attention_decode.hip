// Single-token (decode) attention against a KV cache, bf16, head width 64 (models/gpt2.py decode_step).
//
// For each (sample b, head h) the new token's q, k, v come from its fused projection qkv [B][3C]; the cache holds
// lens[b] earlier keys. The kernel writes the new k and v rows to cache index lens[b] and returns
//   softmax(q . K[0..lens[b]]^T * scale) . V[0..lens[b]]        (lens[b] + 1 keys, the new one included)
//
// Memory-bound: every K and V row is read once, so the rows go straight to VGPRs in 16-B pieces (a row is 8 lanes, a
// wave has 8 rows in flight per load and 8 + 8 loads outstanding); the products run on the VALU in fp32, which at one
// query per head is a few percent of the time of the loads. No LDS, no MFMA.
//
// Parallelism: B * H is far below the chip's wave slots, so the key range is cut into chunks of kAttnDecodeChunk keys
// (a compile-time constant, not derived from the batch), one wave each; a second launch combines the chunks'
// (max, sum, partial O) in chunk order. No atomics. A sample's result depends on its own row of qkv, its own cache
// rows and lens[b] only: the same bits on every run, in any batch.
//
// One-launch form (tickets): a row has nc = lens[b] / CH + 1 live chunks, known on the device. Each stores its slot
// write-through, draws a ticket on the (b, h) counter, and the wave that draws nc - 1 acquires at agent scope and runs
// the same combine in the same chunk order (handoff.h): the same bits, no second launch, and the grid may cover Smax.
// Nothing waits on a counter.
//
// Keys past lens[b] never reach the result: their loads are redirected to the new token's own row (so nothing is read
// from cache rows >= lens[b], which may hold anything), their scores and probabilities are selected away, not
// multiplied by zero. The chunk that contains index lens[b] owns the cache write, and takes that key from qkv, so no
// wave reads a row that another wave writes.
//
// The arithmetic of a chunk, the slot layout and the chunk-order combine are attn_chunk.h's, shared with
// attention_append.hip, whose queries get this kernel's bits by calling the same lines.
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "attn_chunk.h"
#include "handoff.h"

namespace sdml {
namespace {

using namespace attn_chunk;

__device__ __forceinline__ float lane_value(float x, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}

// attn_chunk.h's combine_chunks for slots that other workgroups wrote in this launch, behind the caller's acquire:
// every load of them bypasses the L1 (handoff.h), and since such a load is a round trip to the L2 or beyond, none
// depends on another. Lane c fetches chunk c's (m, l) and computes its weight, the partial outputs are fetched eight
// chunks at a time; each lane then runs combine_chunks' fmaf chain in chunk order on the same operands (the max is
// exact in any order): the same bits.
__device__ __forceinline__ void combine_handed_off(const AttnDecodeArgs& p, int b, int h, int nc, int lane) {
  const int64_t slot = ((int64_t)b * p.H + h) * p.max_chunks;
  const float* ml = p.ws_ml + slot * 2;
  const float* po = p.ws_o + slot * 64 + lane;
  float m0 = -INFINITY, l0 = 0.f;  // chunk `lane`
  if (lane < nc) handoff::ld_sc1_x2(ml + 2 * lane, m0, l0);
  float M = m0;
  for (int c = 64 + lane; c < nc; c += 64) M = fmaxf(M, handoff::ld_sc1(ml + 2 * c));
  M = wv::max64(M);
  float L = 0.f, O = 0.f;
  for (int c0 = 0; c0 < nc; c0 += 64) {
    float mc = m0, lc = l0;  // chunk c0 + lane
    if (c0 > 0) {
      mc = -INFINITY, lc = 0.f;
      if (c0 + lane < nc) handoff::ld_sc1_x2(ml + 2 * (c0 + lane), mc, lc);
    }
    const float w = __builtin_amdgcn_exp2f(mc - M);
    const int n = min(64, nc - c0);
    for (int j0 = 0; j0 < n; j0 += 8) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = handoff::ld_sc1(po + (int64_t)(c0 + min(j0 + j, n - 1)) * 64);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j0 + j < n) {
          const float wj = lane_value(w, j0 + j);
          L = fmaf(lane_value(lc, j0 + j), wj, L);
          O = fmaf(o[j], wj, O);
        }
    }
  }
  static_cast<u16*>(p.out)[(int64_t)b * p.H * 64 + h * 64 + lane] = f2bf(O / L);
}

// grid (chunks, H, B), one wave per block. Lane l: piece l & 7 (channels 8 (l & 7) ..), row group l >> 3; its keys
// are chunk * CH + 8 i + (l >> 3), i = 0 .. RPL - 1. TK: the one-launch form.
template <bool TK>
__global__ void __launch_bounds__(64) attn_decode_chunk_kernel(AttnDecodeArgs p) {
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const int len = p.lens[b];
  if (len < 0 || len >= p.Smax) return;  // (refused by the host API; never index outside the cache)
  if (c * CH > len) return;
  const int pc = lane & 7, rg = lane >> 3;
  const int C = p.H * 64;
  const u16* qrow = static_cast<const u16*>(p.qkv) + (int64_t)b * p.ldq + h * 64 + 8 * pc;
  const u16* knew = qrow + C;
  const u16* vnew = qrow + 2 * C;
  const int64_t base = (int64_t)b * p.sb + (int64_t)h * p.sh + 8 * pc;
  u16* kc = static_cast<u16*>(p.k_cache) + base;
  u16* vc = static_cast<u16*>(p.v_cache) + base;

  u16x8 kv[RPL], vv[RPL];
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg;
    const bool cached = j < len;
    kv[i] = *reinterpret_cast<const u16x8*>(cached ? kc + (int64_t)j * p.ss : knew);
  }
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 8 * i + rg;
    const bool cached = j < len;
    vv[i] = *reinterpret_cast<const u16x8*>(cached ? vc + (int64_t)j * p.ss : vnew);
  }
  float m, l, o[8];
  chunk_query(kv, vv, qrow, c, len, p.scale, lane, m, l, o, [&](int i, int j) {
    if (j == len) {  // the new token's row: bit for bit from qkv
      *reinterpret_cast<u16x8*>(kc + (int64_t)j * p.ss) = kv[i];
      *reinterpret_cast<u16x8*>(vc + (int64_t)j * p.ss) = vv[i];
    }
  });

  const int64_t slot = ((int64_t)b * p.H + h) * p.max_chunks + c;
  if constexpr (TK) {
    if (lane < 8) {
      float* dst = p.ws_o + slot * 64 + 8 * pc;
#pragma unroll
      for (int e = 0; e < 8; e += 2) handoff::st_sc1_x2(dst + e, o[e], o[e + 1]);
    }
    if (lane == 0) handoff::st_sc1_x2(p.ws_ml + slot * 2, m, l);
    // the slot went out write-through; draw a ticket on (b, h): the drawer of the last live chunk's combines
    int* counter = p.tickets + (int64_t)b * p.H + h;
    const bool mine = handoff::draw_ticket(counter) == len / CH;  // (lane 0's answer counts)
    handoff::acquire_partials(mine);  // one wave: the drawing lane's wait orders the wave's loads
    if (!__builtin_amdgcn_readfirstlane(mine)) return;
    combine_handed_off(p, b, h, len / CH + 1, lane);
    if (lane == 0) handoff::reset_ticket(counter);
  } else {
    store_slot(p.ws_ml, p.ws_o, slot, lane, m, l, o);
  }
}

// grid (H, B), one wave per block, lane = channel: the chunks of one (b, h) in chunk order
__global__ void __launch_bounds__(64) attn_decode_combine_kernel(AttnDecodeArgs p) {
  const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int len = p.lens[b];
  if (len < 0 || len >= p.Smax) return;
  const int nc = len / CH + 1;  // <= max_chunks: the host checked lens[b] + 1 <= n_keys
  if (nc > p.max_chunks) return;
  static_cast<u16*>(p.out)[(int64_t)b * p.H * 64 + h * 64 + lane] =
      combine_chunks(p.ws_ml, p.ws_o, ((int64_t)b * p.H + h) * p.max_chunks, nc, lane);
}

}  // namespace

int attention_decode_chunks(int n_keys) { return (n_keys + CH - 1) / CH; }

void attention_decode_bf16(const AttnDecodeArgs& a, hipStream_t stream) {
  if (a.B <= 0 || a.H <= 0 || a.max_chunks <= 0) return;
  if (a.tickets != nullptr) {  // one launch: the last live chunk of a (b, h) to arrive combines
    hipLaunchKernelGGL(attn_decode_chunk_kernel<true>, dim3(a.max_chunks, a.H, a.B), dim3(64), 0, stream, a);
    return;
  }
  hipLaunchKernelGGL(attn_decode_chunk_kernel<false>, dim3(a.max_chunks, a.H, a.B), dim3(64), 0, stream, a);
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(a.H, a.B), dim3(64), 0, stream, a);
}

}  // namespace sdml

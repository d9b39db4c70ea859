// Single-token (decode) attention against an fp4 (OCP microscaling e2m1) KV cache, head width 64:
// attention_decode_fp8.hip's semantics and liveness rules on rows of two MX blocks, 16 bytes of nibbles and one int8
// exponent each (kv_fp4.h: the format). The kernel streams 34 B per cached row where fp8 streams 66 B and bf16 128 B.
//
// For each (sample b, head h): the new token's q, k, v come from its fused projection qkv [B][3C] bf16. Its k and v are
// quantised in registers (kv_fp4.h quantize_block, the lines kv_quantize_fp4.hip runs), written to cache row lens[b],
// nibbles and exponents, and scored as the DEQUANTISED row: the result is the attention over the cache as later steps
// read it.
//
// Work split: two lanes hold a row, one MX block each, so a lane's 16-byte load is exactly one block and one load
// instruction of the wave covers 32 rows. Lane l holds block l & 1 of row group l >> 1; its keys in chunk c are
// c * 64 + 32 i + (l >> 1), i = 0, 1: a 64-key chunk is 2 loads of K and 2 of V per lane. The exponents lie as
// [B][H][Smax][2], so those of key j, block k are byte 2 j + k: lane l fetches byte 128 c + 64 i + l, its own, and a
// chunk's 128 exponents of an operand are one 128-byte line in two coalesced loads. No broadcast, no LDS, no atomics.
//
// Loads in flight: a chunk is only 2 KB of payload per operand pair, so a wave owns a run of `run` consecutive chunks
// of one (sample, head), grid (ceil(chunks / run), H, B), and issues the next chunk's four loads and exponent bytes
// before it computes the current one. Each chunk still writes its own attn_chunk.h slot, so the second launch
// (attention_decode.hip's combine, called, not copied) and the result's bits do not depend on the run length; the
// host picks it so that small grids still fill the CUs (run 1) and large ones keep two chunks in flight per wave.
//
// Arithmetic: v_cvt_scalef32_pk_f32_fp4 with the block's 2^e as its scale operand widens and scales at once, exactly
// (e2m1 * 2^e in fp32), so neither the score nor the probability is multiplied by a scale. A score is a 32-long fp32
// fma chain per lane in channel order and one DPP add between the row's two lanes (block 0 + block 1). Softmax, exp2,
// sums and the slot are fp32, no contraction: the products and sums are the ones written. The sums over the wave's 32
// row groups are DPP steps inside a row of 16 lanes and two permlane swaps across rows, symmetric in their operands.
//
// Keys at or past lens[b] other than the new one never reach the result and are not read, nibbles or exponents: their
// loads are redirected to the token's own q and what they return is replaced by zeros, their scores and
// probabilities are selected away, not multiplied by zero. The chunk that contains index lens[b] owns the cache write
// and takes that key from qkv, so no wave reads a row that another wave writes. A sample's bits depend on its own qkv
// row, its own cache rows and lens[b] only.
#include <hip/hip_runtime.h>

#include "attn_chunk.h"
#include "kv_fp4.h"

namespace sdml {
namespace {

using namespace kv_fp4;
using attn_chunk::CH;
using attn_chunk::f32x4;
using attn_chunk::kLog2e;

constexpr int RPL = CH / 32;  // rows per lane (2 lanes hold one row)
constexpr int ROR4 = 0x124, ROR8 = 0x128;  // DPP row_ror:4 / :8 inside a row of 16
constexpr int kMaxRun = 4;
// the waves that fill the device at 4 per SIMD (256 CUs x 4 SIMDs x 4): a longer run must leave at least these
constexpr int kFillWaves = 4096;
static_assert(CH == 64 && RPL == 2, "the lane map covers a 64-key chunk with two 16-byte loads per operand");

// sum / max over the 32 row groups of a wave (lane bits 1..5): the lanes that differ only in those bits hold the
// operands; every combine is symmetric, so every lane of a group ends with the same bits
__device__ __forceinline__ float sum_groups(float x) {
  x += wv::dpp<wv::XOR2>(x);
  x += wv::dpp<ROR8>(x);
  return wv::sum_rows(x + wv::dpp<ROR4>(x));
}
__device__ __forceinline__ float max_groups(float x) {
  x = fmaxf(x, wv::dpp<wv::XOR2>(x));
  x = fmaxf(x, wv::dpp<ROR8>(x));
  return wv::max_rows(fmaxf(x, wv::dpp<ROR4>(x)));
}

// the 8 channels of one 4-byte word of a block, times scale: four packed converts
__device__ __forceinline__ void widen_word(unsigned w, float scale, float (&x)[8]) {
  const f32x2 a = widen_fp4<0>(w, scale), b = widen_fp4<1>(w, scale);
  const f32x2 c = widen_fp4<2>(w, scale), d = widen_fp4<3>(w, scale);
  x[0] = a[0], x[1] = a[1], x[2] = b[0], x[3] = b[1], x[4] = c[0], x[5] = c[1], x[6] = d[0], x[7] = d[1];
}

// a chunk as the loads return it: this lane's blocks of its two rows and their exponent bytes
struct Chunk {
  u32x4 k[RPL], v[RPL];
  int ek[RPL], ev[RPL];
};

__global__ void __launch_bounds__(64) attn_decode_fp4_chunk_kernel(KvFp4Args p) {
#pragma clang fp contract(off)
  const int c0 = blockIdx.x * p.run, h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const int len = p.lens[b];
  if (len < 0 || len >= p.Smax) return;  // (refused by the host API; never index outside the cache)
  if (c0 * CH > len) return;
  const int cend = min(min(c0 + p.run, len / CH + 1), p.max_chunks);  // the run's chunks that hold a live key
  const int blk = lane & 1, rg = lane >> 1;
  const int C = p.H * 64, KB = p.H * 32;  // a key is KB bytes on
  const unsigned short* qrow = static_cast<const unsigned short*>(p.qkv) + (int64_t)b * p.ldq + h * 64 + 32 * blk;
  const int64_t row0 = ((int64_t)b * p.Smax * p.H + h) * 32 + 16 * blk;  // key 0's block
  unsigned char* kc = static_cast<unsigned char*>(p.k4) + row0;
  unsigned char* vc = static_cast<unsigned char*>(p.v4) + row0;
  signed char* kex = p.ke + ((int64_t)b * p.H + h) * p.Smax * 2 + lane;  // this lane's byte of key rg's pair
  signed char* vex = p.ve + ((int64_t)b * p.H + h) * p.Smax * 2 + lane;
  // A dead key's loads are redirected to the token's own q (valid memory that no wave writes) and what they return
  // is replaced by zeros before its use, so the loads need no branch and none waits for another.
  const unsigned char* dead = reinterpret_cast<const unsigned char*>(qrow);

  auto issue = [&](int c, Chunk& t) {
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
      const int j = c * CH + 32 * i + rg;
      t.k[i] = *reinterpret_cast<const u32x4*>(j < len ? kc + (int64_t)j * KB : dead);
    }
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
      const int j = c * CH + 32 * i + rg;
      t.v[i] = *reinterpret_cast<const u32x4*>(j < len ? vc + (int64_t)j * KB : dead);
    }
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
      const int j = c * CH + 32 * i + rg;
      t.ek[i] = *(j < len ? kex + 2 * (c * CH + 32 * i) : reinterpret_cast<const signed char*>(dead));
      t.ev[i] = *(j < len ? vex + 2 * (c * CH + 32 * i) : reinterpret_cast<const signed char*>(dead));
    }
  };

  Chunk cur;
  issue(c0, cur);
  float q[32];
  {
    const Bf16Block qb = load_block_bf16(qrow);
#pragma unroll
    for (int t = 0; t < 16; ++t) q[2 * t] = bf16_lo(qb.p[t / 4][t % 4]), q[2 * t + 1] = bf16_hi(qb.p[t / 4][t % 4]);
  }
  const float sl2 = p.scale * kLog2e;

  for (int c = c0; c < cend; ++c) {
    // (wave-uniform) The next chunk's loads fly while this one computes. The chunk that owns key lens[b] is the last
    // live one and has no next: it quantises the new k, v into the idle registers instead and writes the cache row.
    Chunk nxt;
    if (c + 1 < cend) {
      issue(c + 1, nxt);
    } else if (c == len / CH) {
      // (every lane pair computes the row; the one at key lens[b] keeps it)
      nxt.ek[0] = quantize_block(load_block_bf16(qrow + C), nxt.k[0]);
      nxt.ev[0] = quantize_block(load_block_bf16(qrow + 2 * C), nxt.v[0]);
      if (rg == len % 32) {
        *reinterpret_cast<u32x4*>(kc + (int64_t)len * KB) = nxt.k[0];
        *reinterpret_cast<u32x4*>(vc + (int64_t)len * KB) = nxt.v[0];
        kex[2 * len - 2 * rg] = (signed char)nxt.ek[0];  // byte 2 len + blk
        vex[2 * len - 2 * rg] = (signed char)nxt.ev[0];
      }
    }
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
      const int j = c * CH + 32 * i + rg;
      if (j >= len) cur.k[i] = cur.v[i] = u32x4{0, 0, 0, 0}, cur.ek[i] = cur.ev[i] = 0;
      if (j == len) cur.k[i] = nxt.k[0], cur.v[i] = nxt.v[0], cur.ek[i] = nxt.ek[0], cur.ev[i] = nxt.ev[0];
    }

    float x[8], s[RPL];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
      const int j = c * CH + 32 * i + rg;
      const float sc = pow2(cur.ek[i]);
      float a = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        widen_word(cur.k[i][w], sc, x);
#pragma unroll
        for (int t = 0; t < 8; ++t) a = fmaf(q[8 * w + t], x[t], a);
      }
      a += wv::dpp<wv::XOR1>(a);  // block 0 + block 1: the row's 2 lanes hold the same sum
      s[i] = j <= len ? a * sl2 : -INFINITY;
      m = fmaxf(m, s[i]);
    }
    m = max_groups(m);  // finite: key c * CH <= len is live

    float l = 0.f, o[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) o[t] = 0.f;
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
      const int j = c * CH + 32 * i + rg;
      const float pr = j <= len ? __builtin_amdgcn_exp2f(s[i] - m) : 0.f;
      l += pr;
      const float sc = pow2(cur.ev[i]);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        widen_word(cur.v[i][w], sc, x);
#pragma unroll
        for (int t = 0; t < 8; ++t) o[8 * w + t] = fmaf(pr, x[t], o[8 * w + t]);
      }
    }
    l = sum_groups(l);
    // (eight at a time: a permlane swap holds both its results, and the scheduler would otherwise keep all 32 sums'
    // pairs live at once and cost the kernel its fourth wave per SIMD)
#pragma unroll
    for (int t = 0; t < 32; ++t) {
      if (t % 8 == 0) __builtin_amdgcn_sched_barrier(0);
      o[t] = sum_groups(o[t]);
    }

    // attn_chunk.h's slot: the 64 partial outputs by the two lanes of row group 0, (m, l) by lane 0
    const int64_t slot = ((int64_t)b * p.H + h) * p.max_chunks + c;
    if (lane < 2) {
      f32x4* dst = reinterpret_cast<f32x4*>(p.ws_o + slot * 64 + 32 * blk);
#pragma unroll
      for (int t = 0; t < 8; ++t) dst[t] = f32x4{o[4 * t], o[4 * t + 1], o[4 * t + 2], o[4 * t + 3]};
    }
    if (lane == 0) {
      p.ws_ml[slot * 2] = m;
      p.ws_ml[slot * 2 + 1] = l;
    }
    cur = nxt;
  }
}

// the run length for a grid of B H max_chunks chunks: doubled while the launch still has kFillWaves waves
int default_run(int B, int H, int max_chunks) {
  int run = 1;
  while (run < kMaxRun && (int64_t)B * H * ((max_chunks + 2 * run - 1) / (2 * run)) >= kFillWaves) run *= 2;
  return run;
}

}  // namespace

void attention_decode_fp4(const KvFp4Args& a0, hipStream_t stream) {
  if (a0.B <= 0 || a0.H <= 0 || a0.max_chunks <= 0) return;
  KvFp4Args a = a0;
  a.run = min(a.run > 0 ? a.run : default_run(a.B, a.H, a.max_chunks), kMaxRun);
  hipLaunchKernelGGL(attn_decode_fp4_chunk_kernel, dim3((a.max_chunks + a.run - 1) / a.run, a.H, a.B), dim3(64), 0,
                     stream, a);
  AttnDecodeArgs cb;  // the chunk-order combine reads the slots, lens and the bounds; it touches no cache
  cb.out = a.out, cb.lens = a.lens, cb.ws_ml = a.ws_ml, cb.ws_o = a.ws_o;
  cb.B = a.B, cb.H = a.H, cb.Smax = a.Smax, cb.max_chunks = a.max_chunks;
  attention_decode_combine(cb, stream);
}

}  // namespace sdml

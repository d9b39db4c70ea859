// Single-token (decode) attention against an fp8 KV cache, head width 64: attention_decode.hip's semantics and
// liveness rules on rows of 64 e4m3 bytes with one int8 exponent each (kv_fp8.h: the format). The kernel streams 66 B
// per cached row where the bf16 kernel streams 128 B, which is what the step pays for at large batch x context.
//
// For each (sample b, head h): the new token's q, k, v come from its fused projection qkv [B][3C] bf16. Its k and v are
// quantised in registers (kv_fp8.h quantize_quad, the lines kv_quantize.hip runs), written to cache row lens[b], bytes
// and exponent, and scored as the DEQUANTISED row: the result is the attention over the cache as later steps read it.
//
// Work split: grid (chunks, H, B), one wave per 64-key chunk, as in attention_decode.hip; a chunk's (max, sum, partial
// O) goes to attn_chunk.h's slot and the second launch is attention_decode.hip's combine, called, not copied.
// Lane l holds piece l & 3 (channels 16 (l & 3) .., 16 bytes) of row group l >> 2; its keys are
// chunk * 64 + 16 i + (l >> 2), i = 0 .. 3. One 16-byte load per lane covers 16 rows per wave, so the chunk is 4 loads
// of K and 4 of V per lane, all issued ahead of the first use. The chunk's 64 exponents are one 64-byte load per
// operand: the lane with piece i fetches the byte of its quad's row i, and four quad broadcasts (DPP) hand each lane
// its four. No LDS, no atomics, no MFMA: the kernel is bound by the loads.
//
// Arithmetic: bytes widen with v_cvt_pk_f32_fp8 (exact). A score is a 16-long fp32 fma chain over the raw e4m3 values
// and the quad's two DPP adds; the row's 2^ek joins the score's scale * log2(e) (a power of two: exact), and 2^ev is
// applied once per row to the probability that multiplies V. Never per element. Softmax, exp2, sums and the slot are
// fp32, no contraction: the products and sums are the ones written.
//
// Keys at or past lens[b] other than the new one never reach the result and are not read, bytes or exponents: their
// loads are redirected to the token's own q and what they return is replaced by zeros, their scores and
// probabilities are selected away, not multiplied by zero. The chunk that contains index lens[b] owns the cache write
// and takes that key from qkv, so no wave reads a row that another wave writes. A sample's bits depend on its own qkv
// row, its own cache rows and lens[b] only.
#include <hip/hip_runtime.h>

#include "attn_chunk.h"
#include "kv_fp8.h"

namespace sdml {
namespace {

using namespace kv_fp8;
using attn_chunk::CH;
using attn_chunk::f32x4;
using attn_chunk::kLog2e;

constexpr int RPL = CH / 16;  // rows per lane (4 lanes hold one row)
constexpr int ROR4 = 0x124, ROR8 = 0x128;  // DPP row_ror:4 / :8 inside a row of 16
static_assert(CH == 64 && RPL == 4, "the lane map covers a 64-key chunk with four 16-byte loads per operand");

// quad_perm [I, I, I, I]: every lane of a quad gets the value of the quad's lane I
template <int I>
__device__ __forceinline__ int quad_bcast(int x) {
  return __builtin_amdgcn_update_dpp(0, x, I * 0x55, 0xf, 0xf, false);
}

// sum / max over the 16 row groups of a wave (lane bits 2..5): the lanes that differ only in those bits hold the
// operands; every combine is symmetric, so every lane of a group ends with the same bits
__device__ __forceinline__ float sum_groups(float x) {
  x += wv::dpp<ROR8>(x);
  return wv::sum_rows(x + wv::dpp<ROR4>(x));
}
__device__ __forceinline__ float max_groups(float x) {
  x = fmaxf(x, wv::dpp<ROR8>(x));
  return wv::max_rows(fmaxf(x, wv::dpp<ROR4>(x)));
}

// the lane's four row exponents from the byte it fetched (the lane with piece i holds row i's)
__device__ __forceinline__ void hand_exponents(int mine, int (&e)[RPL]) {
  e[0] = quad_bcast<0>(mine), e[1] = quad_bcast<1>(mine), e[2] = quad_bcast<2>(mine), e[3] = quad_bcast<3>(mine);
}

__global__ void __launch_bounds__(64) attn_decode_fp8_chunk_kernel(KvFp8Args p) {
#pragma clang fp contract(off)
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const int len = p.lens[b];
  if (len < 0 || len >= p.Smax) return;  // (refused by the host API; never index outside the cache)
  if (c * CH > len) return;
  const int pc = lane & 3, rg = lane >> 2;
  const int C = p.H * 64;
  const unsigned short* qrow = static_cast<const unsigned short*>(p.qkv) + (int64_t)b * p.ldq + h * 64 + 16 * pc;
  const int64_t row0 = ((int64_t)b * p.Smax * p.H + h) * 64 + 16 * pc;  // key 0's piece; a key is H * 64 bytes on
  unsigned char* kc = static_cast<unsigned char*>(p.k8) + row0;
  unsigned char* vc = static_cast<unsigned char*>(p.v8) + row0;
  signed char* kex = p.ke + ((int64_t)b * p.H + h) * p.Smax;
  signed char* vex = p.ve + ((int64_t)b * p.H + h) * p.Smax;

  // every load of the chunk ahead of its first use: 4 + 4 rows, the two exponent bytes, q. A dead key's loads are
  // redirected to the token's own q (valid memory that no wave writes) and what they return is replaced by zeros
  // below, so the loads need no branch and none waits for another.
  const unsigned char* dead = reinterpret_cast<const unsigned char*>(qrow);
  u32x4 kq[RPL], vq[RPL];
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 16 * i + rg;
    kq[i] = *reinterpret_cast<const u32x4*>(j < len ? kc + (int64_t)j * C : dead);
  }
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 16 * i + rg;
    vq[i] = *reinterpret_cast<const u32x4*>(j < len ? vc + (int64_t)j * C : dead);
  }
  const int jx = c * CH + 16 * pc + rg;  // the key whose exponents this lane fetches: row pc of its quad
  int kmine = *(jx < len ? kex + jx : reinterpret_cast<const signed char*>(dead));
  int vmine = *(jx < len ? vex + jx : reinterpret_cast<const signed char*>(dead));
  const u32x4 q0 = *reinterpret_cast<const u32x4*>(qrow);
  const u32x4 q1 = *reinterpret_cast<const u32x4*>(qrow + 8);
#pragma unroll
  for (int i = 0; i < RPL; ++i)
    if (c * CH + 16 * i + rg >= len) kq[i] = vq[i] = u32x4{0, 0, 0, 0};
  if (jx >= len) kmine = vmine = 0;
  int ek[RPL], ev[RPL];
  hand_exponents(kmine, ek);
  hand_exponents(vmine, ev);

  if (c == len / CH) {  // (wave-uniform) this chunk owns key lens[b]: quantise the new k, v and write the row
    const u32x4 k0 = *reinterpret_cast<const u32x4*>(qrow + C), k1 = *reinterpret_cast<const u32x4*>(qrow + C + 8);
    const u32x4 v0 = *reinterpret_cast<const u32x4*>(qrow + 2 * C);
    const u32x4 v1 = *reinterpret_cast<const u32x4*>(qrow + 2 * C + 8);
    float x[16];
    u32x4 kn, vn;
    widen_bf16(k0, k1, x);
    const int ekn = quantize_quad(x, kn);  // (every quad computes the row; the one at key lens[b] keeps it)
    widen_bf16(v0, v1, x);
    const int evn = quantize_quad(x, vn);
#pragma unroll
    for (int i = 0; i < RPL; ++i)
      if (c * CH + 16 * i + rg == len) {
        kq[i] = kn, vq[i] = vn, ek[i] = ekn, ev[i] = evn;
        *reinterpret_cast<u32x4*>(kc + (int64_t)len * C) = kn;
        *reinterpret_cast<u32x4*>(vc + (int64_t)len * C) = vn;
        if (pc == 0) kex[len] = (signed char)ekn, vex[len] = (signed char)evn;
      }
  }

  float q[16], x[16];
  widen_bf16(q0, q1, q);
  const float sl2 = p.scale * kLog2e;
  float s[RPL];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 16 * i + rg;
    widen_fp8(kq[i], x);
    float a = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) a = fmaf(q[t], x[t], a);
    a += wv::dpp<wv::XOR1>(a);
    a += wv::dpp<wv::XOR2>(a);  // the row's 4 lanes hold the same sum
    s[i] = j <= len ? a * (sl2 * pow2(ek[i])) : -INFINITY;
    m = fmaxf(m, s[i]);
  }
  m = max_groups(m);  // finite: key c * CH <= len is live

  float l = 0.f, o[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] = 0.f;
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int j = c * CH + 16 * i + rg;
    const float pr = j <= len ? __builtin_amdgcn_exp2f(s[i] - m) : 0.f;
    l += pr;
    const float pv = pr * pow2(ev[i]);  // (exact unless it underflows, where the term is below fp32's reach anyway)
    widen_fp8(vq[i], x);
#pragma unroll
    for (int t = 0; t < 16; ++t) o[t] = fmaf(pv, x[t], o[t]);
  }
  l = sum_groups(l);
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] = sum_groups(o[t]);

  // attn_chunk.h's slot: the 64 partial outputs by the four lanes of row group 0, (m, l) by lane 0
  const int64_t slot = ((int64_t)b * p.H + h) * p.max_chunks + c;
  if (lane < 4) {
    f32x4* dst = reinterpret_cast<f32x4*>(p.ws_o + slot * 64 + 16 * pc);
#pragma unroll
    for (int t = 0; t < 4; ++t) dst[t] = f32x4{o[4 * t], o[4 * t + 1], o[4 * t + 2], o[4 * t + 3]};
  }
  if (lane == 0) {
    p.ws_ml[slot * 2] = m;
    p.ws_ml[slot * 2 + 1] = l;
  }
}

}  // namespace

void attention_decode_fp8(const KvFp8Args& a, hipStream_t stream) {
  if (a.B <= 0 || a.H <= 0 || a.max_chunks <= 0) return;
  hipLaunchKernelGGL(attn_decode_fp8_chunk_kernel, dim3(a.max_chunks, a.H, a.B), dim3(64), 0, stream, a);
  AttnDecodeArgs cb;  // the chunk-order combine reads the slots, lens and the bounds; it touches no cache
  cb.out = a.out, cb.lens = a.lens, cb.ws_ml = a.ws_ml, cb.ws_o = a.ws_o;
  cb.B = a.B, cb.H = a.H, cb.Smax = a.Smax, cb.max_chunks = a.max_chunks;
  attention_decode_combine(cb, stream);
}

}  // namespace sdml

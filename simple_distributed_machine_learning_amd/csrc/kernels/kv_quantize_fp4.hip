// Prefill's write of an fp4 KV cache (kv_fp4.h: the format): the k and v of positions 0 .. S-1 of a layer's fused
// projection qkv [B][S][3C] bf16 become e2m1 nibbles k4 / v4 [B][Smax][H][32] and block exponents ke / ve
// [B][H][Smax][2], one launch for both operands. It stands where the bf16 cache has two strided copies.
//
// A row (sample, position, head) is a lane pair, one MX block of 32 channels per lane: the lane loads its 64 B of bf16
// as four 16-byte pieces (the pair reads the row's 128 contiguous bytes), takes the block's amax in-lane, derives the
// exponent from the bit fields, makes the nibbles with sixteen packed converts and stores its 16 bytes (the pair
// writes the row's 32 contiguous bytes). A block of 256 threads holds 128 consecutive positions of one (operand,
// sample, head): lane (position, block) owns exponent byte 2 position + block, so a wave's 64 exponent bytes are
// consecutive in [B][H][Smax][2] and go out as one 64-byte run. No LDS, no atomics, no cross-lane step.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kv_fp4.h"

namespace sdml {
namespace {

using namespace kv_fp4;

constexpr int kRowsPerBlock = 128;

// grid (ceil(S / 128), H, 2 B): blockIdx.z = 2 b + operand (0: k, 1: v)
__global__ void __launch_bounds__(2 * kRowsPerBlock) kv_quantize_rows_fp4_kernel(KvFp4Args p) {
  const int s = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 1), blk = threadIdx.x & 1;
  const int h = blockIdx.y, b = blockIdx.z >> 1, op = blockIdx.z & 1;
  if (s >= p.S) return;
  const int C = p.H * 64;
  const unsigned short* src = static_cast<const unsigned short*>(p.qkv) + (int64_t)b * p.sqb + (int64_t)s * p.ldq +
                              (1 + op) * C + h * 64 + 32 * blk;
  u32x4 q;
  const int e = quantize_block(load_block_bf16(src), q);
  unsigned char* bytes = static_cast<unsigned char*>(op ? p.v4 : p.k4);
  *reinterpret_cast<u32x4*>(bytes + (((int64_t)b * p.Smax + s) * p.H + h) * 32 + 16 * blk) = q;
  (op ? p.ve : p.ke)[(((int64_t)b * p.H + h) * p.Smax + s) * 2 + blk] = (signed char)e;
}

}  // namespace

void kv_quantize_rows_fp4(const KvFp4Args& a, hipStream_t stream) {
  if (a.B <= 0 || a.H <= 0 || a.S <= 0) return;
  hipLaunchKernelGGL(kv_quantize_rows_fp4_kernel, dim3((a.S + kRowsPerBlock - 1) / kRowsPerBlock, a.H, 2 * a.B),
                     dim3(2 * kRowsPerBlock), 0, stream, a);
}

}  // namespace sdml

// Prefill's write of an fp8 KV cache (kv_fp8.h: the format): the k and v of positions 0 .. S-1 of a layer's fused
// projection qkv [B][S][3C] bf16 become e4m3 bytes k8 / v8 [B][Smax][H][64] and exponents ke / ve [B][H][Smax], one
// launch for both operands. It stands where the bf16 cache has two strided copies.
//
// A row (sample, position, head) is a DPP quad: each lane loads 16 channels as two 16-byte pieces (the quad reads the
// row's 128 contiguous bytes), the quad's amax takes two DPP steps, and each lane stores its 16 bytes (the quad writes
// the row's 64 contiguous bytes). A block of 256 threads holds 64 consecutive positions of one (operand, sample, head),
// so a wave's 16 exponent bytes are consecutive in [B][H][Smax] and go out as one 16-byte run. No LDS, no atomics.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kv_fp8.h"

namespace sdml {
namespace {

using namespace kv_fp8;

constexpr int kRowsPerBlock = 64;

// grid (ceil(S / 64), H, 2 B): blockIdx.z = 2 b + operand (0: k, 1: v)
__global__ void __launch_bounds__(4 * kRowsPerBlock) kv_quantize_rows_kernel(KvFp8Args p) {
  const int s = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 2), pc = threadIdx.x & 3;
  const int h = blockIdx.y, b = blockIdx.z >> 1, op = blockIdx.z & 1;
  if (s >= p.S) return;  // (a quad leaves as one: the DPP steps stay inside a quad)
  const int C = p.H * 64;
  const unsigned short* src = static_cast<const unsigned short*>(p.qkv) + (int64_t)b * p.sqb + (int64_t)s * p.ldq +
                              (1 + op) * C + h * 64 + 16 * pc;
  const u32x4 lo = *reinterpret_cast<const u32x4*>(src);
  const u32x4 hi = *reinterpret_cast<const u32x4*>(src + 8);
  float x[16];
  widen_bf16(lo, hi, x);
  u32x4 q;
  const int e = quantize_quad(x, q);
  unsigned char* bytes = static_cast<unsigned char*>(op ? p.v8 : p.k8);
  *reinterpret_cast<u32x4*>(bytes + (((int64_t)b * p.Smax + s) * p.H + h) * 64 + 16 * pc) = q;
  if (pc == 0) (op ? p.ve : p.ke)[((int64_t)b * p.H + h) * p.Smax + s] = (signed char)e;
}

}  // namespace

void kv_quantize_rows_fp8(const KvFp8Args& a, hipStream_t stream) {
  if (a.B <= 0 || a.H <= 0 || a.S <= 0) return;
  hipLaunchKernelGGL(kv_quantize_rows_kernel, dim3((a.S + kRowsPerBlock - 1) / kRowsPerBlock, a.H, 2 * a.B),
                     dim3(4 * kRowsPerBlock), 0, stream, a);
}

}  // namespace sdml

// Primitives shared by the MFMA GEMM kernels (gemm_bf16.hip, gemm_f16x2.hip, gemm_bf16_wgrad.hip and wgrad_tiles.h;
// conv_bf16.hip, gemm_f32x3.hip, attention.hip and mlp_u8.hip use parts): vector types, the LDS-DMA instruction, the
// LDS image swizzles, the transposed LDS reads, and the two operand policies (bf16 and fp16) of the shared templates.
#pragma once

#include <hip/hip_runtime.h>

namespace sdml {

typedef unsigned short u16;
typedef short bf16x8 __attribute__((ext_vector_type(8)));  // MFMA operand: 8 x bf16 (bit patterns)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef u16 u16x4 __attribute__((ext_vector_type(4)));
typedef u16 u16x8 __attribute__((ext_vector_type(8)));

// LDS-DMA (global_load_lds_dwordx4): 16 B per lane from src, lane-linear into the wave's 1-KiB LDS block
__device__ __forceinline__ void glds16(const void* src, void* lds_block) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_block, 16, 0, 0);
}

// LDS images are lane-linear per DMA instruction, so the bank swizzles live on the per-lane SOURCE address (an
// involution applied again on the read).
//   [rows][64 k] images: 16-B chunk c of row r stored at c ^ rk_swz(r): the 16 rows of a ds_read_b128 lane group land
//     in 16 distinct 16-B bank slots (conflict-free)
//   [64 k][256 n] image: chunk c of k-row r at c ^ kn_swz(r): the 8 rows of a 32-lane half of the ds_read_b64_tr_b16
//     pair (k-rows q, q + 8 of the block) hit distinct 32-B slots
//   k-major [64 k][128 cols] images (u16 offsets): chunk ch of k-row k at km_off(k, ch): conflict-free transposed
//     reads and 16-B writes
__device__ __forceinline__ int rk_swz(int r) { return (r >> 1) & 7; }
__device__ __forceinline__ int kn_swz(int r) { return ((r & 3) | ((r >> 1) & 4)) << 1; }
__device__ __forceinline__ int km_off(int k, int ch) { return k * 128 + 8 * (ch ^ (((k & 3) << 2) | ((k >> 2) & 3))); }

// hardware transpose read (ds_read_b64_tr_b16) through the builtin: the compiler places its waits
__device__ __forceinline__ s16x4 ds_tr16(const void* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}

// The same read as inline assembly, for loops that keep LDS-DMA in flight across their fragment reads. Why asm: the
// compiler's wait pass puts an `s_waitcnt vmcnt(0)` (every LDS-DMA in flight, the prefetched K-steps included) in front
// of each __builtin_amdgcn_ds_read_tr16_b64 it cannot tell apart from the DMA stores, which serialises the ring. The
// asm reads are invisible to that pass, so their lgkmcnt waits are explicit (lgkm_wait): LDS returns in order, and the
// fragments are "+v" operands of the wait, so no MFMA moves above it.
__device__ __forceinline__ s16x4 ds_tr16_asm(const u16* p) {
  const unsigned a = (unsigned)(size_t)(const __attribute__((address_space(3))) u16*)p;
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(a));
  return v;
}

// wait until at most N LDS operations are outstanding; f = the half-fragments (6 or 8) that must have arrived
template <int N>
__device__ __forceinline__ void lgkm_wait(s16x4 (&f)[8]) {
  asm volatile("s_waitcnt lgkmcnt(%8)"
               : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7])
               : "n"(N));
}
template <int N>
__device__ __forceinline__ void lgkm_wait(s16x4 (&f)[6]) {
  asm volatile("s_waitcnt lgkmcnt(%6)"
               : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5])
               : "n"(N));
}

// two transposed-read halves -> one 8-element MFMA fragment (F = bf16x8 or f16x8)
template <typename F>
__device__ __forceinline__ F cat(s16x4 lo, s16x4 hi) {
  return __builtin_bit_cast(F, s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
}

// Operand policies: the fragment type and its MFMAs (16x16x32 for the output-tiled loops, 32x32x16 for the weight
// gradients), and how a stored element widens to float (the bias column sums of KmTile::store).
struct Bf16Ops {
  typedef bf16x8 frag;
  static __device__ __forceinline__ f32x4 mfma16(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x16 mfma32(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ float widen(u16 v) { return __uint_as_float(((unsigned)v) << 16); }
};
struct F16Ops {
  typedef f16x8 frag;
  static __device__ __forceinline__ f32x4 mfma16(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x16 mfma32(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ float widen(u16 v) { return static_cast<float>(__builtin_bit_cast(_Float16, v)); }
};

}  // namespace sdml

// Handing fp32 partials from one workgroup to another inside a launch (linear_decode.hip, attention_decode.hip: the
// one-launch forms). gfx950 has one L2 per XCD and they are not coherent with each other, and a CU's L1 is never
// refreshed by another CU's stores. The protocol, the same at both call sites:
//
//   writers   every partial goes out with a write-through (sc1) store, st_sc1 / st_sc1_x2, which needs no release
//             fence (an agent-scope release would write the whole L2 back, once per workgroup; measured several times
//             slower: docs/TUNING_NOTES.md "Graph-replayed decode") -> every storing wave waits vmcnt(0) ->
//             __syncthreads() -> one lane draws a ticket with a relaxed agent-scope fetch_add (draw_ticket)
//   reducer   the workgroup that draws the last ticket acquires at agent scope before any of its waves loads a
//             partial (acquire_partials: the drawing lane's fence, its vmcnt(0) wait, then the workgroup's barrier),
//             whatever else runs on its CU, and reads the partials with L1-bypassing (sc1) loads, ld_sc1 / ld_sc1_x2.
//             Dropping the acquire for sc1 loads alone is measured safe only at one workgroup per CU, which neither
//             call site is, so it stays.
//
// Nothing waits on a counter: a ticket is drawn once, and the workgroup reduces or exits.
#pragma once
#include <hip/hip_runtime.h>

namespace sdml {
namespace handoff {

__device__ __forceinline__ void st_sc1(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_sc1(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// two adjacent floats at an 8-byte aligned address, one 8-byte access
__device__ __forceinline__ void st_sc1_x2(float* p, float a, float b) {
  const unsigned long long v = ((unsigned long long)__float_as_uint(b) << 32) | __float_as_uint(a);
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ld_sc1_x2(const float* p, float& a, float& b) {
  const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
  a = __uint_as_float((unsigned)v);
  b = __uint_as_float((unsigned)(v >> 32));
}

// After the workgroup's partials are stored: drain this wave's stores, meet the other waves, then one lane draws.
// Returns the ticket in the drawing lane (thread 0 of the workgroup), -1 in every other lane.
__device__ __forceinline__ int draw_ticket(int* counter) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x != 0) return -1;
  return __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The drawing lane of the workgroup that drew the last ticket (`last`, meaningful in that lane only): the agent-scope
// acquire and its wait. The caller's barrier (for a one-wave workgroup the wait alone) then orders every wave's loads
// of the partials behind it.
__device__ __forceinline__ void acquire_partials(bool last) {
  if (threadIdx.x == 0 && last) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

__device__ __forceinline__ void reset_ticket(int* counter) {
  __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace handoff
}  // namespace sdml

// Counter-hash dropout masks of the GPT-2 kernels. A mask bit is a pure function of WHAT is dropped:
//   (seed, step counter, site, global layer, dataset index of the sample, global head, coordinates in the sample)
// and of nothing else (not of the micro-batch split, the pipeline placement or the tensor-parallel rank), so every
// schedule draws the same masks. The host twin is ops/reference.py (gpt2_dropout_*): the two agree bit for bit.
//
//   eff   = seed + 0x9E3779B97F4A7C15 * ctr                       (ref_cnn.hip's eff_seed; ctr: device step counter)
//   skey  = splitmix64(eff ^ (site << 32 | layer))                (64 bits)
//   rkey  = splitmix64(skey ^ (sample << 32 | head)) >> 32        (32 bits; once per wave or row, outside hot loops)
//   word  = fmix32(rkey ^ a * 0x9E3779B1 ^ (b >> 2) * 0x85EBCA77) (Murmur3's finaliser; one word per four b)
//   byte  = (word >> 8 (b & 3)) & 255;  keep iff byte >= T,  T = round(256 p) in 1..255
//   kept values are scaled by 256 / (256 - T) in fp32
// (a, b) = (query, key) for the attention probabilities, (position, channel) for the element-wise sites.
#pragma once
#include <hip/hip_runtime.h>

namespace sdml {

enum DropSite : unsigned { DROP_SITE_EMBD = 1, DROP_SITE_ATTN = 2, DROP_SITE_RESID_ATTN = 3, DROP_SITE_RESID_MLP = 4 };
// the sampler's noise (sample.hip) draws from the same hash: layer 0, head 0, a = position, b4 = vocabulary id
constexpr unsigned DROP_SITE_SAMPLE = 5;

__host__ __device__ __forceinline__ unsigned long long drop_splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__host__ __device__ __forceinline__ unsigned drop_fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__device__ __forceinline__ unsigned long long drop_eff_seed(unsigned long long seed, const long long* ctr) {
  return ctr ? seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(*ctr) : seed;
}
// site_layer = site << 16 | layer, as the launch arguments carry it
__host__ __device__ __forceinline__ unsigned long long drop_site_key(unsigned long long eff, unsigned site_layer) {
  return drop_splitmix64(eff ^ ((unsigned long long)(site_layer >> 16) << 32 | (site_layer & 0xFFFFu)));
}
__host__ __device__ __forceinline__ unsigned drop_row_key(unsigned long long skey, unsigned sample, unsigned head) {
  return (unsigned)(drop_splitmix64(skey ^ ((unsigned long long)sample << 32 | head)) >> 32);
}
// the word of coordinates (a, 4 b4 .. 4 b4 + 3)
__host__ __device__ __forceinline__ unsigned drop_word(unsigned rkey, unsigned a, unsigned b4) {
  return drop_fmix32(rkey ^ (a * 0x9E3779B1u) ^ (b4 * 0x85EBCA77u));
}
__host__ __device__ __forceinline__ unsigned drop_byte(unsigned word, unsigned e) { return (word >> (8 * e)) & 255u; }
__host__ __device__ __forceinline__ float drop_scale(unsigned T) { return 256.f / (float)(256u - T); }

// launch-side description of one dropout site (T == 0: off)
struct DropArgs {
  unsigned T = 0;                  // threshold, round(256 p)
  unsigned site_layer = 0;         // site << 16 | global layer
  unsigned long long seed = 0;     // the run's dropout seed
  const long long* ctr = nullptr;  // device step counter (may be null: counter 0)
  unsigned sample0 = 0;            // dataset index of the first sample of the call
  unsigned head0 = 0;              // global index of the first head of the call
};

}  // namespace sdml

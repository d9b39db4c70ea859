// Extend attention: T >= 1 new positions per sample against a KV cache plus themselves, bf16, head width 64
// (models/gpt2.py extend: chunked prefill and the catch-up of a generation session). These are attention_append.hip's
// semantics without its limit on T, on the training forward's arithmetic instead of the decode kernel's.
//
// qkv [B][T][3C] holds the chunk's fused projections (right-padded), the cache holds lens[b] earlier keys, nq[b] in
// 0 .. T of the sample's positions are live. Position t of sample b is live iff t < nq[b] and lens[b] + t < n_keys
// (the host's bound on the rows in use). A live position writes its k, v to cache row lens[b] + t, bit for bit from
// qkv, and returns
//   softmax(q_t . K[0..lens[b]+t]^T * scale) . V[0..lens[b]+t]
// A dead position writes no cache row and returns exact zeros. lens is not changed. No LSE: inference only.
//
// Two launches, no atomics. extend_rows_kernel copies the live rows into the cache; extend_attn_kernel, behind it in
// the stream, reads every key from the cache at its ABSOLUTE position: tiles of 64 keys from key 0 on, whatever
// lens[b] is. It is attention.hip's attn_fwd_kernel<64, 1> (S^T = K Q^T so each lane owns one query, the swizzled LDS
// tile image with double buffering, V^T by ds_read_b64_tr_b16) with the query taken from qkv, the keys from the
// cache, and the loop bound a uniform scalar read of lens[b], nq[b].
//
// Bit contract (docs/NUMERICS.md "Extend attention"): with cache rows [0, L_b) holding the bf16 k, v a full sequence
// holds there, output row (b, t) has the bits attention_fwd (causal, 64-key tiles, one query sub-block) gives
// position L_b + t of that sequence. A lane's result depends on its own query and the key tiles only: the MFMA
// computes each output column from that column's operand, and the two half-waves' partial max / sum meet in a
// commutative xor-32 exchange. So it is enough that a query sees the tiles 0, 64, 128, ... in order with the
// forward's operations (S over t = 0..3, mask by select, p = exp2(fma(s, scale log2e, -m)), P V over c, st, d, the
// final o * (1 / l) and bf16 round), and that a tile wholly masked for a query leaves its m, l, o unchanged bit for
// bit: mr = -inf, mx = m, alpha = exp2(0) = 1, p = exp2(-inf) = 0, and every query has seen key 0, so m is finite
// after the first tile. The forward skips such tiles per wave or masks them; here the waves are aligned to t, not to
// the absolute position, so the masked form covers what the forward would have skipped.
//
// Rows at or past the sample's last live row are never used as data (they may hold NaN): tile loads clamp to that
// row, so a masked P = 0 only ever meets finite V.
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "attn_tile.h"
#include "kernels.h"
#include "mma_prims.h"

namespace sdml {
namespace {

using namespace attn_tile;

constexpr int QW = 32;       // queries per wave
constexpr int NW = 4;        // waves per workgroup
constexpr int QB = QW * NW;  // new positions per workgroup
constexpr int KB = 64;       // keys per tile
constexpr int NTH = 64 * NW;

// live positions of sample b given its length (attention_append.hip live_queries): t < nq[b], and row len + t inside
// the host's bound, so inside the cache. 0 for a length outside the cache.
__device__ __forceinline__ int live_positions(const AttnExtendArgs& p, int b, int len) {
  if (len < 0 || len >= p.n_keys) return 0;
  return max(0, min(min(p.nq[b], p.T), p.n_keys - len));
}

// grid (T, B), 64 threads: the k and v of live position t to cache row lens[b] + t, 16 bytes per thread and trip
__global__ void __launch_bounds__(64) extend_rows_kernel(AttnExtendArgs p) {
  const int t = blockIdx.x, b = blockIdx.y;
  const int len = p.lens[b];
  if (t >= live_positions(p, b, len)) return;
  const int C = p.H * HD;
  const u16* src = static_cast<const u16*>(p.qkv) + ((long)b * p.T + t) * p.ldq + C;
  const long row = (long)b * p.sb + (long)(len + t) * p.ss;  // len + t < n_keys <= Smax
  u16* kc = static_cast<u16*>(p.k_cache) + row;
  u16* vc = static_cast<u16*>(p.v_cache) + row;
  for (int i = threadIdx.x; i < p.H * 8; i += 64) {  // chunk i & 7 of head i >> 3
    const long dst = (long)(i >> 3) * p.sh + 8 * (i & 7);
    *reinterpret_cast<u16x8*>(kc + dst) = *reinterpret_cast<const u16x8*>(src + 8 * i);
    *reinterpret_cast<u16x8*>(vc + dst) = *reinterpret_cast<const u16x8*>(src + C + 8 * i);
  }
}

// one workgroup = 4 waves = 128 new positions of one (sample, head); wave = 32 positions, one per lane column
__global__ void __launch_bounds__(NTH, 2) extend_attn_kernel(AttnExtendArgs p) {
  __shared__ __attribute__((aligned(16))) u16 Ks[2][KB * HD];
  __shared__ __attribute__((aligned(16))) u16 Vs[2][KB * HD];
  const int nqb = (p.T + QB - 1) / QB;
  const int blk = xcd_block(blockIdx.x, gridDim.x);
  const int bh = blk / nqb;
  const int qb = nqb - 1 - (blk % nqb);  // heaviest blocks first
  const int b = bh / p.H, hh = bh % p.H;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 31,
            h = lane >> 5;
  const int len = __builtin_amdgcn_readfirstlane(p.lens[b]);
  const int n = __builtin_amdgcn_readfirstlane(live_positions(p, b, len));
  const int t0 = qb * QB, tw = t0 + w * QW;  // the block's and this wave's first new position
  const int ti = tw + r;                     // this lane's new position
  u16* O = static_cast<u16*>(p.out) + (((long)b * p.T + ti) * p.H + hh) * HD;
  if (t0 >= n) {  // nothing live in this block (uniform): zeros
    if (ti < p.T) {
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) *reinterpret_cast<u16x4*>(O + 32 * d + 8 * g + 4 * h) = u16x4{0, 0, 0, 0};
    }
    return;
  }
  const int last = len + n - 1;  // the sample's last live row: < n_keys <= Smax, written by extend_rows_kernel
  const int qpos = len + ti;     // this lane's absolute position (live lanes: <= last)
  // Q fragments (B operand of S^T = K Q^T): element j = Q[ti][16t + 8h + j]; a dead lane carries zeros
  bf16x8 qf[4];
  {
    const u16* Q = static_cast<const u16*>(p.qkv) + ((long)b * p.T + ti) * p.ldq + hh * HD;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (ti < n) qf[t] = *reinterpret_cast<const bf16x8*>(Q + 16 * t + 8 * h);
      else qf[t] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  const long coff = (long)b * p.sb + (long)hh * p.sh;
  const u16* K = static_cast<const u16*>(p.k_cache) + coff;
  const u16* V = static_cast<const u16*>(p.v_cache) + coff;
  const float sl2 = p.scale * LOG2E;
  float m = -INFINITY, l = 0.f;
  f32x16 o[2];  // O^T[d][q]: d tile 0..1
  o[0] = o[1] = zero16();
  const int kend = len + min(t0 + QB, n);  // one past the block's last live key
  const bool wave_live = tw < n;           // (uniform) a wave of dead positions only loads tiles
  TileRegs<KB, NTH> kr, vr;
  tile_load_clamped(kr, K, p.ss, 0, last + 1);
  tile_load_clamped(vr, V, p.ss, 0, last + 1);
  tile_store(Ks[0], kr);
  tile_store(Vs[0], vr);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < kend; k0 += KB, buf ^= 1) {
    const bool more = k0 + KB < kend;
    if (more) {  // next tile's loads fly during this tile's MFMAs
      tile_load_clamped(kr, K, p.ss, k0 + KB, last + 1);
      tile_load_clamped(vr, V, p.ss, k0 + KB, last + 1);
    }
    if (wave_live && k0 <= len + tw + QW - 1) {  // else: all this wave's positions precede k0
      const u16* Kt = Ks[buf];
      const u16* Vt = Vs[buf];
      f32x16 s[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        s[c] = zero16();
#pragma unroll
        for (int t = 0; t < 4; ++t) s[c] = mfma(rowf(Kt, 32 * c + r, t, h), qf[t], s[c]);
      }
      // mask (tiles that reach past the wave's first position) by compare + select; a dead lane of a live wave is
      // held to the last live row, so it sees finite rows only
      if (k0 + KB - 1 > len + tw) {
        const int lim = min(qpos, last) - (k0 + 4 * h);  // last key this lane may see
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int i = 0; i < 16; ++i) s[c][i] = (32 * c + (i & 3) + 8 * (i >> 2) > lim) ? -INFINITY : s[c][i];
      }
      float mr = -INFINITY;
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) mr = fmaxf(mr, s[c][i]);
      mr = fmaxf(mr, __shfl_xor(mr, 32));
      const float mx = fmaxf(m, mr * sl2);  // running max, log2 domain
      const float alpha = (m == -INFINITY) ? 0.f : ex2(m - mx);
      const float msub = (mx == -INFINITY) ? 0.f : mx;
      float rs = 0.f;
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float pr = ex2(__builtin_fmaf(s[c][i], sl2, -msub));
          s[c][i] = pr;
          rs += pr;
        }
      rs += __shfl_xor(rs, 32);
      l = l * alpha + rs;
      m = mx;
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[d][i] *= alpha;
      // O^T[d][q] += sum_k V^T[d][k] P^T[k][q]
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          const bf16x8 pb = pack8(s[c], st);
#pragma unroll
          for (int d = 0; d < 2; ++d) o[d] = mfma(trf(Vt, 32 * c + 16 * st, 32 * d, lane), pb, o[d]);
        }
    }
    if (more) {
      tile_store(Ks[buf ^ 1], kr);
      tile_store(Vs[buf ^ 1], vr);
    }
    __syncthreads();
  }
  if (ti >= p.T) return;
  const float inv = (ti < n && l > 0.f) ? 1.f / l : 0.f;
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u16x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ti < n ? f2bf(o[d][4 * g + e] * inv) : (u16)0;
      *reinterpret_cast<u16x4*>(O + 32 * d + 8 * g + 4 * h) = v;
    }
}

}  // namespace

void attention_extend_bf16(const AttnExtendArgs& a, hipStream_t stream) {
  if (a.B <= 0 || a.H <= 0 || a.T <= 0) return;
  hipLaunchKernelGGL(extend_rows_kernel, dim3(a.T, a.B), dim3(64), 0, stream, a);
  const int nqb = (a.T + QB - 1) / QB;
  hipLaunchKernelGGL(extend_attn_kernel, dim3(nqb * a.H * a.B), dim3(NTH), 0, stream, a);
}

}  // namespace sdml

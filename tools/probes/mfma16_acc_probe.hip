// Numerics probe for the uint8 forward's MFMA shape: the fp32 accumulation of v_mfma_f32_16x16x32_f16 against
// v_mfma_f32_32x32x16_f16 (mfma_acc_probe.hip measured only the bf16 32x32x16 form). Operands as in mlp_u8.hip: random
// pixel bytes (exact in fp16) against the two fp16 planes of W * 2^8 (hi = fp16(256 w), lo = fp16(256 w - hi)), one
// straight chain per output, lo plane first at every k-substep. Compared with fp64 and with a host fp32 fmaf chain in
// k order (hi then lo at every k: tests/mlp_numerics.py's chain model), K = 784 and 4096.
//   hipcc --offload-arch=gfx950 -O3 mfma16_acc_probe.hip -o probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// X [32][Kp] bytes, Whi / Wlo [32][Kp] fp16 (zero past K); C32 / C16 [32][32]
__global__ void probe(const unsigned char* X, const _Float16* Whi, const _Float16* Wlo, int Kp, float* C32, float* C16) {
  const int l = threadIdx.x;
  {  // 32x32x16: lane (r, h) holds row / column r, k = 16 s + 8 h + j
    const int r = l & 31, h = l >> 5;
    f32x16 acc = {};
    for (int k0 = 0; k0 < Kp; k0 += 16) {
      f16x8 a, bh, bl;
      for (int j = 0; j < 8; ++j) {
        const int k = k0 + 8 * h + j;
        a[j] = (_Float16)(float)X[r * Kp + k];
        bh[j] = Whi[r * Kp + k];
        bl[j] = Wlo[r * Kp + k];
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bh, acc, 0, 0, 0);
    }
    for (int i = 0; i < 16; ++i) C32[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = acc[i];
  }
  {  // 16x16x32: lane (r, g) holds row / column r, k = 32 s + 8 g + j; 2 x 2 tiles
    const int r = l & 15, g = l >> 4;
    for (int ti = 0; ti < 2; ++ti)
      for (int tj = 0; tj < 2; ++tj) {
        f32x4 acc = {};
        for (int k0 = 0; k0 < Kp; k0 += 32) {
          f16x8 a, bh, bl;
          for (int j = 0; j < 8; ++j) {
            const int k = k0 + 8 * g + j;
            a[j] = (_Float16)(float)X[(16 * ti + r) * Kp + k];
            bh[j] = Whi[(16 * tj + r) * Kp + k];
            bl[j] = Wlo[(16 * tj + r) * Kp + k];
          }
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bl, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bh, acc, 0, 0, 0);
        }
        for (int v = 0; v < 4; ++v) C16[(16 * ti + 4 * g + v) * 32 + 16 * tj + r] = acc[v];
      }
  }
}

int main() {
  const int Ks[2] = {784, 4096};
  for (int K : Ks) {
    const int Kp = (K + 31) / 32 * 32;
    std::mt19937 gen(99 + K);
    std::uniform_int_distribution<int> B(0, 255);
    std::normal_distribution<float> Nw(0.f, 0.05f);
    std::vector<unsigned char> X(32 * Kp, 0);
    std::vector<_Float16> Whi(32 * Kp, (_Float16)0.f), Wlo(32 * Kp, (_Float16)0.f);
    for (int i = 0; i < 32; ++i)
      for (int k = 0; k < K; ++k) {
        X[i * Kp + k] = (unsigned char)B(gen);
        const float s = Nw(gen) * 256.f;
        const _Float16 hi = (_Float16)s;
        Whi[i * Kp + k] = hi;
        Wlo[i * Kp + k] = (_Float16)(s - (float)hi);
      }
    unsigned char* dX;
    _Float16 *dH, *dL;
    float *d32, *d16;
    if (hipMalloc(&dX, X.size()) != hipSuccess) return 1;
    (void)hipMalloc(&dH, Whi.size() * 2);
    (void)hipMalloc(&dL, Wlo.size() * 2);
    (void)hipMalloc(&d32, 4096);
    (void)hipMalloc(&d16, 4096);
    (void)hipMemcpy(dX, X.data(), X.size(), hipMemcpyHostToDevice);
    (void)hipMemcpy(dH, Whi.data(), Whi.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(dL, Wlo.data(), Wlo.size() * 2, hipMemcpyHostToDevice);
    probe<<<1, 64>>>(dX, dH, dL, Kp, d32, d16);
    std::vector<float> C32(1024), C16(1024);
    if (hipMemcpy(C32.data(), d32, 4096, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    (void)hipMemcpy(C16.data(), d16, 4096, hipMemcpyDeviceToHost);
    double e[3] = {0, 0, 0}, rms[3] = {0, 0, 0}, bias[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    for (int i = 0; i < 32; ++i)
      for (int j = 0; j < 32; ++j) {
        double ex = 0, mag = 0;
        float f = 0.f;
        for (int k = 0; k < K; ++k) {
          const float x = X[i * Kp + k], hi = (float)Whi[j * Kp + k], lo = (float)Wlo[j * Kp + k];
          ex += (double)x * hi + (double)x * lo;
          mag += fabs((double)x * hi);
          f = fmaf(x, hi, f);
          f = fmaf(x, lo, f);
        }
        const double got[3] = {C32[i * 32 + j], C16[i * 32 + j], f};
        for (int t = 0; t < 3; ++t) {
          const double d = (got[t] - ex) / mag;
          e[t] += fabs(d) / 1024;
          rms[t] += d * d / 1024;
          bias[t] += d / 1024;
          mx[t] = fmax(mx[t], fabs(d));
        }
      }
    const char* nm[3] = {"32x32x16 chain", "16x16x32 chain", "host fmaf chain"};
    for (int t = 0; t < 3; ++t)
      printf("K=%5d  %-16s mean %.3g rms %.3g max %.3g bias %+.3g  (relative to sum|x*w|)\n", K, nm[t], e[t],
             sqrt(rms[t]), mx[t], bias[t]);
    (void)hipFree(dX);
    (void)hipFree(dH);
    (void)hipFree(dL);
    (void)hipFree(d32);
    (void)hipFree(d16);
  }
  return 0;
}

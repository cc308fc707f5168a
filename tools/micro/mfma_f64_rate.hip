// Rate of v_mfma_f64_16x16x4_f64, the instruction behind sdy_member_gram (csrc/member_gram.hip): back-to-back on register
// operands, no memory traffic, with 1 / 2 / 4 / 8 independent accumulators (1: the dependent-accumulator latency; 8: the
// issue interval) and one or two waves per SIMD.  Build + run on the GPU box:
//   make -C tools/micro mfma_f64_rate && tools/micro/mfma_f64_rate
// Prints the time per instruction and SIMD in ns and in cycles of the clock that v_mfma_f32_32x32x16_f16 (8 passes = 32
// cycles per instruction, NOTEBOOK.md section 2) shows in the same process.
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int NACC>
__global__ void k64(double* out, int iters) {
  const double a = threadIdx.x * 0.001 + 1.0, b = 0.01 * (threadIdx.x & 15);
  f64x4 acc[NACC];
  for (int i = 0; i < NACC; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
  }
  double s = 0.0;
  for (int i = 0; i < NACC; ++i) for (int r = 0; r < 4; ++r) s += acc[i][r];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

__global__ void k16(double* out, int iters) {
  f16x8 a, b;
  for (int e = 0; e < 8; ++e) { a[e] = (_Float16)(threadIdx.x * 0.001f + e); b[e] = (_Float16)(e * 0.01f); }
  f32x16 acc[4];
  for (int i = 0; i < 4; ++i) for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[i], 0, 0, 0);
  }
  float s = 0.f;
  for (int i = 0; i < 4; ++i) for (int r = 0; r < 16; ++r) s += acc[i][r];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <class K>
static float timed(K kernel, int threads, double* out, int iters) {
  float best = 1e30f;
  for (int rep = 0; rep < 3; ++rep) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0);
    hipLaunchKernelGGL(kernel, dim3(256), dim3(threads), 0, 0, out, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    if (rep > 0 && ms < best) best = ms;
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  return best;
}

int main() {
  double* out;
  if (hipMalloc(&out, 256 * 1024 * sizeof(double)) != hipSuccess) { printf("no device\n"); return 1; }
  const int iters = 20000;
  // the clock: 256 threads per CU = one wave per SIMD, 4 independent accumulators, 32 cycles per instruction
  const float ms16 = timed(k16, 256, out, iters);
  const double ghz = (double)iters * 4 * 32 / ms16 * 1e-6;
  printf("clock by v_mfma_f32_32x32x16_f16 at 32 cycles: %.3f GHz (%.3f ms)\n", ghz, ms16);
  for (int threads : {256, 512}) {
    const int waves = threads / 256;   // per SIMD
    const float ms[4] = {timed(k64<1>, threads, out, iters), timed(k64<2>, threads, out, iters),
                         timed(k64<4>, threads, out, iters), timed(k64<8>, threads, out, iters)};
    const int nacc[4] = {1, 2, 4, 8};
    for (int j = 0; j < 4; ++j) {
      const double per = ms[j] * 1e6 / ((double)iters * nacc[j] * waves);   // ns per instruction and SIMD
      printf("v_mfma_f64_16x16x4_f64, %d wave(s)/SIMD, %d accumulator(s): %.3f ms, %.2f ns = %.1f cycles per instruction and "
             "SIMD, %.1f TFLOP/s on 256 CUs\n", waves, nacc[j], ms[j], per, per * ghz,
             2048.0 * iters * nacc[j] * waves * 1024 / ms[j] * 1e-9);
    }
  }
  hipFree(out);
  return 0;
}

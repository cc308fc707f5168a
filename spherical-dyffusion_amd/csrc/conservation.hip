// Dry-air conservation diagnostics (compute_dry_air_absolute_differences, core/aggregator/climate_data.py; ConservationLoss,
// core/loss.py; DryAir, core/aggregator/one_step/derived.py), gfx950: reduce -> combine, two launches whatever the batch, the
// number of times and the level count.  HBM-bound streaming: the reduce pass reads every plane once (K water levels, the
// pressure, the weights from L2) and forms the column quantity with the corrector's fp32 chain (corrector_math.h).  Sums:
// float64, one partial pair per (sample, time, 1024-column chunk) in the workspace; one small block then adds a row's partials
// in chunk order, the samples in sample order and the times in time order.  No atomics.  The host entry point walks the same
// tree (four columns per thread in order, the wave butterfly, the four waves in order), so it gives the device's bits.
#include <vector>

#include "common.h"
#include "corrector_math.h"
#include "ordered_sum.h"

namespace {

constexpr int kThreads = 256;
constexpr int kColsPerThread = 4;
constexpr int kChunk = kThreads * kColsPerThread;   // columns of one workgroup: the partition of the sums, fixed
constexpr int kWaves = kThreads / 64;
constexpr int kCombineThreads = 256;

int n_chunks(int HW) { return (HW + kChunk - 1) / kChunk; }

// one column's contribution: w and w * dry, both float64, never contracted
SDY_CORR_HD void dry_air_accumulate(float w, float dry, double* acc_w, double* acc_d) {
#pragma clang fp contract(off)
  const double wd = (double)w;
  *acc_w += wd;
  *acc_d += wd * (double)dry;
}

// the thread's 4 neighbouring columns p .. p+3 of row (b, t); the entry point made sure that every plane takes 16-byte loads
__device__ __forceinline__ f32x4 load_cols(const sdy_dry_air_var& v, int b, int t, int p) {
  f32x4 x = *reinterpret_cast<const f32x4*>(v.base + (long)b * v.stride_b + (long)t * v.stride_t + p);
#pragma unroll
  for (int c = 0; c < kColsPerThread; ++c) x[c] = sdy_corr_denorm(x[c], v.mean, v.std);
  return x;
}

// grid (chunks, B*T).  Every variable's planes have been moved to their channel by the entry point (channel == 0 here).
template <int K>
__global__ __launch_bounds__(kThreads) void dry_air_reduce_kernel(const sdy_dry_air_args a, double* partials) {
  const int row = blockIdx.y, HW = a.HW;
  const int b = row / a.T, t = row - b * a.T;
  const int p = (blockIdx.x * kThreads + threadIdx.x) * kColsPerThread;
  double acc_w = 0.0, acc_d = 0.0;
  if (p < HW) {   // HW % 4 == 0: p < HW covers all four columns
    const f32x4 w = *reinterpret_cast<const f32x4*>(a.area + p);
    f32x4 q[K];
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = load_cols(a.q[k], b, t, p);
    const f32x4 ps = load_cols(a.ps, b, t, p);
#pragma unroll
    for (int c = 0; c < kColsPerThread; ++c) {
      const float twp = sdy_corr_twp(sdy_corr_dp_q(K, a.ak, a.bk, ps[c], [&](int k) { return q[k][c]; }));
      dry_air_accumulate(w[c], sdy_corr_dry(ps[c], twp), &acc_w, &acc_d);
    }
  }
  // wave butterfly, then the four waves in order: the same tree for every chunk of every row
  __shared__ double sh[kWaves][2];
  sdy_wave_sum(acc_w, acc_d);
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6][0] = acc_w;
    sh[threadIdx.x >> 6][1] = acc_d;
  }
  __syncthreads();
  if (threadIdx.x < 2) partials[((size_t)row * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = sdy_fold_rows(sh, threadIdx.x);
}

// the three combines, shared by the one-block kernel and the host entry point
SDY_CORR_HD double dry_air_row_mean(const double* partials, int row, int chunks) {
#pragma clang fp contract(off)
  double s[2];   // sum of w, sum of w * dry
  sdy_sum_chunks(partials + (size_t)row * chunks * 2, chunks, 2, 0, s);
  return s[1] / s[0];
}
SDY_CORR_HD double dry_air_absdiff(const double* gm, int B, int T, int t) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += fabs(gm[(size_t)b * T + t + 1] - gm[(size_t)b * T + t]);
  return s / (double)B;
}
SDY_CORR_HD double dry_air_mean(const double* absdiff, int T) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int t = 0; t < T - 1; ++t) s += absdiff[t];
  return s / (double)(T - 1);
}

// one block: rows, then times, then the mean; each stage reads what the stage before wrote (block-wide barrier in between)
__global__ __launch_bounds__(kCombineThreads) void dry_air_combine_kernel(const double* partials, int B, int T, int chunks,
                                                                          int accumulate, double* gm, double* absdiff,
                                                                          double* mean_absdiff) {
  for (int row = threadIdx.x; row < B * T; row += kCombineThreads) gm[row] = dry_air_row_mean(partials, row, chunks);
  if (T < 2) return;
  __threadfence_block();
  __syncthreads();
  for (int t = threadIdx.x; t < T - 1; t += kCombineThreads) absdiff[t] = dry_air_absdiff(gm, B, T, t);
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) {
    const double m = dry_air_mean(absdiff, T);
    mean_absdiff[0] = accumulate ? mean_absdiff[0] + m : m;
  }
}

template <int K>
int launch_dry_air(const sdy_dry_air_args& a, hipStream_t stream) {
  if (a.K != K) return launch_dry_air<K - 1>(a, stream);
  const int chunks = n_chunks(a.HW);
  double* partials = static_cast<double*>(a.ws);
  hipLaunchKernelGGL(dry_air_reduce_kernel<K>, dim3(chunks, a.B * a.T), dim3(kThreads), 0, stream, a, partials);
  SDY_TRY(sdy_launch_status());
  hipLaunchKernelGGL(dry_air_combine_kernel, dim3(1), dim3(kCombineThreads), 0, stream, partials, a.B, a.T, chunks,
                     a.accumulate, a.gm, a.absdiff, a.mean_absdiff);
  return sdy_launch_status();
}
template <>
int launch_dry_air<0>(const sdy_dry_air_args&, hipStream_t) {
  return SDY_ERR_ARG;
}

// Everything that bounds an address, for the device and the host entry point alike.  On success *r is the argument block with
// every plane moved to its channel (channel = 0).
int check_args(const sdy_dry_air_args* a, bool need_ws, sdy_dry_air_args* r) {
  if (!a || a->B < 1 || a->T < 1 || a->HW < 1 || (a->HW & 3)) return SDY_ERR_ARG;
  if (a->K < 1 || a->K > SDY_DERIVED_MAX_LEVELS) return SDY_ERR_ARG;
  if (!a->area || ((uintptr_t)a->area & 15)) return SDY_ERR_ARG;
  if (!a->gm || ((uintptr_t)a->gm & 7)) return SDY_ERR_ARG;
  if (a->T > 1 && (!a->absdiff || ((uintptr_t)a->absdiff & 7) || !a->mean_absdiff || ((uintptr_t)a->mean_absdiff & 7)))
    return SDY_ERR_ARG;
  if ((long)a->B * a->T > 65535) return SDY_ERR_UNSUPPORTED;
  if (need_ws && !sdy_ws_ok(a->ws, a->ws_bytes, sdy_dry_air_workspace_bytes(a->B, a->T, a->HW))) return SDY_ERR_ARG;
  *r = *a;
  bool ok = true;
  auto use_var = [&](sdy_dry_air_var& v) {
    if (!v.base || v.channel < 0 || v.stride_b < 0 || v.stride_t < 0 || (v.stride_b & 3) || (v.stride_t & 3) ||
        !(std::isfinite(v.mean) && std::isfinite(v.std) && v.std > 0.f)) {
      ok = false;
      return;
    }
    v.base += (long)v.channel * a->HW;
    v.channel = 0;
    if ((uintptr_t)v.base & 15) ok = false;
  };
  for (int k = 0; k < a->K; ++k) use_var(r->q[k]);
  use_var(r->ps);
  return ok ? SDY_OK : SDY_ERR_ARG;
}

}  // namespace

extern "C" size_t sdy_dry_air_workspace_bytes(int B, int T, int HW) {
  if (B < 1 || T < 1 || HW < 1) return 0;
  return (size_t)B * T * n_chunks(HW) * 2 * sizeof(double);
}

extern "C" int sdy_dry_air_series_host(const sdy_dry_air_args* args) {
  sdy_dry_air_args a;
  SDY_TRY(check_args(args, false, &a));
  const int HW = a.HW, K = a.K, chunks = n_chunks(HW), rows = a.B * a.T;
  std::vector<double> partials((size_t)rows * chunks * 2);
  auto get = [&](const sdy_dry_air_var& v, int b, int t, int p) {
    return sdy_corr_denorm(v.base[(long)b * v.stride_b + (long)t * v.stride_t + p], v.mean, v.std);
  };
  for (int row = 0; row < rows; ++row) {
    const int b = row / a.T, t = row - b * a.T;
    for (int chunk = 0; chunk < chunks; ++chunk) {
      // the device's tree: a thread's four columns in order, the butterfly over the 64 lanes of a wave, the waves in order
      double lane[2][kThreads];
      for (int tid = 0; tid < kThreads; ++tid) {
        double acc_w = 0.0, acc_d = 0.0;
        const int p0 = (chunk * kThreads + tid) * kColsPerThread;
        for (int p = p0; p < p0 + kColsPerThread && p < HW; ++p) {
          const float ps = get(a.ps, b, t, p);
          const float twp = sdy_corr_twp(sdy_corr_dp_q(K, a.ak, a.bk, ps, [&](int k) { return get(a.q[k], b, t, p); }));
          dry_air_accumulate(a.area[p], sdy_corr_dry(ps, twp), &acc_w, &acc_d);
        }
        lane[0][tid] = acc_w;
        lane[1][tid] = acc_d;
      }
      for (int j = 0; j < 2; ++j) {
        double total = sdy_wave_sum_host(lane[j]);
        for (int wv = 1; wv < kWaves; ++wv) total += sdy_wave_sum_host(lane[j] + wv * 64);
        partials[((size_t)row * chunks + chunk) * 2 + j] = total;
      }
    }
  }
  for (int row = 0; row < rows; ++row) a.gm[row] = dry_air_row_mean(partials.data(), row, chunks);
  if (a.T < 2) return SDY_OK;
  for (int t = 0; t < a.T - 1; ++t) a.absdiff[t] = dry_air_absdiff(a.gm, a.B, a.T, t);
  const double m = dry_air_mean(a.absdiff, a.T);
  a.mean_absdiff[0] = a.accumulate ? a.mean_absdiff[0] + m : m;
  return SDY_OK;
}

extern "C" int sdy_dry_air_series(const sdy_dry_air_args* args, void* stream) {
  sdy_dry_air_args a;
  SDY_TRY(check_args(args, true, &a));
  return launch_dry_air<SDY_DERIVED_MAX_LEVELS>(a, (hipStream_t)stream);
}

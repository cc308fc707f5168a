// Regional area-weighted metric sums (sdy_region_series, include/sdy_amd.h), gfx950: MeanAggregator's eight sums for every
// region, all variables of one window in one launch.
//   region_series_kernel: one block per (variable, sample, time, chunk of SDY_RS_CHUNK grid points), one quarter of the chunk
//     (256 points) after the other.  Stage: the quarter's M x 256 member values go from the window, read in place (16-byte loads
//     where the window allows them), to LDS -- the pair term of the CRPS reads every member M times, and M planes of a chunk
//     do not fit the 32 KB L1: re-read from global memory they came from L2 and beyond.  Point: one thread per grid point
//     reads its members from LDS (conflict-free: consecutive lanes, consecutive words; nobody keeps a member array) and writes
//     the point's four quantities (em - y, member variance, CRPS, y) to LDS.  Reduce: a wave takes the regions r = wave, wave
//     + 4, ...; for each it reads the region's weights, adds the weighted terms of the 256 points into eight float64 registers
//     (a lane takes points lane, lane + 64, ... in ascending order), adds the lanes by a butterfly and leaves the quarter's
//     sums in LDS.  Last: the quarters are added in order into the chunk's 8 * n_regions partials in ws.
//     The window is read once whatever n_regions; the registers hold one region's eight sums at a time.
//   region_combine_kernel: a plane's chunks in ascending order -> out.
// No atomics; what a block adds, and in which order, depends on its plane and the weights alone.
// The arithmetic of a point is ensemble_point.h and region_series.h, the tree of the sums ordered_sum.h.
#include <vector>

#include "common.h"
#include "ensemble_point.h"
#include "ordered_sum.h"
#include "region_series.h"
#include "window.h"

namespace {

constexpr int kThreads = SDY_RS_QUARTER;     // 256: one thread per grid point of a quarter
constexpr int kWaves = kThreads / 64;
constexpr int kMaxMembers = SDY_REGION_MAX_MEMBERS;
static_assert(kThreads == SDY_RS_QUARTER && kThreads * SDY_RS_QUARTERS == SDY_RS_CHUNK, "one thread per point of a quarter");

// Block blockIdx.x of variable blockIdx.y: chunk = x % chunks of plane x / chunks = sample * T + time.  Every index is bounded
// by the entry point: x < 2^31, a point p < HW before any access (HW % 4 == 0 on the 16-byte path, so 4 points are inside or
// outside together), partial indices < nvars * 2^31 * 128.  Dynamic LDS: M * kThreads floats.
template <int W>
__global__ __launch_bounds__(kThreads) void region_series_kernel(const sdy_region_series_args a, int chunks, double* partials) {
  extern __shared__ float sh_m[];                                        // [M][256]: the members of the quarter's points
  __shared__ double sh_q[4][SDY_RS_QUARTER];                             // em - y | variance | CRPS | y of the quarter's points
  __shared__ double sh_part[SDY_REGION_MAX][SDY_RS_QUARTERS][SDY_RS_SUMS];
  const int v = blockIdx.y, M = a.win.n0, T = a.win.T, R = a.n_regions;
  const long HW = a.HW;
  const int chunk = blockIdx.x % chunks, plane = blockIdx.x / chunks;
  const int s = plane / T, t = plane - s * T;
  const float* gen = a.win.gen[v] + (long)s * a.win.gs1 + (long)t * HW;
  const float* tgt = a.win.target[v] + (long)s * a.win.ts1 + (long)t * HW;
  const long gs0 = a.win.gs0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int quarter = 0; quarter < SDY_RS_QUARTERS; ++quarter) {
    const long q0 = (long)chunk * SDY_RS_CHUNK + (long)quarter * SDY_RS_QUARTER;   // the quarter's first point
    if (q0 >= HW) {                                                      // (the same for the whole block) past the plane: sums 0
      for (int i = tid; i < R * SDY_RS_SUMS; i += kThreads) sh_part[i / SDY_RS_SUMS][quarter][i % SDY_RS_SUMS] = 0.0;
      continue;
    }
    // (the previous quarter's readers of sh_m finished before its last barrier; sh_q is written after the next one)
    if (W == 4) {
      const int at = lane * 4;
      if (q0 + at < HW) {
#pragma unroll 4
        for (int i = wave; i < M; i += kWaves)
          *reinterpret_cast<f32x4*>(sh_m + i * kThreads + at) = ld<4>(gen + (long)i * gs0 + q0 + at);
      }
    } else if (q0 + tid < HW) {
#pragma unroll 4
      for (int i = 0; i < M; ++i) sh_m[i * kThreads + tid] = gen[(long)i * gs0 + q0 + tid];
    }
    __syncthreads();
    {
      const long p = q0 + tid;
      sdy_ens_stats st = {0.0, 0.0, 0.0};                                  // past the plane: every weight reads as 0 below
      double y = 0.0;
      if (p < HW) {
        y = (double)tgt[p];
        st = sdy_ens_point(M, y, [&](int i) { return (double)sh_m[i * kThreads + tid]; }, [](int, double) {});
      }
      sh_q[0][tid] = st.e;
      sh_q[1][tid] = st.var;
      sh_q[2][tid] = st.crps;
      sh_q[3][tid] = y;
    }
    __syncthreads();
    for (int r = wave; r < R; r += kWaves) {
      const float* wr = a.weights + (long)r * HW;
      double acc[SDY_RS_SUMS];
#pragma unroll
      for (int k = 0; k < SDY_RS_SUMS; ++k) acc[k] = 0.0;
#pragma unroll
      for (int j = 0; j < SDY_RS_QUARTER / 64; ++j) {
        const int at = j * 64 + lane;
        const long p = q0 + at;
        const float w = p < HW ? wr[p] : 0.0f;
        if (w != 0.0f) sdy_rs_add((double)w, sh_q[0][at], sh_q[1][at], sh_q[2][at], sh_q[3][at], acc);   // the zero-weight rule
      }
#pragma unroll
      for (int k = 0; k < SDY_RS_SUMS; ++k) {
        sdy_wave_sum(acc[k]);
        if (lane == 0) sh_part[r][quarter][k] = acc[k];
      }
    }
  }
  __syncthreads();

  double* out = partials + ((long)v * gridDim.x + blockIdx.x) * ((long)R * SDY_RS_SUMS);
  for (int i = tid; i < R * SDY_RS_SUMS; i += kThreads) {
    const int r = i / SDY_RS_SUMS, k = i - r * SDY_RS_SUMS;
    out[i] = sdy_fold_rows(sh_part[r], k);
  }
}

// one thread per element of out (nvars, R, n1 * T, 8); partials (nvars, n1 * T, chunks, R, 8): a plane's chunks in chunk order
__global__ __launch_bounds__(kThreads) void region_combine_kernel(const double* partials, int chunks, int R, long planes, long n_out,
                                                                  double* out) {
  const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= n_out) return;
  const int k = (int)(idx % SDY_RS_SUMS);
  long rest = idx / SDY_RS_SUMS;
  const long plane = rest % planes;
  rest /= planes;
  const int r = (int)(rest % R);
  const long v = rest / R;
  const int stride = R * SDY_RS_SUMS;
  out[idx] = sdy_sum_chunks(partials + (v * planes + plane) * chunks * stride, chunks, stride, r * SDY_RS_SUMS + k);
}

int check(const sdy_region_series_args* a, bool need_ws) {
  if (!a) return SDY_ERR_ARG;
  if (a->n_regions < 1 || a->n_regions > SDY_REGION_MAX || a->HW < 1) return SDY_ERR_ARG;
  if (!a->weights || !a->out || ((uintptr_t)a->out & 7)) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, a->HW));
  if (a->win.n0 > kMaxMembers) return SDY_ERR_UNSUPPORTED;
  // 32-bit block numbers within a variable
  if ((long)a->win.n1 * a->win.T * sdy_rs_chunks(a->HW) > 0x7fffffffL) return SDY_ERR_UNSUPPORTED;
  // ... and of the combine launch: 256 elements of out per block (nvars * n_regions * 8 <= 96 * 16 * 8 < 2^14)
  if ((long)a->win.nvars * a->n_regions * SDY_RS_SUMS * ((long)a->win.n1 * a->win.T) >= (1L << 38)) return SDY_ERR_UNSUPPORTED;
  if (need_ws && !sdy_ws_ok(a->ws, a->ws_bytes,
                            sdy_region_series_workspace_bytes(a->win.nvars, a->n_regions, a->win.n1, a->win.T, a->HW)))
    return SDY_ERR_ARG;
  return SDY_OK;
}

}  // namespace

extern "C" size_t sdy_region_series_workspace_bytes(int nvars, int n_regions, int n1, int T, int HW) {
  if (nvars < 1 || nvars > SDY_MAX_VARS || n_regions < 1 || n_regions > SDY_REGION_MAX || n1 < 1 || T < 1 || HW < 1) return 0;
  return (size_t)nvars * (size_t)n1 * (size_t)T * (size_t)sdy_rs_chunks(HW) * n_regions * SDY_RS_SUMS * sizeof(double);
}

// The device's partition: chunks, quarters, then the quarters and the chunks in order; inside a quarter the points are added
// in point order, where the device adds lane-strided partial sums by a butterfly.
extern "C" int sdy_region_series_host(const sdy_region_series_args* a) {
  SDY_TRY(check(a, false));
  const sdy_window& w = a->win;
  const int R = a->n_regions, M = w.n0, chunks = (int)sdy_rs_chunks(a->HW), stride = R * SDY_RS_SUMS;
  const long HW = a->HW;
  std::vector<double> partials((size_t)chunks * stride), q(4 * (size_t)SDY_RS_CHUNK);
  for (int v = 0; v < w.nvars; ++v)
    for (long s = 0; s < w.n1; ++s)
      for (int t = 0; t < w.T; ++t) {
        const float* gen = w.gen[v] + s * w.gs1 + (long)t * HW;
        const float* tgt = w.target[v] + s * w.ts1 + (long)t * HW;
        for (int c = 0; c < chunks; ++c) {
          const long base = (long)c * SDY_RS_CHUNK;
          const int n = (int)(HW - base < SDY_RS_CHUNK ? HW - base : SDY_RS_CHUNK);
          for (int at = 0; at < n; ++at) {
            const long p = base + at;
            const double y = (double)tgt[p];
            const sdy_ens_stats st =
                sdy_ens_point(M, y, [&](int i) { return (double)gen[(long)i * w.gs0 + p]; }, [](int, double) {});
            q[at] = st.e, q[SDY_RS_CHUNK + at] = st.var, q[2 * SDY_RS_CHUNK + at] = st.crps, q[3 * SDY_RS_CHUNK + at] = y;
          }
          for (int r = 0; r < R; ++r) {
            const float* wr = a->weights + (long)r * HW;
            double* part = partials.data() + (size_t)c * stride + (size_t)r * SDY_RS_SUMS;
            for (int k = 0; k < SDY_RS_SUMS; ++k) part[k] = 0.0;
            for (int quarter = 0; quarter < SDY_RS_QUARTERS; ++quarter) {
              double acc[SDY_RS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
              for (int at = quarter * SDY_RS_QUARTER; at < (quarter + 1) * SDY_RS_QUARTER && at < n; ++at) {
                const float wt = wr[base + at];
                if (wt != 0.0f)
                  sdy_rs_add((double)wt, q[at], q[SDY_RS_CHUNK + at], q[2 * SDY_RS_CHUNK + at], q[3 * SDY_RS_CHUNK + at], acc);
              }
              for (int k = 0; k < SDY_RS_SUMS; ++k) part[k] = quarter == 0 ? acc[k] : part[k] + acc[k];
            }
          }
        }
        for (int r = 0; r < R; ++r)
          for (int k = 0; k < SDY_RS_SUMS; ++k)
            a->out[((((long)v * R + r) * w.n1 + s) * w.T + t) * SDY_RS_SUMS + k] =
                sdy_sum_chunks(partials.data(), chunks, stride, r * SDY_RS_SUMS + k);
      }
  return SDY_OK;
}

extern "C" int sdy_region_series(const sdy_region_series_args* a, void* stream) {
  SDY_TRY(check(a, true));
  const int chunks = (int)sdy_rs_chunks(a->HW);
  const long planes = (long)a->win.n1 * a->win.T;
  const dim3 grid((unsigned)(planes * chunks), a->win.nvars);
  double* partials = static_cast<double*>(a->ws);
  // up to 64 members x 256 points x 4 bytes of dynamic LDS on top of the 12 KB of static: more than the 64 KB a kernel gets unasked
  static SdyOncePerDevice once;
  std::atomic<bool>* attr_done = nullptr;
  SDY_TRY(once.slot(&attr_done));
  if (!*attr_done) {
    constexpr int max_smem = kMaxMembers * kThreads * (int)sizeof(float);
    SDY_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&region_series_kernel<4>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, max_smem));
    SDY_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&region_series_kernel<1>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, max_smem));
    *attr_done = true;
  }
  const size_t smem = (size_t)a->win.n0 * kThreads * sizeof(float);
  if (sdy_window_vec4(&a->win, a->HW))
    hipLaunchKernelGGL(region_series_kernel<4>, grid, dim3(kThreads), smem, (hipStream_t)stream, *a, chunks, partials);
  else
    hipLaunchKernelGGL(region_series_kernel<1>, grid, dim3(kThreads), smem, (hipStream_t)stream, *a, chunks, partials);
  SDY_TRY(sdy_launch_status());
  const long n_out = (long)a->win.nvars * a->n_regions * planes * SDY_RS_SUMS;
  hipLaunchKernelGGL(region_combine_kernel, dim3((unsigned)((n_out + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, partials, chunks, a->n_regions, planes, n_out, a->out);
  return sdy_launch_status();
}

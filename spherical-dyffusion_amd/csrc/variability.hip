// Per-trajectory time variance and lag-1 autocorrelation of a rollout at every grid point (no counterpart in the reference),
// gfx950.
//   sdy_time_variability_accumulate: all variables of one window in one launch, read in place through the strided views the
//     window driver hands over.  The state of a trajectory and grid point -- three float64 sums and the fp32 pair (origin, last
//     value) -- stays on the device and carries the run across window boundaries: the lag product of a window's first time
//     takes its predecessor from the state.  HBM-bound streaming: every input element is read once, the state is read and
//     written once, exactly one thread owns a state element: no atomics, no LDS.
//   sdy_time_variability_maps: elementwise, state -> variance and lag-1 autocorrelation.
//   sdy_time_variability_stats: once per get_logs, reduce -> combine.  One thread per (sample, grid point) walks the members;
//     a slot's terms are added over a wave by a butterfly, over the four waves in order, and a second launch adds the blocks'
//     partials in block order (ordered_sum.h).
// The arithmetic of an element and of a grid point is variability.h.
#include <vector>

#include "common.h"
#include "ordered_sum.h"
#include "variability.h"
#include "window.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBlocksPerLaunch = 1024;  // over all variables; a variable with more work strides over its items
constexpr int kMinBlocksPerVar = 32;
constexpr int kTimesInFlight = 6;       // independent time loads a thread issues before it consumes the first

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// the state of a work item's W points as one value: 32-byte accesses (two 16-byte instructions) when W == 4
template <int W>
using Sums = std::conditional_t<W == 4, f64x4, double>;
template <int W>
using Pairs = std::conditional_t<W == 4, f32x8, f32x2>;
__device__ __forceinline__ double sum_of(double v, int) { return v; }
__device__ __forceinline__ double sum_of(f64x4 v, int k) { return v[k]; }
__device__ __forceinline__ void set_sum(double& v, int, double x) { v = x; }
__device__ __forceinline__ void set_sum(f64x4& v, int k, double x) { v[k] = x; }

// Work item idx of variable blockIdx.y: W grid points (4 or 1) at point W * q of state row r, idx = r * (HW / W) + q; rows
// 0 .. n0*n1 - 1 are the generated rows (member i0 = r / n1, sample i1 = r % n1), rows n0*n1 .. n0*n1 + n1 - 1 the target's.
// Consecutive lanes touch consecutive addresses of every time and of the state.  Every index is bounded by the entry point:
// r < n0*n1 + n1 < 2^32, q * W < HW, t < T with T * HW <= 2^30, state indices < 2^50.
template <int W>
__global__ __launch_bounds__(kThreads) void variability_kernel(const sdy_variability_args a, unsigned long n_items) {
  const int v = blockIdx.y;
  const unsigned long per_row = (unsigned long)(a.HW / W);
  const unsigned long gen_rows = (unsigned long)a.win.n0 * (unsigned long)a.win.n1;
  const unsigned long rows = gen_rows + (unsigned long)a.win.n1;
  const long HW = a.HW;
  const int T = a.win.T;
  const bool first = a.first != 0;
  for (unsigned long idx = (unsigned long)blockIdx.x * kThreads + threadIdx.x; idx < n_items;
       idx += (unsigned long)gridDim.x * kThreads) {
    const unsigned long r = idx / per_row, q = idx - r * per_row;
    const float* src;
    if (r < gen_rows) {
      const unsigned long i0 = r / (unsigned)a.win.n1, i1 = r - i0 * (unsigned)a.win.n1;
      src = a.win.gen[v] + (long)i0 * a.win.gs0 + (long)i1 * a.win.gs1;
    } else {
      src = a.win.target[v] + (long)(r - gen_rows) * a.win.ts1;
    }
    src += (long)q * W;
    const long at = ((long)v * (long)rows + (long)r) * HW + (long)q * W;
    Sums<W>* const ps1 = reinterpret_cast<Sums<W>*>(a.s1 + at);
    Sums<W>* const ps2 = reinterpret_cast<Sums<W>*>(a.s2 + at);
    Sums<W>* const pp = reinterpret_cast<Sums<W>*>(a.p + at);
    Pairs<W>* const pol = reinterpret_cast<Pairs<W>*>(a.origin_last + 2 * at);
    // the state and the first kTimesInFlight times are requested together; a batch past the end of the window re-reads the last
    // time (from cache) and adds nothing
    double s1[W], s2[W], p[W], d_prev[W];
    float c[W], last[W];
    bool has_prev = !first;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      s1[k] = s2[k] = p[k] = d_prev[k] = 0.0;
      c[k] = last[k] = 0.0f;
    }
    if (!first) {
      const Sums<W> v1 = *ps1, v2 = *ps2, vp = *pp;
      const Pairs<W> ol = *pol;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        s1[k] = sum_of(v1, k);
        s2[k] = sum_of(v2, k);
        p[k] = sum_of(vp, k);
        c[k] = ol[2 * k];
        d_prev[k] = sdy_tv_dev(ol[2 * k + 1], ol[2 * k]);
      }
    }
    for (int t = a.t0; t < T; t += kTimesInFlight) {
      Vec<W> x[kTimesInFlight];
#pragma unroll
      for (int k = 0; k < kTimesInFlight; ++k) x[k] = ld<W>(src + (long)(t + k < T ? t + k : T - 1) * HW);
      if (first && t == a.t0) {
#pragma unroll
        for (int k = 0; k < W; ++k) c[k] = comp(x[0], k);       // the origin: the trajectory's first counted value
      }
#pragma unroll
      for (int k = 0; k < kTimesInFlight; ++k)
        if (t + k < T) {
#pragma unroll
          for (int e = 0; e < W; ++e) {
            const float xe = comp(x[k], e);
            const double d = sdy_tv_dev(xe, c[e]);
            sdy_tv_step(s1[e], s2[e], p[e], d, d_prev[e], has_prev);
            d_prev[e] = d;
            last[e] = xe;
          }
          has_prev = true;
        }
    }
    Sums<W> v1, v2, vp;
    Pairs<W> ol;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      set_sum(v1, k, s1[k]);
      set_sum(v2, k, s2[k]);
      set_sum(vp, k, p[k]);
      ol[2 * k] = c[k];
      ol[2 * k + 1] = last[k];
    }
    *ps1 = v1;
    *ps2 = v2;
    *pp = vp;
    *pol = ol;
  }
}

// one thread per state element
__global__ __launch_bounds__(kThreads) void variability_maps_kernel(const sdy_variability_maps_args a) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n_elems) return;
  const f32x2 ol = reinterpret_cast<const f32x2*>(a.origin_last)[i];
  const sdy_tv_moments r = sdy_tv_finish(a.s1[i], a.s2[i], a.p[i], ol[0], ol[1], a.n_times);
  a.variance[i] = r.variance;
  a.lag1[i] = r.lag1;
}

// grid (chunks of kThreads points of the n1 * HW of a variable, nvars).  partials: (nvars, chunks, SDY_TV_SLOTS).
__global__ __launch_bounds__(kThreads) void variability_stats_kernel(const sdy_variability_stats_args a, double* partials) {
  __shared__ double sh[kWaves][SDY_TV_SLOTS];
  const int v = blockIdx.y, M = a.M;
  const long n = (long)a.n1 * a.HW;                          // <= 2^30
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;  // sample * HW + grid point
  const bool active = p < n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double n_times = a.n_times;
  const long base = (long)v * (M + 1) * n + p;               // member i at base + i * n, the target at base + M * n
  const f32x2* const ol = reinterpret_cast<const f32x2*>(a.origin_last);
  // an idle lane reads nothing and contributes 0 to every slot
  auto moments = [&](int i) {
    const long at = base + (long)i * n;
    return sdy_tv_finish(a.s1[at], a.s2[at], a.p[at], ol[at][0], ol[at][1], n_times);
  };
  auto emit = [&](int slot, double x) {
    if (!active) x = 0.0;
    sdy_wave_sum(x);
    if (lane == 0) sh[wave][slot] = x;
  };
  const sdy_tv_moments zero = {0.0, 0.0, 0.0};
  const sdy_tv_moments t = active ? moments(M) : zero;
  const double w = active ? (double)a.weights[p % a.HW] : 0.0;
  sdy_tv_point(M, n_times, w, t, [&](int i) { return active ? moments(i) : zero; }, emit);
  __syncthreads();
  double* out = partials + ((long)v * gridDim.x + blockIdx.x) * SDY_TV_SLOTS;
  if (threadIdx.x < SDY_TV_SLOTS) out[threadIdx.x] = sdy_fold_rows(sh, threadIdx.x);
}

long n_chunks(long n) { return (n + kThreads - 1) / kThreads; }

// the window's own checks are sdy_window_check's; here the time offset and what bounds a state address
int check_accumulate(const sdy_variability_args* a) {
  if (!a) return SDY_ERR_ARG;
  if (a->t0 < 0 || a->t0 >= a->win.T) return SDY_ERR_ARG;
  if (!a->s1 || !a->s2 || !a->p || !a->origin_last) return SDY_ERR_ARG;
  if (((uintptr_t)a->s1 | (uintptr_t)a->s2 | (uintptr_t)a->p | (uintptr_t)a->origin_last) & 7) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, a->HW));
  // 64-bit flat state indices: nvars <= 96 < 2^7, (n0 + 1) * n1 < 2^32, HW <= 2^30 -- the product can leave 2^50
  const long per_var = ((long)a->win.n0 + 1) * a->win.n1 * a->HW;      // < 2^62
  if (per_var >= (1L << 50) || (long)a->win.nvars * per_var >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

int check_maps(const sdy_variability_maps_args* a) {
  if (!a) return SDY_ERR_ARG;
  if (a->n_elems < 1) return SDY_ERR_ARG;
  if (!a->s1 || !a->s2 || !a->p || !a->origin_last || !a->variance || !a->lag1) return SDY_ERR_ARG;
  if (((uintptr_t)a->s1 | (uintptr_t)a->s2 | (uintptr_t)a->p | (uintptr_t)a->origin_last | (uintptr_t)a->variance |
       (uintptr_t)a->lag1) & 7)
    return SDY_ERR_ARG;
  if (!(a->n_times >= 1.0) || !std::isfinite(a->n_times)) return SDY_ERR_ARG;
  if (a->n_elems > (long)kThreads * 0x7fffffffL) return SDY_ERR_UNSUPPORTED;     // blocks of one launch
  return SDY_OK;
}

int check_stats(const sdy_variability_stats_args* a, bool need_ws) {
  if (!a) return SDY_ERR_ARG;
  if (a->nvars < 1 || a->M < 1 || a->n1 < 1 || a->HW < 1) return SDY_ERR_ARG;
  if (!a->s1 || !a->s2 || !a->p || !a->origin_last || !a->weights || !a->out) return SDY_ERR_ARG;
  if (((uintptr_t)a->s1 | (uintptr_t)a->s2 | (uintptr_t)a->p | (uintptr_t)a->origin_last | (uintptr_t)a->out) & 7)
    return SDY_ERR_ARG;
  if (!(a->n_times >= 1.0) || !std::isfinite(a->n_times)) return SDY_ERR_ARG;
  if (a->nvars > 65535 || (long)a->n1 * a->HW > (1L << 30)) return SDY_ERR_UNSUPPORTED;
  if ((long)a->nvars * ((long)a->M + 1) * ((long)a->n1 * a->HW) >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  if (need_ws && !sdy_ws_ok(a->ws, a->ws_bytes, sdy_time_variability_workspace_bytes(a->nvars, a->n1, a->HW)))
    return SDY_ERR_ARG;
  return SDY_OK;
}

}  // namespace

extern "C" size_t sdy_time_variability_workspace_bytes(int nvars, int n1, int HW) {
  if (nvars < 1 || n1 < 1 || HW < 1) return 0;
  return (size_t)nvars * (size_t)n_chunks((long)n1 * HW) * SDY_TV_SLOTS * sizeof(double);
}

extern "C" int sdy_time_variability_accumulate_host(const sdy_variability_args* a) {
  SDY_TRY(check_accumulate(a));
  const sdy_window& w = a->win;
  const long HW = a->HW, rows = ((long)w.n0 + 1) * w.n1;
  const bool first = a->first != 0;
  auto add_row = [&](const float* src, long at) {
    for (long e = 0; e < HW; ++e) {
      double s1 = 0.0, s2 = 0.0, p = 0.0, d_prev = 0.0;
      float c = src[(long)a->t0 * HW + e], last = c;
      bool has_prev = !first;
      if (!first) {
        s1 = a->s1[at + e];
        s2 = a->s2[at + e];
        p = a->p[at + e];
        c = a->origin_last[2 * (at + e)];
        d_prev = sdy_tv_dev(a->origin_last[2 * (at + e) + 1], c);
      }
      for (int t = a->t0; t < w.T; ++t) {
        last = src[(long)t * HW + e];
        const double d = sdy_tv_dev(last, c);
        sdy_tv_step(s1, s2, p, d, d_prev, has_prev);
        d_prev = d;
        has_prev = true;
      }
      a->s1[at + e] = s1;
      a->s2[at + e] = s2;
      a->p[at + e] = p;
      a->origin_last[2 * (at + e)] = c;
      a->origin_last[2 * (at + e) + 1] = last;
    }
  };
  for (int v = 0; v < w.nvars; ++v) {
    for (long i0 = 0; i0 < w.n0; ++i0)
      for (long i1 = 0; i1 < w.n1; ++i1) add_row(w.gen[v] + i0 * w.gs0 + i1 * w.gs1, ((long)v * rows + i0 * w.n1 + i1) * HW);
    for (long i1 = 0; i1 < w.n1; ++i1) add_row(w.target[v] + i1 * w.ts1, ((long)v * rows + (long)w.n0 * w.n1 + i1) * HW);
  }
  return SDY_OK;
}

extern "C" int sdy_time_variability_accumulate(const sdy_variability_args* a, void* stream) {
  SDY_TRY(check_accumulate(a));
  // four points per work item: 16-byte loads of the window and 32-byte accesses of the state
  const bool vec = sdy_window_vec4(&a->win, a->HW) &&
                   (((uintptr_t)a->s1 | (uintptr_t)a->s2 | (uintptr_t)a->p | (uintptr_t)a->origin_last) & 31) == 0;
  const unsigned long rows = (unsigned long)a->win.n0 * a->win.n1 + a->win.n1;
  const unsigned long n_items = rows * (unsigned long)(vec ? a->HW / 4 : a->HW);
  const dim3 grid(sdy_grid_cap((n_items + kThreads - 1) / kThreads, a->win.nvars, kBlocksPerLaunch, kMinBlocksPerVar),
                  a->win.nvars);
  if (vec)
    hipLaunchKernelGGL(variability_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, *a, n_items);
  else
    hipLaunchKernelGGL(variability_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, *a, n_items);
  return sdy_launch_status();
}

extern "C" int sdy_time_variability_maps_host(const sdy_variability_maps_args* a) {
  SDY_TRY(check_maps(a));
  for (long i = 0; i < a->n_elems; ++i) {
    const sdy_tv_moments r =
        sdy_tv_finish(a->s1[i], a->s2[i], a->p[i], a->origin_last[2 * i], a->origin_last[2 * i + 1], a->n_times);
    a->variance[i] = r.variance;
    a->lag1[i] = r.lag1;
  }
  return SDY_OK;
}

extern "C" int sdy_time_variability_maps(const sdy_variability_maps_args* a, void* stream) {
  SDY_TRY(check_maps(a));
  hipLaunchKernelGGL(variability_maps_kernel, dim3((unsigned)n_chunks(a->n_elems)), dim3(kThreads), 0, (hipStream_t)stream, *a);
  return sdy_launch_status();
}

// The device's partition (chunks of kThreads points, then the chunks in order); inside a chunk the points are added in
// order, where the device adds them in a butterfly: the two agree to the rounding of a 256-term float64 sum.
extern "C" int sdy_time_variability_stats_host(const sdy_variability_stats_args* a) {
  SDY_TRY(check_stats(a, false));
  const int M = a->M;
  const long n = (long)a->n1 * a->HW, chunks = n_chunks(n);
  std::vector<double> partials((size_t)chunks * SDY_TV_SLOTS);
  for (int v = 0; v < a->nvars; ++v) {
    for (long c = 0; c < chunks; ++c) {
      double* part = partials.data() + c * SDY_TV_SLOTS;
      for (int k = 0; k < SDY_TV_SLOTS; ++k) part[k] = 0.0;
      for (long p = c * kThreads; p < (c + 1) * kThreads && p < n; ++p) {
        const long base = (long)v * (M + 1) * n + p;
        auto moments = [&](int i) {
          const long at = base + (long)i * n;
          return sdy_tv_finish(a->s1[at], a->s2[at], a->p[at], a->origin_last[2 * at], a->origin_last[2 * at + 1], a->n_times);
        };
        sdy_tv_point(M, a->n_times, (double)a->weights[p % a->HW], moments(M), moments,
                     [&](int slot, double x) { part[slot] += x; });
      }
    }
    for (int k = 0; k < SDY_TV_SLOTS; ++k) a->out[(long)v * SDY_TV_SLOTS + k] = sdy_sum_chunks(partials.data(), (int)chunks, SDY_TV_SLOTS, k);
  }
  return SDY_OK;
}

extern "C" int sdy_time_variability_stats(const sdy_variability_stats_args* a, void* stream) {
  SDY_TRY(check_stats(a, true));
  const int chunks = (int)n_chunks((long)a->n1 * a->HW);
  double* partials = static_cast<double*>(a->ws);
  hipLaunchKernelGGL(variability_stats_kernel, dim3(chunks, a->nvars), dim3(kThreads), 0, (hipStream_t)stream, *a, partials);
  SDY_TRY(sdy_launch_status());
  return sdy_combine_chunks_launch(partials, a->nvars, chunks, SDY_TV_SLOTS, a->out, (hipStream_t)stream);
}

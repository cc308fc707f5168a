// Per-member time means of an ensemble rollout and their statistics (the reference's ensemble TimeMeanAggregator,
// src/evaluation/aggregators/time_mean.py with is_ensemble=True), gfx950.
//   sdy_member_time_sum: all variables of one window in one launch, read in place through the strided views the window driver
//     hands over, added to float64 accumulators per (variable, member, sample, grid point) that stay on the device.  HBM-bound
//     streaming: every input element is read once, exactly one thread owns an accumulator element: no atomics, no LDS.
//   sdy_member_map_stats: once per get_logs, reduce -> combine.  One thread per (sample, grid point); the members of a point
//     are read from the accumulators twice (the pair term of the CRPS re-reads them from cache: M (M - 1) / 2 loads of lines
//     that the first pass brought in), so no thread keeps a member array.  A slot's terms are added over a wave by a butterfly,
//     over the four waves in order, and a second launch adds the blocks' partials in block order (ordered_sum.h).
// The arithmetic of an element and of a grid point is member_mean.h.
#include <vector>

#include "common.h"
#include "member_mean.h"
#include "ordered_sum.h"
#include "window.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBlocksPerLaunch = 1024;  // over all variables; a variable with more work strides over its items
constexpr int kMinBlocksPerVar = 32;
constexpr int kTimesInFlight = 8;       // independent time loads a thread issues before it consumes the first
constexpr int kMaxMembers = SDY_MEMBER_STATS_MAX_MEMBERS;

// Work item idx of variable blockIdx.y: W grid points (4 or 1) at point W * q of row r, idx = r * (HW / W) + q; rows
// 0 .. n0*n1 - 1 are the generated rows (member i0 = r / n1, sample i1 = r % n1), rows n0*n1 .. n0*n1 + n1 - 1 the target's.
// Consecutive lanes touch consecutive addresses of every time and of the accumulators.  Every index is bounded by the entry
// point: r < n0*n1 + n1 < 2^32, q * W < HW, t < T with T * HW <= 2^30, accumulator indices < 2^50.
template <int W>
__global__ __launch_bounds__(kThreads) void member_sum_kernel(const sdy_member_sum_args a, unsigned long n_items) {
  const int v = blockIdx.y;
  const unsigned long per_row = (unsigned long)(a.HW / W);
  const unsigned long gen_rows = (unsigned long)a.win.n0 * (unsigned long)a.win.n1;
  const long HW = a.HW;
  const int T = a.win.T;
  for (unsigned long idx = (unsigned long)blockIdx.x * kThreads + threadIdx.x; idx < n_items;
       idx += (unsigned long)gridDim.x * kThreads) {
    const unsigned long r = idx / per_row, q = idx - r * per_row;
    const float* src;
    double* acc;
    if (r < gen_rows) {
      const unsigned long i0 = r / (unsigned)a.win.n1, i1 = r - i0 * (unsigned)a.win.n1;
      src = a.win.gen[v] + (long)i0 * a.win.gs0 + (long)i1 * a.win.gs1;
      acc = a.gen_sum + ((long)v * (long)gen_rows + (long)r) * HW;
    } else {
      const unsigned long i1 = r - gen_rows;
      src = a.win.target[v] + (long)i1 * a.win.ts1;
      acc = a.target_sum + ((long)v * a.win.n1 + (long)i1) * HW;
    }
    src += (long)q * W;
    acc += (long)q * W;
    // the accumulator elements and the first kTimesInFlight times are requested together; a batch past the end of the window
    // re-reads the last time (from cache) and adds nothing
    double before[W], s[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
      before[c] = acc[c];
      s[c] = 0.0;
    }
    for (int t = a.t0; t < T; t += kTimesInFlight) {
      Vec<W> x[kTimesInFlight];
#pragma unroll
      for (int k = 0; k < kTimesInFlight; ++k) x[k] = ld<W>(src + (long)(t + k < T ? t + k : T - 1) * HW);
#pragma unroll
      for (int k = 0; k < kTimesInFlight; ++k)
        if (t + k < T) {
#pragma unroll
          for (int c = 0; c < W; ++c) s[c] = sdy_mm_add(s[c], comp(x[k], c));
        }
    }
#pragma unroll
    for (int c = 0; c < W; ++c) acc[c] = sdy_mm_fold(before[c], s[c]);
  }
}

// grid (chunks of kThreads points of the n1 * HW of a variable, nvars).  partials: (nvars, chunks, 2 M + 4).
__global__ __launch_bounds__(kThreads) void member_stats_kernel(const sdy_member_stats_args a, double* partials) {
  __shared__ double sh[kWaves][2 * kMaxMembers + 4];
  const int v = blockIdx.y, M = a.M, slots = sdy_mm_slots(M);
  const long n = (long)a.n1 * a.HW;                          // <= 2^30
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;  // sample * HW + grid point
  const bool active = p < n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double n_times = a.n_times;
  const double* g = a.gen_sum + (long)v * M * n + p;         // member i at g[i * n], read only where active
  double t = 0.0, w = 0.0;
  if (active) {
    t = a.target_sum[(long)v * n + p] / n_times;
    w = (double)a.weights[p % a.HW];
  }
  // an idle lane contributes 0 to every slot: w = 0 and every member 0
  auto member = [&](int i) { return active ? g[(long)i * n] / n_times : 0.0; };
  auto emit = [&](int slot, double x) {
    sdy_wave_sum(x);
    if (lane == 0) sh[wave][slot] = x;
  };
  sdy_mm_point(M, t, w, member, emit);
  __syncthreads();
  double* out = partials + ((long)v * gridDim.x + blockIdx.x) * slots;
  for (int k = threadIdx.x; k < slots; k += kThreads) out[k] = sdy_fold_rows(sh, k);
}

long n_chunks(long n) { return (n + kThreads - 1) / kThreads; }

// the window's own checks are sdy_window_check's; here the time offset and what bounds an accumulator address
int check_sum(const sdy_member_sum_args* a) {
  if (!a) return SDY_ERR_ARG;
  if (a->t0 < 0 || a->t0 >= a->win.T) return SDY_ERR_ARG;
  if (!a->gen_sum || !a->target_sum || (((uintptr_t)a->gen_sum | (uintptr_t)a->target_sum) & 7)) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, a->HW));
  // 64-bit flat accumulator indices: nvars <= 96 < 2^7, n0 * n1 < 2^31, HW <= 2^30 -- the product can leave 2^50
  const long per_var = (long)a->win.n0 * a->win.n1 * a->HW;      // < 2^61
  if (per_var >= (1L << 50) || (long)a->win.nvars * per_var >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

int check_stats(const sdy_member_stats_args* a, bool need_ws) {
  if (!a) return SDY_ERR_ARG;
  if (a->nvars < 1 || a->M < 1 || a->n1 < 1 || a->HW < 1) return SDY_ERR_ARG;
  if (!a->gen_sum || !a->target_sum || !a->weights || !a->out) return SDY_ERR_ARG;
  if (((uintptr_t)a->gen_sum | (uintptr_t)a->target_sum | (uintptr_t)a->out) & 7) return SDY_ERR_ARG;
  if (!(a->n_times > 0.0) || !std::isfinite(a->n_times)) return SDY_ERR_ARG;
  if (a->M > kMaxMembers) return SDY_ERR_UNSUPPORTED;
  if (a->nvars > 65535 || (long)a->n1 * a->HW > (1L << 30)) return SDY_ERR_UNSUPPORTED;
  if ((long)a->nvars * a->M * ((long)a->n1 * a->HW) >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  if (need_ws && !sdy_ws_ok(a->ws, a->ws_bytes, sdy_member_stats_workspace_bytes(a->nvars, a->M, a->n1, a->HW)))
    return SDY_ERR_ARG;
  return SDY_OK;
}

}  // namespace

extern "C" size_t sdy_member_stats_workspace_bytes(int nvars, int M, int n1, int HW) {
  if (nvars < 1 || M < 1 || M > kMaxMembers || n1 < 1 || HW < 1) return 0;
  return (size_t)nvars * (size_t)n_chunks((long)n1 * HW) * sdy_mm_slots(M) * sizeof(double);
}

extern "C" int sdy_member_time_sum_host(const sdy_member_sum_args* a) {
  SDY_TRY(check_sum(a));
  const sdy_window& w = a->win;
  const long HW = a->HW, rows = (long)w.n0 * w.n1;
  auto add_row = [&](const float* src, double* acc) {
    for (long p = 0; p < HW; ++p) {
      double s = 0.0;
      for (int t = a->t0; t < w.T; ++t) s = sdy_mm_add(s, src[(long)t * HW + p]);
      acc[p] = sdy_mm_fold(acc[p], s);
    }
  };
  for (int v = 0; v < w.nvars; ++v) {
    for (long i0 = 0; i0 < w.n0; ++i0)
      for (long i1 = 0; i1 < w.n1; ++i1)
        add_row(w.gen[v] + i0 * w.gs0 + i1 * w.gs1, a->gen_sum + ((long)v * rows + i0 * w.n1 + i1) * HW);
    for (long i1 = 0; i1 < w.n1; ++i1) add_row(w.target[v] + i1 * w.ts1, a->target_sum + ((long)v * w.n1 + i1) * HW);
  }
  return SDY_OK;
}

extern "C" int sdy_member_time_sum(const sdy_member_sum_args* a, void* stream) {
  SDY_TRY(check_sum(a));
  const bool vec = sdy_window_vec4(&a->win, a->HW);
  const unsigned long rows = (unsigned long)a->win.n0 * a->win.n1 + a->win.n1;
  const unsigned long n_items = rows * (unsigned long)(vec ? a->HW / 4 : a->HW);
  const dim3 grid(sdy_grid_cap((n_items + kThreads - 1) / kThreads, a->win.nvars, kBlocksPerLaunch, kMinBlocksPerVar),
                  a->win.nvars);
  if (vec)
    hipLaunchKernelGGL(member_sum_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, *a, n_items);
  else
    hipLaunchKernelGGL(member_sum_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, *a, n_items);
  return sdy_launch_status();
}

// The device's partition (chunks of kThreads points, then the chunks in order); inside a chunk the points are added in
// order, where the device adds them in a butterfly: the two agree to the rounding of a 256-term float64 sum.
extern "C" int sdy_member_map_stats_host(const sdy_member_stats_args* a) {
  SDY_TRY(check_stats(a, false));
  const int M = a->M, slots = sdy_mm_slots(M);
  const long n = (long)a->n1 * a->HW, chunks = n_chunks(n);
  std::vector<double> partials((size_t)chunks * slots);
  for (int v = 0; v < a->nvars; ++v) {
    for (long c = 0; c < chunks; ++c) {
      double* part = partials.data() + c * slots;
      for (int k = 0; k < slots; ++k) part[k] = 0.0;
      for (long p = c * kThreads; p < (c + 1) * kThreads && p < n; ++p) {
        const double* g = a->gen_sum + (long)v * M * n + p;
        const double t = a->target_sum[(long)v * n + p] / a->n_times;
        const double w = (double)a->weights[p % a->HW];
        sdy_mm_point(M, t, w, [&](int i) { return g[(long)i * n] / a->n_times; }, [&](int slot, double x) { part[slot] += x; });
      }
    }
    for (int k = 0; k < slots; ++k) a->out[(long)v * slots + k] = sdy_sum_chunks(partials.data(), (int)chunks, slots, k);
  }
  return SDY_OK;
}

extern "C" int sdy_member_map_stats(const sdy_member_stats_args* a, void* stream) {
  SDY_TRY(check_stats(a, true));
  const int slots = sdy_mm_slots(a->M);
  const int chunks = (int)n_chunks((long)a->n1 * a->HW);
  double* partials = static_cast<double*>(a->ws);
  hipLaunchKernelGGL(member_stats_kernel, dim3(chunks, a->nvars), dim3(kThreads), 0, (hipStream_t)stream, *a, partials);
  SDY_TRY(sdy_launch_status());
  return sdy_combine_chunks_launch(partials, a->nvars, chunks, slots, a->out, (hipStream_t)stream);
}

// Time sums and extremes per time bin (no counterpart in the reference), gfx950.
//   sdy_binned_time_accumulate: a run of same-shaped variables of one window in one launch, read in place through the strided
//     views the window driver hands over.  The host has grouped the window's counted times by bin and passes the groups by value
//     (sdy_binned_sum_args: 64 times per call, 16-bit entries; the structure stays inside the 4 KB of kernel arguments).  A work
//     item owns W grid points of one trajectory row of one variable; per group it loads the bin's accumulator elements once,
//     adds the group's times to them one by one with kInFlight independent loads in flight, and stores them once.  HBM-bound
//     streaming: every input value is read once, exactly one thread owns an accumulator element: no atomics, no LDS.  The
//     chain of an element is sequential in the accumulator itself, so its bits do not depend on the cut into windows.
//     W, the pooling of members and the extremes are template arguments: every per-thread array is indexed at compile time
//     and stays in registers.
// The arithmetic of an element is time_bins.h.
#include "common.h"
#include "time_bins.h"
#include "window.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBlocksPerLaunch = 1024;  // over all variables; a variable with more work strides over its items
constexpr int kMinBlocksPerVar = 32;
constexpr int kInFlight = 8;            // independent loads a thread issues before it consumes the first

typedef double f64x4 __attribute__((ext_vector_type(4)));

// the accumulator elements of a work item's W points as one value: 32-byte accesses (two 16-byte instructions) when W == 4
template <int W>
using Sums = std::conditional_t<W == 4, f64x4, double>;
__device__ __forceinline__ double sum_of(double v, int) { return v; }
__device__ __forceinline__ double sum_of(f64x4 v, int k) { return v[k]; }
__device__ __forceinline__ void set_sum(double& v, int, double x) { v = x; }
__device__ __forceinline__ void set_sum(f64x4& v, int k, double x) { v[k] = x; }
__device__ __forceinline__ void set_comp(float& v, int, float x) { v = x; }
__device__ __forceinline__ void set_comp(f32x4& v, int k, float x) { v[k] = x; }

// the accumulator rows of the generated data of one variable of one bin: members x samples, pooled: samples
inline __host__ __device__ long gen_acc_rows(const sdy_binned_sum_args& a) {
  return a.pool_members ? (long)a.win.n1 : (long)a.win.n0 * a.win.n1;
}

// Work item idx of variable blockIdx.y: W grid points (4 or 1) at point W * q of accumulator row r, idx = r * (HW / W) + q;
// rows 0 .. gen_rows - 1 are the generated rows (member i0 = r / n1, sample i1 = r % n1; POOL: sample r, all its members),
// rows gen_rows .. gen_rows + n1 - 1 the target's.  Consecutive lanes touch consecutive addresses of every time and of the
// accumulators.  Every index is bounded by the entry point: r < n0*n1 + n1 < 2^32, q * W < HW, times[i] < T with T * HW <=
// 2^30, group_bin[g] < n_bins, accumulator indices < 2^50.
template <int W, bool POOL, bool EXT>
__global__ __launch_bounds__(kThreads) void binned_sum_kernel(const sdy_binned_sum_args a, unsigned long n_items) {
  const int v = blockIdx.y;
  const unsigned long per_row = (unsigned long)(a.HW / W);
  const unsigned n1 = (unsigned)a.win.n1;
  const unsigned long gen_rows = POOL ? (unsigned long)n1 : (unsigned long)a.win.n0 * n1;
  const long HW = a.HW;
  for (unsigned long idx = (unsigned long)blockIdx.x * kThreads + threadIdx.x; idx < n_items;
       idx += (unsigned long)gridDim.x * kThreads) {
    const unsigned long r = idx / per_row, q = idx - r * per_row;
    const bool is_gen = r < gen_rows;
    const float* src;
    long at, bin_stride;       // the element of bin 0 and the elements between two bins, in a sum or an extreme alike
    int inner = 1;             // POOL: the members a generated row adds inside each time
    if (is_gen) {
      if (POOL) {
        src = a.win.gen[v] + (long)r * a.win.gs1;
        inner = a.win.n0;
      } else {
        const unsigned long i0 = r / n1, i1 = r - i0 * n1;
        src = a.win.gen[v] + (long)i0 * a.win.gs0 + (long)i1 * a.win.gs1;
      }
      at = ((long)v * (long)gen_rows + (long)r) * HW;
      bin_stride = (long)a.bin_vars * (long)gen_rows * HW;
    } else {
      const unsigned long i1 = r - gen_rows;
      src = a.win.target[v] + (long)i1 * a.win.ts1;
      at = ((long)v * n1 + (long)i1) * HW;
      bin_stride = (long)a.bin_vars * n1 * HW;
    }
    src += (long)q * W;
    at += (long)q * W;
    double* const sums = is_gen ? a.gen_sum : a.target_sum;
    float* const maxs = is_gen ? a.gen_max : a.target_max;
    float* const mins = is_gen ? a.gen_min : a.target_min;
    for (int g = 0; g < a.n_groups; ++g) {
      const int begin = sdy_tb_group_begin(a, g), end = a.group_end[g];
      const long e = at + (long)a.group_bin[g] * bin_stride;
      // the accumulator elements and the group's first kInFlight values are requested together
      Sums<W>* const ps = reinterpret_cast<Sums<W>*>(sums + e);
      const Sums<W> vs = *ps;
      Vec<W> vmax = {}, vmin = {};
      if (EXT) {
        vmax = *reinterpret_cast<const Vec<W>*>(maxs + e);
        vmin = *reinterpret_cast<const Vec<W>*>(mins + e);
      }
      double s[W];
      float hi[W], lo[W];
#pragma unroll
      for (int c = 0; c < W; ++c) {
        s[c] = sum_of(vs, c);
        hi[c] = EXT ? comp(vmax, c) : 0.0f;
        lo[c] = EXT ? comp(vmin, c) : 0.0f;
      }
      auto take = [&](const Vec<W>& x) {
#pragma unroll
        for (int c = 0; c < W; ++c) {
          s[c] = sdy_tb_add(s[c], comp(x, c));
          if (EXT) {
            hi[c] = sdy_tb_max(hi[c], comp(x, c));
            lo[c] = sdy_tb_min(lo[c], comp(x, c));
          }
        }
      };
      if (!POOL) {
        // a batch past the end of the group re-reads its last time (from cache) and adds nothing
        for (int t = begin; t < end; t += kInFlight) {
          Vec<W> x[kInFlight];
#pragma unroll
          for (int k = 0; k < kInFlight; ++k) x[k] = ld<W>(src + (long)a.times[t + k < end ? t + k : end - 1] * HW);
#pragma unroll
          for (int k = 0; k < kInFlight; ++k)
            if (t + k < end) take(x[k]);
        }
      } else {
        // time by time, a time's members in member order, kInFlight of them in flight
        for (int t = begin; t < end; ++t) {
          const float* const at_t = src + (long)a.times[t] * HW;
          for (int m = 0; m < inner; m += kInFlight) {
            Vec<W> x[kInFlight];
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) x[k] = ld<W>(at_t + (long)(m + k < inner ? m + k : inner - 1) * a.win.gs0);
#pragma unroll
            for (int k = 0; k < kInFlight; ++k)
              if (m + k < inner) take(x[k]);
          }
        }
      }
      Sums<W> out;
#pragma unroll
      for (int c = 0; c < W; ++c) set_sum(out, c, s[c]);
      *ps = out;
      if (EXT) {
#pragma unroll
        for (int c = 0; c < W; ++c) {
          set_comp(vmax, c, hi[c]);
          set_comp(vmin, c, lo[c]);
        }
        *reinterpret_cast<Vec<W>*>(maxs + e) = vmax;
        *reinterpret_cast<Vec<W>*>(mins + e) = vmin;
      }
    }
  }
}

bool has_extremes(const sdy_binned_sum_args* a) { return a->gen_max != nullptr; }

// the window's own checks are sdy_window_check's; here the groups and what bounds an accumulator address
int check_args(const sdy_binned_sum_args* a) {
  if (!a || a->struct_size != sizeof(sdy_binned_sum_args)) return SDY_ERR_ARG;
  if (a->n_bins < 1 || a->n_groups < 0 || a->n_groups > SDY_BIN_MAX_TIMES) return SDY_ERR_ARG;
  if (!a->gen_sum || !a->target_sum || (((uintptr_t)a->gen_sum | (uintptr_t)a->target_sum) & 7)) return SDY_ERR_ARG;
  const int n_ext = (a->gen_max != nullptr) + (a->gen_min != nullptr) + (a->target_max != nullptr) + (a->target_min != nullptr);
  if (n_ext != 0 && n_ext != 4) return SDY_ERR_ARG;
  if (((uintptr_t)a->gen_max | (uintptr_t)a->gen_min | (uintptr_t)a->target_max | (uintptr_t)a->target_min) & 3) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, a->HW));
  if (a->bin_vars < a->win.nvars) return SDY_ERR_ARG;
  for (int g = 0; g < a->n_groups; ++g) {
    const int begin = sdy_tb_group_begin(*a, g), end = a->group_end[g];
    if (end <= begin || end > SDY_BIN_MAX_TIMES) return SDY_ERR_ARG;
    if (a->group_bin[g] < 0 || a->group_bin[g] >= a->n_bins) return SDY_ERR_ARG;
    for (int h = 0; h < g; ++h)
      if (a->group_bin[h] == a->group_bin[g]) return SDY_ERR_ARG;
    for (int i = begin; i < end; ++i) {
      if ((int)a->times[i] >= a->win.T) return SDY_ERR_ARG;
      if (i > begin && a->times[i] <= a->times[i - 1]) return SDY_ERR_ARG;
      for (int j = 0; j < begin; ++j)
        if (a->times[j] == a->times[i]) return SDY_ERR_ARG;
    }
  }
  // 64-bit flat accumulator indices: bin_vars < 2^31, n_bins < 2^31, (n0 + 1) * n1 < 2^32, HW <= 2^30
  const long per_var = ((long)a->win.n0 + 1) * a->win.n1 * a->HW;      // < 2^62
  if (per_var >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  const long vars = (long)a->n_bins * a->bin_vars;                     // < 2^62
  if (vars >= (1L << 50) || vars >= (1L << 50) / per_var) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

template <int W, bool POOL, bool EXT>
int launch(const sdy_binned_sum_args* a, hipStream_t stream) {
  const unsigned long rows = (unsigned long)gen_acc_rows(*a) + a->win.n1;
  const unsigned long n_items = rows * (unsigned long)(a->HW / W);
  const dim3 grid(sdy_grid_cap((n_items + kThreads - 1) / kThreads, a->win.nvars, kBlocksPerLaunch, kMinBlocksPerVar),
                  a->win.nvars);
  hipLaunchKernelGGL((binned_sum_kernel<W, POOL, EXT>), grid, dim3(kThreads), 0, stream, *a, n_items);
  return sdy_launch_status();
}

template <int W>
int launch_w(const sdy_binned_sum_args* a, hipStream_t stream) {
  if (a->pool_members) return has_extremes(a) ? launch<W, true, true>(a, stream) : launch<W, true, false>(a, stream);
  return has_extremes(a) ? launch<W, false, true>(a, stream) : launch<W, false, false>(a, stream);
}

}  // namespace

extern "C" int sdy_binned_time_accumulate_host(const sdy_binned_sum_args* a) {
  SDY_TRY(check_args(a));
  const sdy_window& w = a->win;
  const bool ext = has_extremes(a), pool = a->pool_members != 0;
  const long HW = a->HW, gen_rows = gen_acc_rows(*a);
  // one accumulator row of one variable: `inner` source rows `inner_stride` apart are added inside each time
  auto add_row = [&](const float* src, int inner, long inner_stride, long at, long bin_stride, double* sums, float* maxs, float* mins) {
    for (int g = 0; g < a->n_groups; ++g) {
      const int begin = sdy_tb_group_begin(*a, g), end = a->group_end[g];
      const long e = at + (long)a->group_bin[g] * bin_stride;
      for (long p = 0; p < HW; ++p) {
        double s = sums[e + p];
        float hi = ext ? maxs[e + p] : 0.0f, lo = ext ? mins[e + p] : 0.0f;
        for (int i = begin; i < end; ++i)
          for (int m = 0; m < inner; ++m) {
            const float x = src[(long)a->times[i] * HW + m * inner_stride + p];
            s = sdy_tb_add(s, x);
            hi = sdy_tb_max(hi, x);
            lo = sdy_tb_min(lo, x);
          }
        sums[e + p] = s;
        if (ext) {
          maxs[e + p] = hi;
          mins[e + p] = lo;
        }
      }
    }
  };
  for (int v = 0; v < w.nvars; ++v) {
    for (long r = 0; r < gen_rows; ++r) {
      const float* src = pool ? w.gen[v] + r * w.gs1 : w.gen[v] + (r / w.n1) * w.gs0 + (r % w.n1) * w.gs1;
      add_row(src, pool ? w.n0 : 1, w.gs0, ((long)v * gen_rows + r) * HW, (long)a->bin_vars * gen_rows * HW, a->gen_sum, a->gen_max,
              a->gen_min);
    }
    for (long i1 = 0; i1 < w.n1; ++i1)
      add_row(w.target[v] + i1 * w.ts1, 1, 0, ((long)v * w.n1 + i1) * HW, (long)a->bin_vars * w.n1 * HW, a->target_sum,
              a->target_max, a->target_min);
  }
  return SDY_OK;
}

extern "C" int sdy_binned_time_accumulate(const sdy_binned_sum_args* a, void* stream) {
  SDY_TRY(check_args(a));
  if (a->n_groups == 0) return SDY_OK;       // nothing counted
  // 16-byte loads of the window, 32-byte accesses of the sums and 16-byte ones of the extremes; HW % 4 == 0 then keeps every
  // block of the accumulators aligned
  bool vec = sdy_window_vec4(&a->win, a->HW) && (((uintptr_t)a->gen_sum | (uintptr_t)a->target_sum) & 31) == 0;
  if (has_extremes(a))
    vec = vec && (((uintptr_t)a->gen_max | (uintptr_t)a->gen_min | (uintptr_t)a->target_max | (uintptr_t)a->target_min) & 15) == 0;
  return vec ? launch_w<4>(a, (hipStream_t)stream) : launch_w<1>(a, (hipStream_t)stream);
}

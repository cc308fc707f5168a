// Transient-eddy covariances of groups of variables at every grid point (no counterpart in the reference), gfx950.
//   sdy_time_covariance_accumulate: all groups of one K of one window in one launch, read in place through the strided views the
//     window driver hands over.  The state of a group, trajectory and grid point -- K + K (K + 1) / 2 float64 sums and the K fp32
//     origins -- stays on the device and carries the run across window boundaries.  HBM-bound streaming: a work item owns W
//     grid points of one trajectory of one group, reads the K variables' values of a time together (a variable that takes part
//     in several pairs is read once), reads and writes the state once; exactly one thread owns a state element: no atomics, no
//     LDS.  K and W are template arguments: every per-variable and per-pair array is indexed at compile time and stays in
//     registers.
//   sdy_time_covariance_maps: elementwise, the state of one group -> covariance and correlation of one pair.
//   sdy_time_covariance_stats: once per get_logs, reduce -> combine.  One thread per (sample, grid point) walks the members and
//     reads a member's state once for all pairs; a slot's terms are added over a wave by a butterfly, over the four waves in
//     order, and a second launch adds the blocks' partials in block order (ordered_sum.h).
// The arithmetic of an element and of a grid point is time_covariance.h.
#include <vector>

#include "common.h"
#include "ordered_sum.h"
#include "time_covariance.h"
#include "window.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBlocksPerLaunch = 1024;  // over all groups; a group with more work strides over its items
constexpr int kMinBlocksPerGroup = 32;

// Points per work item and independent times a thread requests before it consumes the first, per K (NOTEBOOK.md, "Eddy
// covariances"): four points keep the 16-byte loads of the window and make the state accesses 32 bytes; the times in flight are
// what the registers of two waves per SIMD leave once the state of 4 K + 4 NP doubles is held.
// A/B builds of the alternatives: EXTRA="-DSDY_TC_TIMES_K4=3" and the like (Makefile), measured with tools/eddy_bench.py.
#ifndef SDY_TC_POINTS
#define SDY_TC_POINTS 4
#endif
#ifndef SDY_TC_TIMES_K2
#define SDY_TC_TIMES_K2 6
#endif
#ifndef SDY_TC_TIMES_K3
#define SDY_TC_TIMES_K3 4
#endif
#ifndef SDY_TC_TIMES_K4
#define SDY_TC_TIMES_K4 2
#endif
static_assert(SDY_TC_POINTS == 4 || SDY_TC_POINTS == 1, "two points per work item would give up the 16-byte loads");
template <int K>
struct Shape;
template <>
struct Shape<2> {
  static constexpr int W = SDY_TC_POINTS, kTimes = SDY_TC_TIMES_K2;
};
template <>
struct Shape<3> {
  static constexpr int W = SDY_TC_POINTS, kTimes = SDY_TC_TIMES_K3;
};
template <>
struct Shape<4> {
  static constexpr int W = SDY_TC_POINTS, kTimes = SDY_TC_TIMES_K4;
};

typedef double f64x4 __attribute__((ext_vector_type(4)));

// the state of a work item's W points as one value: 32-byte accesses (two 16-byte instructions) when W == 4
template <int W>
using Sums = std::conditional_t<W == 4, f64x4, double>;
__device__ __forceinline__ double sum_of(double v, int) { return v; }
__device__ __forceinline__ double sum_of(f64x4 v, int k) { return v[k]; }
__device__ __forceinline__ void set_sum(double& v, int, double x) { v = x; }
__device__ __forceinline__ void set_sum(f64x4& v, int k, double x) { v[k] = x; }
__device__ __forceinline__ void set_comp(float& v, int, float x) { v = x; }
__device__ __forceinline__ void set_comp(f32x4& v, int k, float x) { v[k] = x; }

// Work item idx of group blockIdx.y: W grid points (4 or 1) at point W * q of state row r, idx = r * (HW / W) + q; rows
// 0 .. n0*n1 - 1 are the generated rows (member i0 = r / n1, sample i1 = r % n1), rows n0*n1 .. n0*n1 + n1 - 1 the target's.
// Consecutive lanes touch consecutive addresses of every time and of the state.  Every index is bounded by the entry point:
// r < n0*n1 + n1 < 2^32, q * W < HW, t < T with T * HW <= 2^30, members[g][k] < nvars, state indices < 2^50.
template <int K, int W, int kTimes>
__global__ __launch_bounds__(kThreads) void time_covariance_kernel(const sdy_time_covariance_args a, unsigned long n_items) {
  constexpr int NP = sdy_tc_pairs(K);
  const int g = blockIdx.y;
  const unsigned long per_row = (unsigned long)(a.HW / W);
  const unsigned long gen_rows = (unsigned long)a.win.n0 * (unsigned long)a.win.n1;
  const unsigned long rows = gen_rows + (unsigned long)a.win.n1;
  const long HW = a.HW;
  const int T = a.win.T;
  const bool first = a.first != 0;
  for (unsigned long idx = (unsigned long)blockIdx.x * kThreads + threadIdx.x; idx < n_items;
       idx += (unsigned long)gridDim.x * kThreads) {
    const unsigned long r = idx / per_row, q = idx - r * per_row;
    long off;                                                // of the item's first time from a variable's base
    if (r < gen_rows) {
      const unsigned long i0 = r / (unsigned)a.win.n1, i1 = r - i0 * (unsigned)a.win.n1;
      off = (long)i0 * a.win.gs0 + (long)i1 * a.win.gs1;
    } else {
      off = (long)(r - gen_rows) * a.win.ts1;
    }
    off += (long)q * W;
    const float* src[K];
#pragma unroll
    for (int k = 0; k < K; ++k) src[k] = (r < gen_rows ? a.win.gen[a.members[g][k]] : a.win.target[a.members[g][k]]) + off;
    const long at = (long)r * HW + (long)q * W;              // within a (rows, HW) block
    const long block = (long)rows * HW;
    Sums<W>* ps[K];
    Vec<W>* pc[K];
    Sums<W>* pp[NP];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      ps[k] = reinterpret_cast<Sums<W>*>(a.sums + ((long)g * K + k) * block + at);
      pc[k] = reinterpret_cast<Vec<W>*>(a.origins + ((long)g * K + k) * block + at);
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) pp[k] = reinterpret_cast<Sums<W>*>(a.products + ((long)g * NP + k) * block + at);
    // the state and the first kTimes times are requested together; a batch past the end of the window re-reads the last time
    // (from cache) and adds nothing
    double s[W][K], p[W][NP];
    float c[W][K];
#pragma unroll
    for (int e = 0; e < W; ++e) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        s[e][k] = 0.0;
        c[e][k] = 0.0f;
      }
#pragma unroll
      for (int k = 0; k < NP; ++k) p[e][k] = 0.0;
    }
    if (!first) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const Sums<W> vs = *ps[k];
        const Vec<W> vc = *pc[k];
#pragma unroll
        for (int e = 0; e < W; ++e) {
          s[e][k] = sum_of(vs, e);
          c[e][k] = comp(vc, e);
        }
      }
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const Sums<W> vp = *pp[k];
#pragma unroll
        for (int e = 0; e < W; ++e) p[e][k] = sum_of(vp, e);
      }
    }
    for (int t = a.t0; t < T; t += kTimes) {
      Vec<W> x[kTimes][K];
#pragma unroll
      for (int i = 0; i < kTimes; ++i)
#pragma unroll
        for (int k = 0; k < K; ++k) x[i][k] = ld<W>(src[k] + (long)(t + i < T ? t + i : T - 1) * HW);
      if (first && t == a.t0) {
#pragma unroll
        for (int e = 0; e < W; ++e)
#pragma unroll
          for (int k = 0; k < K; ++k) c[e][k] = comp(x[0][k], e);   // the origins: the trajectory's first counted values
      }
#pragma unroll
      for (int i = 0; i < kTimes; ++i)
        if (t + i < T) {
#pragma unroll
          for (int e = 0; e < W; ++e) {
            double d[K];
#pragma unroll
            for (int k = 0; k < K; ++k) d[k] = sdy_tc_dev(comp(x[i][k], e), c[e][k]);
            sdy_tc_step<K>(s[e], p[e], d);
          }
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      Sums<W> vs;
      Vec<W> vc;
#pragma unroll
      for (int e = 0; e < W; ++e) {
        set_sum(vs, e, s[e][k]);
        set_comp(vc, e, c[e][k]);
      }
      *ps[k] = vs;
      *pc[k] = vc;
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      Sums<W> vp;
#pragma unroll
      for (int e = 0; e < W; ++e) set_sum(vp, e, p[e][k]);
      *pp[k] = vp;
    }
  }
}

// one thread per element of the group's (rows, HW)
__global__ __launch_bounds__(kThreads) void time_covariance_maps_kernel(const sdy_time_covariance_maps_args a) {
  const long e = (long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= a.n_elems) return;
  const int K = a.K, i = a.i, j = a.j;
  const sdy_tc_moments r =
      sdy_tc_finish(a.sums[(long)i * a.n_elems + e], a.sums[(long)j * a.n_elems + e],
                    a.products[(long)sdy_tc_pair_index(K, i, i) * a.n_elems + e],
                    a.products[(long)sdy_tc_pair_index(K, j, j) * a.n_elems + e],
                    a.products[(long)sdy_tc_pair_index(K, i, j) * a.n_elems + e], a.n_times, i == j);
  a.cov[e] = r.cov;
  a.corr[e] = r.corr;
}

// the sums of group g, row `row` (member i: i * n1 + sample; the target: M * n1 + sample), grid point `point` -- host and device
template <int K>
__host__ __device__ inline sdy_tc_state<K> load_state(const sdy_time_covariance_stats_args& a, int g, long row, long point) {
  constexpr int NP = sdy_tc_pairs(K);
  const long block = ((long)a.M + 1) * a.n1 * a.HW, at = row * a.HW + point;
  sdy_tc_state<K> st;
#pragma unroll
  for (int k = 0; k < K; ++k) st.s[k] = a.sums[((long)g * K + k) * block + at];
#pragma unroll
  for (int k = 0; k < NP; ++k) st.p[k] = a.products[((long)g * NP + k) * block + at];
  return st;
}

template <int K>
__host__ __device__ inline sdy_tc_state<K> zero_state() {
  sdy_tc_state<K> st;
#pragma unroll
  for (int k = 0; k < K; ++k) st.s[k] = 0.0;
#pragma unroll
  for (int k = 0; k < sdy_tc_pairs(K); ++k) st.p[k] = 0.0;
  return st;
}

// grid (chunks of kThreads points of the n1 * HW of a group, n_groups).  partials: (n_groups, chunks, NP, SDY_TC_SLOTS).
template <int K>
__global__ __launch_bounds__(kThreads) void time_covariance_stats_kernel(const sdy_time_covariance_stats_args a, double* partials) {
  constexpr int NS = sdy_tc_pairs(K) * SDY_TC_SLOTS;
  __shared__ double sh[kWaves][NS];
  const int g = blockIdx.y, M = a.M;
  const long n = (long)a.n1 * a.HW;                          // <= 2^30
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;  // sample * HW + grid point
  const bool active = p < n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long sample = active ? p / a.HW : 0, point = active ? p - sample * a.HW : 0;
  // an idle lane reads nothing and contributes 0 to every slot
  auto state = [&](int i) { return active ? load_state<K>(a, g, (long)i * a.n1 + sample, point) : zero_state<K>(); };
  auto emit = [&](int pair, int slot, double x) {
    if (!active) x = 0.0;
    sdy_wave_sum(x);
    if (lane == 0) sh[wave][pair * SDY_TC_SLOTS + slot] = x;
  };
  const double w = active ? (double)a.weights[point] : 0.0;
  sdy_tc_point<K>(M, a.n_times, w, state(M), state, emit);
  __syncthreads();
  double* out = partials + ((long)g * gridDim.x + blockIdx.x) * NS;
  if (threadIdx.x < NS) out[threadIdx.x] = sdy_fold_rows(sh, threadIdx.x);
}

long n_chunks(long n) { return (n + kThreads - 1) / kThreads; }

bool k_ok(int K) { return K >= 2 && K <= SDY_TC_MAX_K; }

// the window's own checks are sdy_window_check's; here the groups, the time offset and what bounds a state address
int check_accumulate(const sdy_time_covariance_args* a) {
  if (!a || a->struct_size != sizeof(sdy_time_covariance_args)) return SDY_ERR_ARG;
  if (!k_ok(a->K) || a->n_groups < 1 || a->n_groups > SDY_TC_MAX_GROUPS) return SDY_ERR_ARG;
  if (a->t0 < 0 || a->t0 >= a->win.T) return SDY_ERR_ARG;
  if (!a->sums || !a->products || !a->origins) return SDY_ERR_ARG;
  if ((((uintptr_t)a->sums | (uintptr_t)a->products) & 7) || ((uintptr_t)a->origins & 3)) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, a->HW));
  for (int g = 0; g < a->n_groups; ++g)
    for (int k = 0; k < a->K; ++k) {
      const int v = a->members[g][k];
      if (v < 0 || v >= a->win.nvars) return SDY_ERR_ARG;
      for (int l = 0; l < k; ++l)
        if (a->members[g][l] == v) return SDY_ERR_ARG;
    }
  // 64-bit flat state indices: n_groups * NP <= 320 < 2^9, (n0 + 1) * n1 < 2^32, HW <= 2^30 -- the product can leave 2^50
  const long per_block = ((long)a->win.n0 + 1) * a->win.n1 * a->HW;      // < 2^62
  if (per_block >= (1L << 50) || (long)a->n_groups * sdy_tc_pairs(a->K) * per_block >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

int check_maps(const sdy_time_covariance_maps_args* a) {
  if (!a || a->struct_size != sizeof(sdy_time_covariance_maps_args)) return SDY_ERR_ARG;
  if (!k_ok(a->K) || a->i < 0 || a->j >= a->K || a->i > a->j) return SDY_ERR_ARG;
  if (a->n_elems < 1) return SDY_ERR_ARG;
  if (!a->sums || !a->products || !a->cov || !a->corr) return SDY_ERR_ARG;
  if (((uintptr_t)a->sums | (uintptr_t)a->products | (uintptr_t)a->cov | (uintptr_t)a->corr) & 7) return SDY_ERR_ARG;
  if (!(a->n_times >= 1.0) || !std::isfinite(a->n_times)) return SDY_ERR_ARG;
  if (a->n_elems >= (1L << 50) / sdy_tc_pairs(a->K)) return SDY_ERR_UNSUPPORTED;
  if (a->n_elems > (long)kThreads * 0x7fffffffL) return SDY_ERR_UNSUPPORTED;     // blocks of one launch
  return SDY_OK;
}

int check_stats(const sdy_time_covariance_stats_args* a, bool need_ws) {
  if (!a || a->struct_size != sizeof(sdy_time_covariance_stats_args)) return SDY_ERR_ARG;
  if (!k_ok(a->K) || a->n_groups < 1 || a->n_groups > SDY_TC_MAX_GROUPS) return SDY_ERR_ARG;
  if (a->M < 1 || a->n1 < 1 || a->HW < 1) return SDY_ERR_ARG;
  if (!a->sums || !a->products || !a->weights || !a->out) return SDY_ERR_ARG;
  if ((((uintptr_t)a->sums | (uintptr_t)a->products | (uintptr_t)a->out) & 7) || ((uintptr_t)a->weights & 3)) return SDY_ERR_ARG;
  if (!(a->n_times >= 1.0) || !std::isfinite(a->n_times)) return SDY_ERR_ARG;
  if ((long)a->n1 * a->HW > (1L << 30)) return SDY_ERR_UNSUPPORTED;
  if ((long)a->n_groups * sdy_tc_pairs(a->K) * ((long)a->M + 1) * ((long)a->n1 * a->HW) >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  if (need_ws && !sdy_ws_ok(a->ws, a->ws_bytes, sdy_time_covariance_workspace_bytes(a->K, a->n_groups, a->n1, a->HW)))
    return SDY_ERR_ARG;
  return SDY_OK;
}

template <int K>
void accumulate_host(const sdy_time_covariance_args* a) {
  constexpr int NP = sdy_tc_pairs(K);
  const sdy_window& w = a->win;
  const long HW = a->HW, rows = ((long)w.n0 + 1) * w.n1, block = rows * HW;
  const bool first = a->first != 0;
  for (int g = 0; g < a->n_groups; ++g)
    for (long r = 0; r < rows; ++r) {
      const float* src[K];
      for (int k = 0; k < K; ++k) {
        const int v = a->members[g][k];
        src[k] = r < (long)w.n0 * w.n1 ? w.gen[v] + (r / w.n1) * w.gs0 + (r % w.n1) * w.gs1 : w.target[v] + (r - (long)w.n0 * w.n1) * w.ts1;
      }
      for (long e = 0; e < HW; ++e) {
        const long at = r * HW + e;
        double s[K], p[NP];
        float c[K];
        for (int k = 0; k < K; ++k) {
          s[k] = first ? 0.0 : a->sums[((long)g * K + k) * block + at];
          c[k] = first ? src[k][(long)a->t0 * HW + e] : a->origins[((long)g * K + k) * block + at];
        }
        for (int k = 0; k < NP; ++k) p[k] = first ? 0.0 : a->products[((long)g * NP + k) * block + at];
        for (int t = a->t0; t < w.T; ++t) {
          double d[K];
          for (int k = 0; k < K; ++k) d[k] = sdy_tc_dev(src[k][(long)t * HW + e], c[k]);
          sdy_tc_step<K>(s, p, d);
        }
        for (int k = 0; k < K; ++k) {
          a->sums[((long)g * K + k) * block + at] = s[k];
          a->origins[((long)g * K + k) * block + at] = c[k];
        }
        for (int k = 0; k < NP; ++k) a->products[((long)g * NP + k) * block + at] = p[k];
      }
    }
}

template <int K, int W>
int launch_accumulate(const sdy_time_covariance_args* a, hipStream_t stream) {
  const unsigned long rows = (unsigned long)a->win.n0 * a->win.n1 + a->win.n1;
  const unsigned long n_items = rows * (unsigned long)(a->HW / W);
  const dim3 grid(sdy_grid_cap((n_items + kThreads - 1) / kThreads, a->n_groups, kBlocksPerLaunch, kMinBlocksPerGroup), a->n_groups);
  hipLaunchKernelGGL((time_covariance_kernel<K, W, Shape<K>::kTimes>), grid, dim3(kThreads), 0, stream, *a, n_items);
  return sdy_launch_status();
}

template <int K>
int accumulate(const sdy_time_covariance_args* a, hipStream_t stream) {
  // Shape<K>::W points per work item: 16-byte loads of the window, 32-byte accesses of the sums and 16-byte ones of the origins
  constexpr int W = Shape<K>::W;
  const long block = ((long)a->win.n0 + 1) * a->win.n1 * a->HW;
  const bool vec = sdy_window_vec4(&a->win, a->HW) && (((uintptr_t)a->sums | (uintptr_t)a->products) & 31) == 0 &&
                   ((uintptr_t)a->origins & 15) == 0 && (block & 3) == 0;
  return vec ? launch_accumulate<K, W>(a, stream) : launch_accumulate<K, 1>(a, stream);
}

template <int K>
void stats_host(const sdy_time_covariance_stats_args* a) {
  constexpr int NS = sdy_tc_pairs(K) * SDY_TC_SLOTS;
  const int M = a->M;
  const long n = (long)a->n1 * a->HW, chunks = n_chunks(n);
  std::vector<double> partials((size_t)chunks * NS);
  for (int g = 0; g < a->n_groups; ++g) {
    for (long c = 0; c < chunks; ++c) {
      double* part = partials.data() + c * NS;
      for (int k = 0; k < NS; ++k) part[k] = 0.0;
      for (long p = c * kThreads; p < (c + 1) * kThreads && p < n; ++p) {
        const long sample = p / a->HW, point = p - sample * a->HW;
        auto state = [&](int i) { return load_state<K>(*a, g, (long)i * a->n1 + sample, point); };
        sdy_tc_point<K>(M, a->n_times, (double)a->weights[point], state(M), state,
                        [&](int pair, int slot, double x) { part[pair * SDY_TC_SLOTS + slot] += x; });
      }
    }
    for (int k = 0; k < NS; ++k) a->out[(long)g * NS + k] = sdy_sum_chunks(partials.data(), (int)chunks, NS, k);
  }
}

template <int K>
int stats(const sdy_time_covariance_stats_args* a, hipStream_t stream) {
  const int chunks = (int)n_chunks((long)a->n1 * a->HW);
  double* partials = static_cast<double*>(a->ws);
  hipLaunchKernelGGL(time_covariance_stats_kernel<K>, dim3(chunks, a->n_groups), dim3(kThreads), 0, stream, *a, partials);
  SDY_TRY(sdy_launch_status());
  return sdy_combine_chunks_launch(partials, a->n_groups, chunks, sdy_tc_pairs(K) * SDY_TC_SLOTS, a->out, stream);
}

}  // namespace

extern "C" size_t sdy_time_covariance_workspace_bytes(int K, int n_groups, int n1, int HW) {
  if (!k_ok(K) || n_groups < 1 || n_groups > SDY_TC_MAX_GROUPS || n1 < 1 || HW < 1) return 0;
  return (size_t)n_groups * (size_t)n_chunks((long)n1 * HW) * sdy_tc_pairs(K) * SDY_TC_SLOTS * sizeof(double);
}

extern "C" int sdy_time_covariance_accumulate_host(const sdy_time_covariance_args* a) {
  SDY_TRY(check_accumulate(a));
  if (a->K == 2) accumulate_host<2>(a);
  if (a->K == 3) accumulate_host<3>(a);
  if (a->K == 4) accumulate_host<4>(a);
  return SDY_OK;
}

extern "C" int sdy_time_covariance_accumulate(const sdy_time_covariance_args* a, void* stream) {
  SDY_TRY(check_accumulate(a));
  if (a->K == 2) return accumulate<2>(a, (hipStream_t)stream);
  if (a->K == 3) return accumulate<3>(a, (hipStream_t)stream);
  return accumulate<4>(a, (hipStream_t)stream);
}

extern "C" int sdy_time_covariance_maps_host(const sdy_time_covariance_maps_args* a) {
  SDY_TRY(check_maps(a));
  const int K = a->K, i = a->i, j = a->j;
  const long n = a->n_elems;
  for (long e = 0; e < n; ++e) {
    const sdy_tc_moments r = sdy_tc_finish(a->sums[i * n + e], a->sums[j * n + e], a->products[sdy_tc_pair_index(K, i, i) * n + e],
                                           a->products[sdy_tc_pair_index(K, j, j) * n + e],
                                           a->products[sdy_tc_pair_index(K, i, j) * n + e], a->n_times, i == j);
    a->cov[e] = r.cov;
    a->corr[e] = r.corr;
  }
  return SDY_OK;
}

extern "C" int sdy_time_covariance_maps(const sdy_time_covariance_maps_args* a, void* stream) {
  SDY_TRY(check_maps(a));
  hipLaunchKernelGGL(time_covariance_maps_kernel, dim3((unsigned)n_chunks(a->n_elems)), dim3(kThreads), 0, (hipStream_t)stream, *a);
  return sdy_launch_status();
}

// The device's partition (chunks of kThreads points, then the chunks in order); inside a chunk the points are added in
// order, where the device adds them in a butterfly: the two agree to the rounding of a 256-term float64 sum.
extern "C" int sdy_time_covariance_stats_host(const sdy_time_covariance_stats_args* a) {
  SDY_TRY(check_stats(a, false));
  if (a->K == 2) stats_host<2>(a);
  if (a->K == 3) stats_host<3>(a);
  if (a->K == 4) stats_host<4>(a);
  return SDY_OK;
}

extern "C" int sdy_time_covariance_stats(const sdy_time_covariance_stats_args* a, void* stream) {
  SDY_TRY(check_stats(a, true));
  if (a->K == 2) return stats<2>(a, (hipStream_t)stream);
  if (a->K == 3) return stats<3>(a, (hipStream_t)stream);
  return stats<4>(a, (hipStream_t)stream);
}

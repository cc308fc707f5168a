// Per-grid-point quantiles along time of gen and target, exactly (no counterpart in the reference), gfx950.  Two entry points:
//   append: the variables of one window, read in place through the strided views the window driver hands over, are written as
//     sortable 32-bit keys into the series (nvars, n_traj, capacity, plane).  (variable, trajectory) is one contiguous run of
//     (T - t0) * plane values on both sides: a copy with the key transform, HBM-bound.
//   select: any set of quantiles of a group of trajectories at every grid point, by digits, most significant first -- no sort,
//     no scratch copy of the series.  A lane owns a grid point (or 4 with 16-byte loads) and walks the group's count x n_slots
//     keys once per pass with several loads in flight.  Pass 0 counts the valid keys n (the ranks differ from lane to lane
//     because n does); each of the 16 digit passes counts, per rank, the keys that share the rank's decided prefix and have the
//     next 2-bit digit below 1, 2 and 3 -- ((key ^ prefix) >> shift) < c says both at once -- and fixes the digit; one more
//     pass counts the keys <= lo and takes the smallest key above lo, which settles hi exactly.  The NaN key is the largest
//     key and has digit 3 everywhere, so it is never counted below anything and no rank < n lands on it.
// No barriers, no LDS, no atomics; every loop bound of a pass is wave-uniform.  The rank count and the load width are template
// arguments: the per-thread rank state (prefix, remaining rank, three counters per rank and point) is indexed at compile
// time only and stays in registers.  More than kRanksPerLaunch quantiles are taken in two launches: at 4 points x 4 ranks
// the state is 80 registers, and the passes are VALU-bound from 3 ranks on, so a second walk costs what the ranks cost anyway.
// The arithmetic is quantile.h.
#include <algorithm>
#include <vector>

#include "common.h"
#include "quantile.h"
#include "window.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRanksPerLaunch = 4;
// independent loads a thread issues before it consumes the first.  Every load of a batch keeps a 64-bit scalar offset alive:
// with a lane per point 16 or 32 in flight are faster (bytes in flight bound that shape, not the VALU) but spill scalar
// registers (15 .. 41), so that path stays at 8
template <int W4>
constexpr int kSlotsInFlight = W4 == 4 ? 16 : 8;
constexpr int kDigitBits = 2;
constexpr int kAppendInFlight = 4;
constexpr unsigned kAppendBlocks = 4096;  // per (variable, trajectory); a longer run strides
constexpr long kSelectBlocks = 1L << 20;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
template <int W4>
using Words = std::conditional_t<W4 == 4, u32x4, unsigned>;
__device__ __forceinline__ unsigned word_of(unsigned v, int) { return v; }
__device__ __forceinline__ unsigned word_of(u32x4 v, int k) { return v[k]; }
__device__ __forceinline__ void set_word(unsigned& v, int, unsigned x) { v = x; }
__device__ __forceinline__ void set_word(u32x4& v, int k, unsigned x) { v[k] = x; }

// ---- append ------------------------------------------------------------------------------------------------------------------
// Block (x, y, z): variable z, trajectories y, y + gridDim.y, .., units x * 256 + thread, + gridDim.x * 256, .. of the run.
// Bounds (entry point): n = (T - t0) * plane / W4 <= 2^30 units and gridDim.x * 256 * kAppendInFlight <= 2^22, so a unit number
// cannot wrap; rows < 2^32; slot0 + (T - t0) <= capacity; series indices < 2^50.
template <int W4>
__global__ __launch_bounds__(kThreads) void append_kernel(const sdy_time_quantile_append_args a) {
  const int v = blockIdx.z;
  const long plane = (long)a.H * a.W;
  const unsigned n = (unsigned)(((long)(a.win.T - a.t0) * plane) / W4);
  const unsigned n1 = (unsigned)a.win.n1;
  const unsigned gen_rows = a.store_gen ? (unsigned)a.win.n0 * n1 : 0u;
  const unsigned rows = gen_rows + n1;
  const unsigned step = gridDim.x * kThreads;
  for (unsigned r = blockIdx.y; r < rows; r += gridDim.y) {
    const float* src;
    if (r < gen_rows) {
      const unsigned i0 = r / n1, i1 = r - i0 * n1;
      src = a.win.gen[v] + (long)i0 * a.win.gs0 + (long)i1 * a.win.gs1;
    } else {
      src = a.win.target[v] + (long)(r - gen_rows) * a.win.ts1;
    }
    src += (long)a.t0 * plane;
    unsigned* const dst = a.series + sdy_q_series_at(v, rows, r, a.capacity, a.slot0, plane, 0);
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < n; i += step * kAppendInFlight) {
      // a unit past the end of the run re-reads unit i and stores nothing
      Vec<W4> x[kAppendInFlight];
#pragma unroll
      for (int k = 0; k < kAppendInFlight; ++k) {
        const unsigned at = i + k * step;
        x[k] = ld<W4>(src + (long)(at < n ? at : i) * W4);
      }
#pragma unroll
      for (int k = 0; k < kAppendInFlight; ++k) {
        const unsigned at = i + k * step;
        if (at < n) {
          Words<W4> keys;
#pragma unroll
          for (int c = 0; c < W4; ++c) set_word(keys, c, sdy_q_key(comp(x[k], c)));
          *reinterpret_cast<Words<W4>*>(dst + (long)at * W4) = keys;
        }
      }
    }
  }
}

int check(const sdy_time_quantile_append_args* a) {
  if (!a || a->struct_size != sizeof(sdy_time_quantile_append_args)) return SDY_ERR_ARG;
  if (a->H < 1 || a->W < 1) return SDY_ERR_ARG;
  const long plane = (long)a->H * a->W;
  SDY_TRY(sdy_window_check(&a->win, plane));                              // T * plane <= 2^30, n0 * n1 < 2^31
  if (!a->series || ((uintptr_t)a->series & 3)) return SDY_ERR_ARG;
  if (a->capacity < 1 || a->slot0 < 0 || a->t0 < 0 || a->t0 > a->win.T) return SDY_ERR_ARG;
  if ((long)a->slot0 + (a->win.T - a->t0) > (long)a->capacity) return SDY_ERR_ARG;
  if (a->store_gen != 0 && a->store_gen != 1) return SDY_ERR_ARG;
  // 64-bit flat indices, compared factor by factor: n_traj < 2^32 and nvars <= 96, plane <= 2^30, capacity < 2^31
  const long n_traj = sdy_q_trajectories(a->win.n0, a->win.n1, a->store_gen);
  const long limit = 1L << 50;
  if (n_traj * (long)a->win.nvars >= limit / plane) return SDY_ERR_UNSUPPORTED;
  if (n_traj * (long)a->win.nvars * plane > (limit - 1) / a->capacity) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

bool vec4(const sdy_time_quantile_append_args* a) {
  return sdy_window_vec4(&a->win, (long)a->H * a->W) && ((uintptr_t)a->series & 15) == 0;
}

// ---- select ------------------------------------------------------------------------------------------------------------------
// Every key of the group of the W4 points at `base`: trajectory i at base + i * tstride, slot s at + s * plane; f(key, point).
// A batch past the last slot re-reads the last slot (from cache) and uses nothing of it.
// Bounds (entry point): the group's trajectories < n_traj, n_slots <= capacity, the points inside the plane.
template <int W4, class Fn>
__device__ __forceinline__ void walk(const unsigned* base, int count, long tstride, int n_slots, long plane, Fn&& f) {
  for (int i = 0; i < count; ++i) {
    const unsigned* const row = base + (long)i * tstride;
    for (int s = 0; s < n_slots; s += kSlotsInFlight<W4>) {
      Words<W4> x[kSlotsInFlight<W4>];
#pragma unroll
      for (int k = 0; k < kSlotsInFlight<W4>; ++k)
        x[k] = *reinterpret_cast<const Words<W4>*>(row + (long)(s + k < n_slots ? s + k : n_slots - 1) * plane);
#pragma unroll
      for (int k = 0; k < kSlotsInFlight<W4>; ++k)
        if (s + k < n_slots) {
#pragma unroll
          for (int c = 0; c < W4; ++c) f(word_of(x[k], c), c);
        }
    }
  }
}

// Quantiles q0 .. q0 + NQ - 1 of a.q.  Item = (group, unit of W4 points), 64-bit, grid-strided.
template <int W4, int NQ>
__global__ __launch_bounds__(kThreads) void select_kernel(const sdy_time_quantile_select_args a, int q0) {
  const long plane = a.plane;
  const long units = plane / W4;
  const long items = (long)a.n_groups * units;
  const long tstride = (long)a.stride * a.capacity * plane;
  const int count = a.count, n_slots = a.n_slots, method = a.method;
  for (long item = (long)blockIdx.x * kThreads + threadIdx.x; item < items; item += (long)gridDim.x * kThreads) {
    const long g = item / units, p = (item - g * units) * W4;
    const unsigned* const base = a.series + ((long)a.first + g * a.step) * a.capacity * plane + p;
    unsigned n[W4];
#pragma unroll
    for (int c = 0; c < W4; ++c) n[c] = 0u;
    walk<W4>(base, count, tstride, n_slots, plane, [&](unsigned key, int c) { n[c] += key != SDY_Q_NAN_KEY ? 1u : 0u; });
    // the rank of lo per (quantile, point); a point without values walks along with rank 0 and is NaN at the end
    unsigned prefix[NQ][W4], k[NQ][W4];
#pragma unroll
    for (int r = 0; r < NQ; ++r)
#pragma unroll
      for (int c = 0; c < W4; ++c) {
        double frac;
        prefix[r][c] = 0u;
        k[r][c] = n[c] != 0u ? sdy_q_rank(a.q[q0 + r], n[c], frac) : 0u;
      }
    for (int shift = 32 - kDigitBits; shift >= 0; shift -= kDigitBits) {
      unsigned c1[NQ][W4], c2[NQ][W4], c3[NQ][W4];
#pragma unroll
      for (int r = 0; r < NQ; ++r)
#pragma unroll
        for (int c = 0; c < W4; ++c) c1[r][c] = c2[r][c] = c3[r][c] = 0u;
      walk<W4>(base, count, tstride, n_slots, plane, [&](unsigned key, int c) {
#pragma unroll
        for (int r = 0; r < NQ; ++r) {
          // < 4 exactly when the decided digits match (the undecided ones of the prefix are 0); then it is the next digit
          const unsigned t = (key ^ prefix[r][c]) >> shift;
          c1[r][c] += t < 1u ? 1u : 0u;
          c2[r][c] += t < 2u ? 1u : 0u;
          c3[r][c] += t < 3u ? 1u : 0u;
        }
      });
#pragma unroll
      for (int r = 0; r < NQ; ++r)
#pragma unroll
        for (int c = 0; c < W4; ++c) {
          const unsigned kk = k[r][c];
          const unsigned d = (kk >= c1[r][c] ? 1u : 0u) + (kk >= c2[r][c] ? 1u : 0u) + (kk >= c3[r][c] ? 1u : 0u);
          const unsigned below = d == 0u ? 0u : d == 1u ? c1[r][c] : d == 2u ? c2[r][c] : c3[r][c];
          k[r][c] = kk - below;
          prefix[r][c] |= d << shift;
        }
    }
    // prefix is the key of lo.  hi: the keys <= lo and the smallest key above it
    unsigned le[NQ][W4], next[NQ][W4];
#pragma unroll
    for (int r = 0; r < NQ; ++r)
#pragma unroll
      for (int c = 0; c < W4; ++c) {
        le[r][c] = 0u;
        next[r][c] = SDY_Q_NAN_KEY;
      }
    if (method != SDY_Q_LOWER)                   // wave-uniform
      walk<W4>(base, count, tstride, n_slots, plane, [&](unsigned key, int c) {
#pragma unroll
        for (int r = 0; r < NQ; ++r) {
          const bool above = key > prefix[r][c];
          le[r][c] += above ? 0u : 1u;
          const unsigned cand = above ? key : SDY_Q_NAN_KEY;
          next[r][c] = cand < next[r][c] ? cand : next[r][c];
        }
      });
#pragma unroll
    for (int r = 0; r < NQ; ++r) {
      double* const out = a.out + ((g * a.nq + q0 + r) * plane + p);
#pragma unroll
      for (int c = 0; c < W4; ++c) {
        double res = __builtin_nan("");
        if (n[c] != 0u) {
          double frac;
          const unsigned j = sdy_q_rank(a.q[q0 + r], n[c], frac);
          const unsigned lo = prefix[r][c];
          const unsigned hi = method != SDY_Q_LOWER ? sdy_q_hi_key(lo, j, n[c], le[r][c], next[r][c]) : lo;
          res = sdy_q_quantile((double)sdy_q_value_of(lo), (double)sdy_q_value_of(hi), frac, method);
        }
        out[c] = res;
      }
    }
    if (q0 == 0) {
#pragma unroll
      for (int c = 0; c < W4; ++c) a.valid[g * plane + p + c] = (int)n[c];
    }
  }
}

int check(const sdy_time_quantile_select_args* a) {
  if (!a || a->struct_size != sizeof(sdy_time_quantile_select_args)) return SDY_ERR_ARG;
  if (!a->series || !a->out || !a->valid) return SDY_ERR_ARG;
  if (((uintptr_t)a->series & 3) || ((uintptr_t)a->out & 7) || ((uintptr_t)a->valid & 3)) return SDY_ERR_ARG;
  if (a->plane < 1 || a->n_traj < 1 || a->capacity < 1 || a->n_slots < 1 || a->count < 1 || a->n_groups < 1) return SDY_ERR_ARG;
  if (a->n_slots > a->capacity || a->first < 0 || a->step < 0 || a->stride < 0) return SDY_ERR_ARG;
  // the last trajectory of the last group (each factor < 2^31: the sum fits a long)
  if ((long)a->first + (long)(a->n_groups - 1) * a->step + (long)(a->count - 1) * a->stride >= (long)a->n_traj) return SDY_ERR_ARG;
  if (a->nq < 1 || a->nq > SDY_MAX_QUANTILES || a->method < SDY_Q_LINEAR || a->method > SDY_Q_HIGHER) return SDY_ERR_ARG;
  for (int i = 0; i < a->nq; ++i)
    if (!(a->q[i] >= 0.0 && a->q[i] <= 1.0)) return SDY_ERR_ARG;          // (a NaN fails both comparisons)
  if (a->plane > (1L << 30)) return SDY_ERR_UNSUPPORTED;
  if ((long)a->count * a->n_slots >= (1L << 31)) return SDY_ERR_UNSUPPORTED;   // 32-bit counts and ranks
  // 64-bit flat indices: n_traj * capacity < 2^62, plane <= 2^30
  const long limit = 1L << 50;
  if ((long)a->n_traj * a->capacity > (limit - 1) / a->plane) return SDY_ERR_UNSUPPORTED;
  if ((long)a->n_groups * a->nq > (limit - 1) / a->plane) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

template <int NQ>
void launch(const sdy_time_quantile_select_args& a, int q0, bool vec, hipStream_t stream) {
  const long items = (long)a.n_groups * (a.plane / (vec ? 4 : 1));
  const long blocks = (items + kThreads - 1) / kThreads;
  const dim3 grid((unsigned)(blocks < kSelectBlocks ? blocks : kSelectBlocks));
  if (vec)
    hipLaunchKernelGGL((select_kernel<4, NQ>), grid, dim3(kThreads), 0, stream, a, q0);
  else
    hipLaunchKernelGGL((select_kernel<1, NQ>), grid, dim3(kThreads), 0, stream, a, q0);
}

}  // namespace

extern "C" int sdy_time_quantile_append_host(const sdy_time_quantile_append_args* a) {
  SDY_TRY(check(a));
  const sdy_window& w = a->win;
  const long plane = (long)a->H * a->W;
  const long gen_rows = a->store_gen ? (long)w.n0 * w.n1 : 0, rows = gen_rows + w.n1;
  for (int v = 0; v < w.nvars; ++v)
    for (long r = 0; r < rows; ++r) {
      const float* src = r < gen_rows ? w.gen[v] + (r / w.n1) * w.gs0 + (r % w.n1) * w.gs1 : w.target[v] + (r - gen_rows) * w.ts1;
      for (long t = a->t0; t < w.T; ++t)
        for (long p = 0; p < plane; ++p)
          a->series[sdy_q_series_at(v, rows, r, a->capacity, a->slot0 + (t - a->t0), plane, p)] = sdy_q_key(src[t * plane + p]);
    }
  return SDY_OK;
}

extern "C" int sdy_time_quantile_append(const sdy_time_quantile_append_args* a, void* stream) {
  SDY_TRY(check(a));
  if (a->win.T - a->t0 == 0) return SDY_OK;        // a window that holds the initial condition only
  const bool vec = vec4(a);
  const long plane = (long)a->H * a->W;
  const long n = (long)(a->win.T - a->t0) * plane / (vec ? 4 : 1);
  const long want = (n + (long)kThreads * kAppendInFlight - 1) / ((long)kThreads * kAppendInFlight);
  const long rows = sdy_q_trajectories(a->win.n0, a->win.n1, a->store_gen);
  const dim3 grid((unsigned)(want < kAppendBlocks ? want : kAppendBlocks), (unsigned)(rows < 65535 ? rows : 65535), a->win.nvars);
  if (vec)
    hipLaunchKernelGGL((append_kernel<4>), grid, dim3(kThreads), 0, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL((append_kernel<1>), grid, dim3(kThreads), 0, (hipStream_t)stream, *a);
  return sdy_launch_status();
}

extern "C" int sdy_time_quantile_select_host(const sdy_time_quantile_select_args* a) {
  SDY_TRY(check(a));
  const long plane = a->plane;
  std::vector<unsigned> keys;
  keys.reserve((size_t)a->count * a->n_slots);
  for (long g = 0; g < a->n_groups; ++g)
    for (long p = 0; p < plane; ++p) {
      keys.clear();
      for (long i = 0; i < a->count; ++i)
        for (long s = 0; s < a->n_slots; ++s) {
          const unsigned key = a->series[sdy_q_series_at(0, a->n_traj, a->first + g * a->step + i * a->stride, a->capacity, s, plane, p)];
          if (key != SDY_Q_NAN_KEY) keys.push_back(key);
        }
      std::sort(keys.begin(), keys.end());
      const unsigned n = (unsigned)keys.size();
      a->valid[g * plane + p] = (int)n;
      for (int i = 0; i < a->nq; ++i) {
        double res = __builtin_nan("");
        if (n != 0u) {
          double frac;
          const unsigned j = sdy_q_rank(a->q[i], n, frac);
          const unsigned r = j + 1u < n - 1u ? j + 1u : n - 1u;
          res = sdy_q_quantile((double)sdy_q_value_of(keys[j]), (double)sdy_q_value_of(keys[r]), frac, a->method);
        }
        a->out[(g * a->nq + i) * plane + p] = res;
      }
    }
  return SDY_OK;
}

extern "C" int sdy_time_quantile_select(const sdy_time_quantile_select_args* a, void* stream) {
  SDY_TRY(check(a));
  // 16-byte loads need 4 points per lane: taken when that still leaves two waves for every SIMD, else a lane per point
  int n_cu = 0;
  SDY_TRY(sdy_cu_count(&n_cu));
  const bool vec = (a->plane & 3) == 0 && ((uintptr_t)a->series & 15) == 0 &&
                   (long)a->n_groups * (a->plane / 4) >= (long)n_cu * 4 * 64 * 2;
  const hipStream_t s = (hipStream_t)stream;
  for (int q0 = 0; q0 < a->nq; q0 += kRanksPerLaunch) {
    switch (a->nq - q0 < kRanksPerLaunch ? a->nq - q0 : kRanksPerLaunch) {
      case 1: launch<1>(*a, q0, vec, s); break;
      case 2: launch<2>(*a, q0, vec, s); break;
      case 3: launch<3>(*a, q0, vec, s); break;
      case 4: launch<4>(*a, q0, vec, s); break;
    }
  }
  return sdy_launch_status();
}

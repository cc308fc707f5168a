// Threshold events of an ensemble (no counterpart in the reference), gfx950: the integer counts behind Brier score,
// reliability diagram, ROC curve and exceedance-frequency maps, all variables of one window in one launch, read in place
// through the strided views the window driver hands over.  HBM-bound streaming: every member value is loaded once and tested
// against all E thresholds of its point.
//   sdy_event_table_accumulate: the ownership of rank_hist.hip.  One group of lanes owns an accumulator row (variable, slot,
//     latitude), keeps the row's E x 2 x (M + 1) bins as 32-bit words in LDS (integer LDS atomics: the bin of a point is known
//     at run time only) and adds them to the float64 accumulators with plain load / add / store once the row is done.
//   sdy_event_frequency_accumulate: the ownership of sdy_member_time_sum.  One thread owns a grid point (four with 16-byte
//     loads) across all samples and times of the window, sums in integer registers and touches the accumulator once.
// No global atomics, no second pass; integers below 2^53 add exactly, so every count has the same bits in any layout, batch or
// run.  The event count is a template argument: the per-thread threshold and counter arrays are indexed at compile time only
// and stay in registers (no private segment).  The arithmetic of a point is events.h.
#include "common.h"
#include "event_count.h"
#include "event_thresholds.h"
#include "events.h"
#include "window.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBlocksPerLaunch = 4096;  // over all variables; a variable with more rows / points strides over them
constexpr int kMinBlocksPerVar = 32;
constexpr int kMaxMembers = SDY_EVENT_MAX_MEMBERS;
constexpr int kLdsBytes = 64 * 1024;    // of a block's rows

long row_words(int E, int M) { return (long)E * 2 * (M + 1); }
long row_bytes_lds(int E, int M) { return row_words(E, M) * 4; }

// G lanes share accumulator row `row` of variable blockIdx.y: row = tt * H + lat, where tt numbers the counted times of the
// window (one row per latitude when the times are pooled).  blockDim.x = rows_per_block * G; the block's rows_per_block rows of
// EC * 2 * (M + 1) words are dynamic LDS (the host keeps them within kLdsBytes).  Each lane takes every G-th unit (4 longitudes
// or 1) of the row's latitude for every sample and every time of the row.  Every thread of a block runs the same number of
// iterations of the row loop (it is over the block's first row), so the barriers are met by all.
// Bounds (entry point): row < n_rows <= T * H <= 2^30; M <= kMaxMembers; a row's points < 2^32 (its LDS words cannot wrap);
// slot < n_slots; flat accumulator indices < 2^50; map planes < n_maps.
template <int W4, int EC>
__global__ __launch_bounds__(kThreads) void event_table_kernel(const sdy_event_args a, int G, unsigned n_rows) {
  extern __shared__ unsigned s_rows[];
  const int v = blockIdx.y;
  const int lig = threadIdx.x & (G - 1), group = threadIdx.x / G, rows_per_block = blockDim.x / G;
  const int units = a.W / W4, M = a.win.n0, n1 = a.win.n1, T = a.win.T, H = a.H, bins = M + 1, words = EC * 2 * bins;
  const bool pool = a.slots.pool_times != 0;
  const unsigned plane = (unsigned)H * (unsigned)a.W;
  const unsigned below = a.thr.below[v], is_map = a.thr.is_map[v];
  const long gs0 = a.win.gs0, gs1 = a.win.gs1, ts1 = a.win.ts1;
  EventRegs<EC> r;
  event_regs<EC>(a.thr, v, is_map, below, r);
  unsigned* mine = s_rows + group * words;      // [e][o][k]
  for (int w = lig; w < words; w += G) mine[w] = 0u;
  for (unsigned base = blockIdx.x * rows_per_block; base < n_rows; base += gridDim.x * rows_per_block) {
    // the row's words are zero: set above, or by the thread that read them behind the previous row
    __syncthreads();
    const unsigned row = base + group;
    const bool active = row < n_rows;
    const unsigned tt = row / (unsigned)H, lat = row - tt * (unsigned)H;
    if (active) {
      const int t_begin = a.slots.t0 + (pool ? 0 : (int)tt), t_end = pool ? T : t_begin + 1;
      for (int u = lig; u < units; u += G) {
        const unsigned in_plane = lat * (unsigned)a.W + (unsigned)(u * W4);             // < plane
        float c[EC][W4];
        thresholds<W4, EC>(a.thr, is_map, r, plane, in_plane, c);
        int valid[W4];                                                     // the points of the unit whose target is not NaN
#pragma unroll
        for (int q = 0; q < W4; ++q) valid[q] = 0;
        for (int s = 0; s < n1; ++s) {
          const float* tg = a.win.target[v] + (long)s * ts1;               // wave-uniform, as is every member's base below
          const float* g = a.win.gen[v] + (long)s * gs1;
          for (int t = t_begin; t < t_end; ++t) {
            const unsigned off_b = ((unsigned)t * plane + in_plane) * 4u;               // < T * plane * 4 <= 2^32
            const Vec<W4> y = ld_u<W4>(tg, off_b);
            int k[EC][W4];
#pragma unroll
            for (int e = 0; e < EC; ++e)
#pragma unroll
              for (int q = 0; q < W4; ++q) k[e][q] = 0;
            count_members<W4, EC>(g, gs0, M, off_b, r, c, k);
            // a point whose target is NaN is counted nowhere
#pragma unroll
            for (int q = 0; q < W4; ++q) {
              if (comp(y, q) == comp(y, q)) {
                ++valid[q];
#pragma unroll
                for (int e = 0; e < EC; ++e) {
                  int o = 0;
                  count_if_above(o, sdy_ev_signed(comp(y, q), r.sign[e]), c[e][q]);
                  atomicAdd(mine + (e * 2 + o) * bins + k[e][q], 1u);                    // k <= M
                }
              }
            }
          }
        }
        // An event whose threshold is NaN at a point counts nothing there.  Every comparison with it was false, so the loop
        // above put the point's valid[q] counts into bin (o = 0, k = 0): this thread takes exactly those out again.  (Tested
        // here, once per unit: as a condition inside the loops above it would be hoisted out of them as EC * W4 lane masks.)
#pragma unroll
        for (int e = 0; e < EC; ++e)
#pragma unroll
          for (int q = 0; q < W4; ++q)
            if (c[e][q] != c[e][q] && valid[q] != 0) atomicSub(mine + e * 2 * bins, (unsigned)valid[q]);
      }
    }
    __syncthreads();
    if (active) {
      // sdy_lead_slot(a.slots, t0 + tt) < n_slots, spelled out: through the helper the compiler allocates the kernels of 6 to 8
      // events two more scalar registers (and one more vector register with 7)
      const long slot = pool ? 0 : (long)a.slots.t_start + a.slots.t0 + (long)tt;
      for (int w = lig; w < words; w += G) {
        const unsigned n = mine[w];
        mine[w] = 0u;
        const int e = w / (2 * bins), ok = w - e * (2 * bins);          // ok = o * (M + 1) + k
        a.acc[sdy_ev_table_at(v, a.slots.n_slots, slot, EC, e, H, lat, M, 0, ok)] += (double)n;
      }
    }
  }
}

// Work item idx of variable blockIdx.y: the W4 grid points at point W4 * idx of the plane, over every sample and counted time
// of the window.  Consecutive lanes touch consecutive addresses of every load and of the accumulators.
// Bounds (entry point): W4 * idx < plane, T * plane <= 2^30; a point's sums <= n0 * n1 * T < 2^31; accumulator indices < 2^50.
template <int W4, int EC>
__global__ __launch_bounds__(kThreads) void event_frequency_kernel(const sdy_event_args a, unsigned n_items) {
  const int v = blockIdx.y;
  const int M = a.win.n0, n1 = a.win.n1, T = a.win.T;
  const unsigned plane = (unsigned)a.H * (unsigned)a.W;
  const unsigned below = a.thr.below[v], is_map = a.thr.is_map[v];
  const long gs0 = a.win.gs0, gs1 = a.win.gs1, ts1 = a.win.ts1;
  EventRegs<EC> r;
  event_regs<EC>(a.thr, v, is_map, below, r);
  for (unsigned idx = blockIdx.x * kThreads + threadIdx.x; idx < n_items; idx += gridDim.x * kThreads) {
    const unsigned p = idx * W4;
    float c[EC][W4];
    thresholds<W4, EC>(a.thr, is_map, r, plane, p, c);
    int hits[EC][W4], obs[EC][W4], valid[W4];
#pragma unroll
    for (int q = 0; q < W4; ++q) valid[q] = 0;
#pragma unroll
    for (int e = 0; e < EC; ++e)
#pragma unroll
      for (int q = 0; q < W4; ++q) hits[e][q] = obs[e][q] = 0;
    for (int s = 0; s < n1; ++s) {
      const float* tg = a.win.target[v] + (long)s * ts1;
      const float* g = a.win.gen[v] + (long)s * gs1;
      for (int t = a.slots.t0; t < T; ++t) {
        const unsigned off_b = ((unsigned)t * plane + p) * 4u;
        const Vec<W4> y = ld_u<W4>(tg, off_b);
        int k[EC][W4];
#pragma unroll
        for (int e = 0; e < EC; ++e)
#pragma unroll
          for (int q = 0; q < W4; ++q) k[e][q] = 0;
        count_members<W4, EC>(g, gs0, M, off_b, r, c, k);
        // a NaN threshold leaves k and o at 0 by itself; a NaN target must drop the members' hits
#pragma unroll
        for (int q = 0; q < W4; ++q) {
          const unsigned seen = sdy_ev_not_nan(comp(y, q));
          valid[q] += (int)seen;
#pragma unroll
          for (int e = 0; e < EC; ++e) {
            hits[e][q] += k[e][q] & -(int)seen;
            count_if_above(obs[e][q], sdy_ev_signed(comp(y, q), r.sign[e]), c[e][q]);
          }
        }
      }
    }
    // the three planes of event e follow one another, the events too: one running pointer
    double* out = a.acc + sdy_ev_freq_at(v, EC, 0, 0, plane, p);
#pragma unroll
    for (int e = 0; e < EC; ++e) {
#pragma unroll
      for (int q = 0; q < W4; ++q) out[q] += (double)hits[e][q];
      out += plane;
#pragma unroll
      for (int q = 0; q < W4; ++q) out[q] += (double)obs[e][q];
      out += plane;
#pragma unroll
      for (int q = 0; q < W4; ++q) out[q] += (double)(valid[q] * (int)sdy_ev_not_nan(c[e][q]));
      out += plane;
    }
  }
}

// everything that bounds an address or a counter, for the device and the host entry points alike
int check(const sdy_event_args* a, bool table) {
  if (!a) return SDY_ERR_ARG;
  if (a->H < 1 || a->W < 1) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, (long)a->H * a->W));
  if (!a->acc || ((uintptr_t)a->acc & 7)) return SDY_ERR_ARG;
  SDY_TRY(sdy_lead_slots_check(&a->slots, a->win.T));
  const long plane = (long)a->H * a->W;                                   // <= 2^30
  SDY_TRY(sdy_event_thresholds_check(&a->thr, a->win.nvars));
  SDY_TRY(sdy_event_thresholds_supported(&a->thr, a->win.nvars, plane));
  if (a->win.n0 > kMaxMembers) return SDY_ERR_UNSUPPORTED;
  const int E = a->thr.n_events, M = a->win.n0;
  if (table) {
    // the 32-bit LDS words of a row: one launch adds at most the row's points to a bin
    const long per_row = (long)a->win.n1 * a->W * (a->slots.pool_times ? (long)a->win.T : 1L);      // < 2^31 * 2^30
    if (per_row >= (1L << 32)) return SDY_ERR_UNSUPPORTED;
    // 64-bit flat accumulator indices: n_slots * H < 2^62, and nvars <= 96 rows of E * 2 * (M + 1) <= 1040 bins stay below 2^57
    const long rows = (long)a->slots.n_slots * a->H;
    if (rows >= (1L << 40) || (long)a->win.nvars * rows * row_words(E, M) >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
    if (row_bytes_lds(E, M) > kLdsBytes) return SDY_ERR_UNSUPPORTED;      // (not reached within the two maxima: 4160 bytes)
  } else {
    // the 32-bit registers of a point: at most n0 * n1 * T member hits
    if ((long)a->win.n0 * a->win.n1 * a->win.T >= (1L << 31)) return SDY_ERR_UNSUPPORTED;
    if ((long)a->win.nvars * E * 3 * plane >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  }
  return SDY_OK;
}

bool vec4(const sdy_event_args* a, long inner) {
  return sdy_window_vec4(&a->win, inner) && (((long)a->H * a->W) & 3) == 0 && sdy_event_thresholds_vec4(&a->thr);
}

template <int W4, int EC>
struct LaunchTable {
  static void go(const sdy_event_args& a, dim3 grid, int threads, size_t lds, hipStream_t stream, int G, unsigned n_rows) {
    hipLaunchKernelGGL((event_table_kernel<W4, EC>), grid, dim3(threads), lds, stream, a, G, n_rows);
  }
};

template <int W4, int EC>
struct LaunchFrequency {
  static void go(const sdy_event_args& a, dim3 grid, hipStream_t stream, unsigned n_items) {
    hipLaunchKernelGGL((event_frequency_kernel<W4, EC>), grid, dim3(kThreads), 0, stream, a, n_items);
  }
};

}  // namespace

extern "C" int sdy_event_table_accumulate_host(const sdy_event_args* a) {
  SDY_TRY(check(a, true));
  const sdy_window& w = a->win;
  const long plane = (long)a->H * a->W;
  const int M = w.n0, E = a->thr.n_events;
  for (int v = 0; v < w.nvars; ++v)
    for (long s = 0; s < w.n1; ++s)
      for (long t = a->slots.t0; t < w.T; ++t)
        for (long lat = 0; lat < a->H; ++lat) {
          const long slot = sdy_lead_slot(a->slots, t);
          const long in_row = t * plane + lat * a->W;
          const float* tg = w.target[v] + s * w.ts1 + in_row;
          const float* g = w.gen[v] + s * w.gs1 + in_row;
          for (long p = 0; p < a->W; ++p)
            for (int e = 0; e < E; ++e) {
              const float c = sdy_event_threshold_host(&a->thr, v, e, plane, lat * a->W + p);
              const bool below = (a->thr.below[v] >> e) & 1u;
              if (!sdy_ev_counted(tg[p], c)) continue;
              int k = 0;
              for (long i0 = 0; i0 < M; ++i0) k += sdy_ev_in(g[i0 * w.gs0 + p], c, below) ? 1 : 0;
              const int o = sdy_ev_in(tg[p], c, below) ? 1 : 0;
              a->acc[sdy_ev_table_at(v, a->slots.n_slots, slot, E, e, a->H, lat, M, o, k)] += 1.0;
            }
        }
  return SDY_OK;
}

extern "C" int sdy_event_table_accumulate(const sdy_event_args* a, void* stream) {
  SDY_TRY(check(a, true));
  if (a->win.T - a->slots.t0 == 0) return SDY_OK;        // a window that holds the initial condition only
  const bool vec = vec4(a, a->W);
  const int G = lane_group(vec ? a->W / 4 : a->W);
  const unsigned n_rows = (unsigned)((a->slots.pool_times ? 1L : (long)(a->win.T - a->slots.t0)) * a->H);      // <= T * H <= 2^30
  // rows of a block: what kThreads lanes cover, capped by the LDS the rows' bins take (at least one: check())
  const long row_bytes = row_bytes_lds(a->thr.n_events, a->win.n0);
  long rows_per_block = kThreads / G;
  if (rows_per_block * row_bytes > kLdsBytes) rows_per_block = kLdsBytes / row_bytes;
  const size_t lds = (size_t)(rows_per_block * row_bytes);
  if (rows_per_block < 1 || lds > (size_t)kLdsBytes) return SDY_ERR_UNSUPPORTED;
  const dim3 grid(sdy_grid_cap((n_rows + rows_per_block - 1) / rows_per_block, a->win.nvars, kBlocksPerLaunch, kMinBlocksPerVar),
                  a->win.nvars);
  dispatch<LaunchTable>(vec, a->thr.n_events, *a, grid, (int)(rows_per_block * G), lds, (hipStream_t)stream, G, n_rows);
  return sdy_launch_status();
}

extern "C" int sdy_event_frequency_accumulate_host(const sdy_event_args* a) {
  SDY_TRY(check(a, false));
  const sdy_window& w = a->win;
  const long plane = (long)a->H * a->W;
  const int M = w.n0, E = a->thr.n_events;
  for (int v = 0; v < w.nvars; ++v)
    for (long s = 0; s < w.n1; ++s)
      for (long t = a->slots.t0; t < w.T; ++t) {
        const float* tg = w.target[v] + s * w.ts1 + t * plane;
        const float* g = w.gen[v] + s * w.gs1 + t * plane;
        for (long p = 0; p < plane; ++p)
          for (int e = 0; e < E; ++e) {
            const float c = sdy_event_threshold_host(&a->thr, v, e, plane, p);
            const bool below = (a->thr.below[v] >> e) & 1u;
            if (!sdy_ev_counted(tg[p], c)) continue;
            int k = 0;
            for (long i0 = 0; i0 < M; ++i0) k += sdy_ev_in(g[i0 * w.gs0 + p], c, below) ? 1 : 0;
            a->acc[sdy_ev_freq_at(v, E, e, 0, plane, p)] += (double)k;
            a->acc[sdy_ev_freq_at(v, E, e, 1, plane, p)] += sdy_ev_in(tg[p], c, below) ? 1.0 : 0.0;
            a->acc[sdy_ev_freq_at(v, E, e, 2, plane, p)] += 1.0;
          }
      }
  return SDY_OK;
}

extern "C" int sdy_event_frequency_accumulate(const sdy_event_args* a, void* stream) {
  SDY_TRY(check(a, false));
  if (a->win.T - a->slots.t0 == 0) return SDY_OK;
  const long plane = (long)a->H * a->W;
  const bool vec = vec4(a, plane);
  const unsigned n_items = (unsigned)(vec ? plane / 4 : plane);                                    // <= 2^30
  const dim3 grid(sdy_grid_cap(((unsigned long)n_items + kThreads - 1) / kThreads, a->win.nvars, kBlocksPerLaunch, kMinBlocksPerVar),
                  a->win.nvars);
  dispatch<LaunchFrequency>(vec, a->thr.n_events, *a, grid, (hipStream_t)stream, n_items);
  return sdy_launch_status();
}

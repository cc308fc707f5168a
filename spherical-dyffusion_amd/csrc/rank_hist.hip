// Rank (Talagrand) histograms of an ensemble per latitude (no counterpart in the reference), gfx950: all variables of one
// window in one launch, read in place through the strided views the window driver hands over.  HBM-bound streaming: every
// input element is read once.  Exactly one group of lanes owns an accumulator row (variable, slot, latitude): it walks every
// sample (and, when the times are pooled, every counted time) of the window that lands in the row, keeps the row's M + 1 bins
// and its tie count as 32-bit words in LDS (integer LDS atomics: the bin of a point is known at run time only), and adds
// them to the float64 accumulators with plain load / add / store once the row is done.  No global atomics, no second pass;
// integers below 2^53 add exactly, so every count has the same bits in any layout, batch or run.  The arithmetic of a grid
// point is rank_hist.h.
#include "common.h"
#include "event_thresholds.h"
#include "rank_hist.h"
#include "window.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBlocksPerLaunch = 4096;  // over all variables; a variable with more rows strides over them
constexpr int kMinBlocksPerVar = 32;
// independent member loads a thread issues before it consumes the first.  By the compiler's report 8 cost 91 VGPRs (5 waves per
// SIMD) and 4 cost 59 (8 waves); at the headline window 8 were 3 % faster (NOTEBOOK.md section 7q): the loads a wave keeps in
// flight count for more than the waves.
constexpr int kMembersInFlight = 8;
constexpr int kMaxMembers = SDY_RANK_HIST_MAX_MEMBERS;
constexpr int kMinGroup = kMinLaneGroup;  // lanes of the narrowest group: at most kThreads / kMinGroup rows per block
constexpr int kRowWords = kMaxMembers + 2;

// G lanes share accumulator row `row` of variable blockIdx.y: row = tt * H + lat, where tt numbers the counted times of the
// window (one row per latitude when the times are pooled).  Each lane takes every G-th unit (4 longitudes or 1) of the
// row's latitude for every sample and every time of the row, holds the unit's targets, and walks the members with
// kMembersInFlight loads in flight; below / equal are running counters per longitude.  Every thread of a block runs the same
// number of iterations of the row loop (it is over the block's first row), so the barriers are met by all.
// Bounds (entry point): row < n_rows <= T * H <= 2^30; M <= kMaxMembers; a row's points < 2^32 (its LDS words cannot wrap);
// slot < n_slots; flat accumulator indices < 2^50.
template <int W4>
__global__ __launch_bounds__(kThreads) void rank_hist_kernel(const sdy_rank_hist_args a, int G, unsigned n_rows) {
  __shared__ unsigned s_rows[(kThreads / kMinGroup) * kRowWords];
  const int v = blockIdx.y;
  const int lig = threadIdx.x & (G - 1), group = threadIdx.x / G, rows_per_block = kThreads / G;
  const int units = a.W / W4, M = a.win.n0, n1 = a.win.n1, T = a.win.T, H = a.H, words = M + 2;
  const bool pool = a.slots.pool_times != 0;
  const unsigned plane = (unsigned)H * (unsigned)a.W;
  const long gs0 = a.win.gs0, gs1 = a.win.gs1, ts1 = a.win.ts1;
  unsigned* mine = s_rows + group * words;      // [0, M]: the bins, [M + 1]: the ties
  for (int k = lig; k < words; k += G) mine[k] = 0u;
  for (unsigned base = blockIdx.x * rows_per_block; base < n_rows; base += gridDim.x * rows_per_block) {
    // the row's words are zero: set above, or by the thread that read them behind the previous row
    __syncthreads();
    const unsigned row = base + group;
    const bool active = row < n_rows;
    const unsigned tt = row / (unsigned)H, lat = row - tt * (unsigned)H;
    if (active) {
      const int t_begin = a.slots.t0 + (pool ? 0 : (int)tt), t_end = pool ? T : t_begin + 1;
      unsigned tied = 0u;
      for (int s = 0; s < n1; ++s) {
        const float* tg = a.win.target[v] + (long)s * ts1;               // wave-uniform, as is every member's base below
        const float* g = a.win.gen[v] + (long)s * gs1;
        for (int t = t_begin; t < t_end; ++t) {
          const unsigned in_row = (unsigned)t * plane + lat * (unsigned)a.W;            // < T * plane <= 2^30
          for (int u = lig; u < units; u += G) {
            const unsigned off_b = (in_row + (unsigned)(u * W4)) * 4u;                  // < 2^32
            const Vec<W4> y = ld_u<W4>(tg, off_b);
            int below[W4], equal[W4];
#pragma unroll
            for (int c = 0; c < W4; ++c) below[c] = equal[c] = 0;
            // the target and the first kMembersInFlight members are requested together and consumed as they arrive; the
            // last batch requests what is left
            int i0 = 0;
            for (; i0 + kMembersInFlight <= M; i0 += kMembersInFlight) {
              Vec<W4> x[kMembersInFlight];
#pragma unroll
              for (int k = 0; k < kMembersInFlight; ++k) x[k] = ld_u<W4>(g + (long)(i0 + k) * gs0, off_b);
#pragma unroll
              for (int k = 0; k < kMembersInFlight; ++k)
#pragma unroll
                for (int c = 0; c < W4; ++c) sdy_rh_member(below[c], equal[c], comp(x[k], c), comp(y, c));
            }
            if (i0 < M) {
              Vec<W4> x[kMembersInFlight - 1];
#pragma unroll
              for (int k = 0; k < kMembersInFlight - 1; ++k)
                if (i0 + k < M) x[k] = ld_u<W4>(g + (long)(i0 + k) * gs0, off_b);
#pragma unroll
              for (int k = 0; k < kMembersInFlight - 1; ++k)
                if (i0 + k < M) {
#pragma unroll
                  for (int c = 0; c < W4; ++c) sdy_rh_member(below[c], equal[c], comp(x[k], c), comp(y, c));
                }
            }
#pragma unroll
            for (int c = 0; c < W4; ++c)
              if (sdy_rh_counted(comp(y, c))) {
                atomicAdd(mine + below[c], 1u);                         // below[c] <= M
                tied += (unsigned)equal[c];
              }
          }
        }
      }
      if (tied) atomicAdd(mine + M + 1, tied);
    }
    __syncthreads();
    if (active) {
      const long r = sdy_rh_row(v, a.slots.n_slots, sdy_lead_slot(a.slots, (long)a.slots.t0 + (long)tt), H, lat);
      double* counts = a.counts + r * (M + 1);
      for (int k = lig; k < words; k += G) {
        const unsigned n = mine[k];
        mine[k] = 0u;
        if (k <= M)
          counts[k] += (double)n;
        else
          a.ties[r] += (double)n;
      }
    }
  }
}

// everything that bounds an address or a counter, for the device and the host entry point alike
int check(const sdy_rank_hist_args* a) {
  if (!a) return SDY_ERR_ARG;
  if (a->H < 1 || a->W < 1) return SDY_ERR_ARG;
  SDY_TRY(sdy_lead_slots_check(&a->slots, a->win.T));
  if (!a->counts || !a->ties || (((uintptr_t)a->counts | (uintptr_t)a->ties) & 7)) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, (long)a->H * a->W));
  if (a->win.n0 > kMaxMembers) return SDY_ERR_UNSUPPORTED;
  // the 32-bit LDS words of a row: one launch adds at most the row's points to a bin
  const long per_row = (long)a->win.n1 * a->W * (a->slots.pool_times ? (long)a->win.T : 1L);      // < 2^31 * 2^30
  if (per_row >= (1L << 32)) return SDY_ERR_UNSUPPORTED;
  // 64-bit flat accumulator indices: n_slots * H < 2^62, and nvars <= 96 rows of M + 1 <= 65 bins stay below 2^53 then
  const long rows = (long)a->slots.n_slots * a->H;
  if (rows >= (1L << 40) || (long)a->win.nvars * rows * (a->win.n0 + 1) >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

}  // namespace

extern "C" int sdy_rank_hist_accumulate_host(const sdy_rank_hist_args* a) {
  SDY_TRY(check(a));
  const sdy_window& w = a->win;
  const long plane = (long)a->H * a->W;
  const int M = w.n0;
  for (int v = 0; v < w.nvars; ++v)
    for (long s = 0; s < w.n1; ++s)
      for (long t = a->slots.t0; t < w.T; ++t)
        for (long lat = 0; lat < a->H; ++lat) {
          const long r = sdy_rh_row(v, a->slots.n_slots, sdy_lead_slot(a->slots, t), a->H, lat);
          const long in_row = t * plane + lat * a->W;
          const float* tg = w.target[v] + s * w.ts1 + in_row;
          const float* g = w.gen[v] + s * w.gs1 + in_row;
          for (long p = 0; p < a->W; ++p) {
            int below = 0, equal = 0;
            for (long i0 = 0; i0 < M; ++i0) sdy_rh_member(below, equal, g[i0 * w.gs0 + p], tg[p]);
            if (sdy_rh_counted(tg[p])) {
              a->counts[r * (M + 1) + below] += 1.0;
              a->ties[r] += (double)equal;
            }
          }
        }
  return SDY_OK;
}

extern "C" int sdy_rank_hist_accumulate(const sdy_rank_hist_args* a, void* stream) {
  SDY_TRY(check(a));
  if (a->win.T - a->slots.t0 == 0) return SDY_OK;        // a window that holds the initial condition only
  const bool vec = sdy_window_vec4(&a->win, a->W);
  const int G = lane_group(vec ? a->W / 4 : a->W);
  const unsigned n_rows = (unsigned)((a->slots.pool_times ? 1L : (long)(a->win.T - a->slots.t0)) * a->H);      // <= T * H <= 2^30
  const unsigned long rows_per_block = kThreads / G;
  const dim3 grid(sdy_grid_cap((n_rows + rows_per_block - 1) / rows_per_block, a->win.nvars, kBlocksPerLaunch, kMinBlocksPerVar),
                  a->win.nvars);
  if (vec)
    hipLaunchKernelGGL(rank_hist_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, *a, G, n_rows);
  else
    hipLaunchKernelGGL(rank_hist_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, *a, G, n_rows);
  return sdy_launch_status();
}

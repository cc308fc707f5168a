// Spell durations of threshold events along every trajectory of a rollout (no counterpart in the reference), gfx950: how long
// an event lasts -- consecutive dry days, warm spells -- all variables of one window in one launch, read in place through the
// strided views the window driver hands over.  HBM-bound streaming: every value of the window is loaded once and tested against
// all E thresholds of its point, the state of a (variable, event, trajectory, grid point) -- four 32-bit words -- is read and
// written once and carries the run across window boundaries.
//   Ownership (rank_hist.hip, event_table_kernel): a block owns an accumulator row (variable, latitude).  Its lanes take the
//   row's work items (trajectory, unit of 4 longitudes or 1); exactly one lane owns a state element.  The row's E x 2 x 16
//   duration bins are 32-bit words in LDS (integer LDS atomics: the bin of a spell is known at run time only) and are added to
//   the float64 accumulator with plain load / add / store once the row is done.
// No global atomics, no second pass; integers below 2^53 add exactly.  The event count and the load width are template
// arguments: the per-thread state and threshold arrays are indexed at compile time only and stay in registers (no private
// segment).  More than kEventsPerPass events of a variable are taken in two passes over the unit's window values (the second
// pass finds them in cache), so that the state of a pass stays within 64 registers.  The arithmetic is spells.h and events.h.
#include "common.h"
#include "event_count.h"
#include "event_thresholds.h"
#include "spells.h"
#include "window.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBlocksPerLaunch = 16384;  // over all variables; a variable with more rows strides over them
constexpr int kMinBlocksPerVar = 32;
constexpr int kMaxMembers = SDY_EVENT_MAX_MEMBERS;
// independent time loads a thread issues before it consumes the first: with more than 4 events (two passes) the second half of 8
// loads would take the scalar registers of its time indices from a kernel that has none to spare
template <int EC>
constexpr int kTimesInFlight = EC > 4 ? 4 : 8;
constexpr int kEventsPerPass = 4;
constexpr int kRowWordsMax = SDY_EVENT_MAX * 2 * SDY_SPELL_BINS;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
template <int W4>
using Words = std::conditional_t<W4 == 4, u32x4, unsigned>;
__device__ __forceinline__ unsigned word_of(unsigned v, int) { return v; }
__device__ __forceinline__ unsigned word_of(u32x4 v, int k) { return v[k]; }
__device__ __forceinline__ void set_word(unsigned& v, int, unsigned x) { v = x; }
__device__ __forceinline__ void set_word(u32x4& v, int k, unsigned x) { v[k] = x; }

// Events e0 .. e0 + EN - 1 of the W4 points at `in_plane` of trajectory r of variable v: thresholds and state loaded once, the
// window's counted times t0 .. T - 1 in ascending order with F loads in flight, the state stored once.  A spell
// that ends adds 1 to bins[(e * 2 + side) * 16 + bin] (LDS).
// Bounds (entry point): in_plane + W4 <= plane, r < rows, e0 + EN <= E <= 8, map planes < n_maps, state indices < 2^50,
// t * plane + in_plane < T * plane <= 2^30.
template <int W4, int EN, int F>
__device__ __forceinline__ void spell_item(const sdy_event_spell_args& a, int v, int E, int e0, unsigned is_map, unsigned below,
                                           long plane, long rows, long r, int side, unsigned in_plane, const float* src,
                                           unsigned* bins) {
  unsigned sign[EN];
  float c[EN][W4];
  // (through a vector register and back, as in event_count.h: the EN bit tests are made here, once per item, as scalar
  // compares; hoisted out of the kernel's loops they would be kept as EN lane masks in pairs of scalar registers)
  unsigned bits = is_map;
  asm volatile("" : "+v"(bits));
  bits = __builtin_amdgcn_readfirstlane(bits);
#pragma unroll
  for (int e = 0; e < EN; ++e) {
    const int ee = e0 + e;
    sign[e] = sdy_ev_sign((below >> ee) & 1u);
    asm volatile("" : "+v"(sign[e]));      // wave-uniform, kept in a vector register on purpose (event_count.h)
    if ((bits >> ee) & 1u) {               // wave-uniform: no divergence
      const Vec<W4> m = ld<W4>(a.thr.maps + ((long)sdy_ev_map_plane(a.thr.map_first[v], is_map, ee) * plane + in_plane));
#pragma unroll
      for (int q = 0; q < W4; ++q) c[e][q] = sdy_ev_signed(comp(m, q), sign[e]);
    } else {
      float s = sdy_ev_signed(a.thr.scalars[v * E + ee], sign[e]);
      asm volatile("" : "+v"(s));
#pragma unroll
      for (int q = 0; q < W4; ++q) c[e][q] = s;
    }
  }
  // the EN x 4 planes of the item's state follow one another at a wave-uniform stride: one running pointer
  const long stride = rows * plane;
  unsigned* const first = a.state + sdy_spell_state_at(v, E, e0, 0, rows, r, plane, in_plane);
  unsigned st[EN][SDY_SPELL_WORDS][W4];
  {
    const unsigned* sp = first;
#pragma unroll
    for (int e = 0; e < EN; ++e)
#pragma unroll
      for (int w = 0; w < SDY_SPELL_WORDS; ++w) {
        const Words<W4> x = *reinterpret_cast<const Words<W4>*>(sp);
        sp += stride;
#pragma unroll
        for (int q = 0; q < W4; ++q) st[e][w][q] = word_of(x, q);
      }
  }
  const int T = a.win.T;
  for (int t = a.t0; t < T; t += F) {
    // a batch past the end of the window re-reads the last time (from cache) and uses nothing of it
    Vec<W4> x[F];
#pragma unroll
    for (int k = 0; k < F; ++k) x[k] = ld<W4>(src + (long)(t + k < T ? t + k : T - 1) * plane);
#pragma unroll
    for (int k = 0; k < F; ++k)
      if (t + k < T) {
#pragma unroll
        for (int e = 0; e < EN; ++e)
#pragma unroll
          for (int q = 0; q < W4; ++q) {
            int in = 0;                      // 1 in the event, else 0 (a NaN on either side compares false)
            count_if_above(in, sdy_ev_signed(comp(x[k], q), sign[e]), c[e][q]);
            const unsigned ended = sdy_spell_step(st[e][SDY_SPELL_RUN][q], st[e][SDY_SPELL_LONGEST][q],
                                                  st[e][SDY_SPELL_SPELLS][q], st[e][SDY_SPELL_HITS][q], (unsigned)in);
            if (ended != 0u) atomicAdd(bins + ((e0 + e) * 2 + side) * SDY_SPELL_BINS + sdy_spell_bin(ended), 1u);
          }
      }
  }
  unsigned* sp = first;
#pragma unroll
  for (int e = 0; e < EN; ++e)
#pragma unroll
    for (int w = 0; w < SDY_SPELL_WORDS; ++w) {
      Words<W4> x;
#pragma unroll
      for (int q = 0; q < W4; ++q) set_word(x, q, st[e][w][q]);
      *reinterpret_cast<Words<W4>*>(sp) = x;
      sp += stride;
    }
}

// Block blockIdx.x of variable blockIdx.y takes the latitudes blockIdx.x, blockIdx.x + gridDim.x, ..: the loop bounds are the
// same for every thread of a block, so every thread meets every barrier.  Work item i of a row: trajectory r = i / units, unit u
// = i % units -- consecutive lanes touch consecutive addresses of every time and of every state plane.
// Bounds (entry point): rows * units + kThreads <= rows * W + kThreads <= 2^32 (i cannot wrap); lat < H; see spell_item.
template <int W4, int EC>
__global__ __launch_bounds__(kThreads) void spell_kernel(const sdy_event_spell_args a) {
  __shared__ unsigned s_bins[kRowWordsMax];
  constexpr int kFirst = EC > kEventsPerPass ? (EC + 1) / 2 : EC, kSecond = EC - kFirst;
  constexpr int words = EC * 2 * SDY_SPELL_BINS;
  const int v = blockIdx.y;
  const int H = a.H, W = a.W, n1 = a.win.n1;
  const unsigned units = (unsigned)(W / W4);
  const long plane = (long)H * W;
  const unsigned gen_rows = (unsigned)a.win.n0 * (unsigned)n1;        // < 2^31
  const unsigned rows = gen_rows + (unsigned)n1;
  const unsigned n_items = rows * units;                              // < 2^32
  const unsigned below = a.thr.below[v], is_map = a.thr.is_map[v];
  for (int w = threadIdx.x; w < words; w += kThreads) s_bins[w] = 0u;
  for (int lat = blockIdx.x; lat < H; lat += gridDim.x) {
    // the row's words are zero: set above, or by the thread that read them behind the previous row
    __syncthreads();
    for (unsigned i = threadIdx.x; i < n_items; i += kThreads) {
      const unsigned r = i / units, u = i - r * units;
      const unsigned in_plane = (unsigned)lat * (unsigned)W + u * W4;   // < plane
      const float* src;
      int side = 0;
      if (r < gen_rows) {
        const unsigned i0 = r / (unsigned)n1, i1 = r - i0 * (unsigned)n1;
        src = a.win.gen[v] + (long)i0 * a.win.gs0 + (long)i1 * a.win.gs1;
      } else {
        src = a.win.target[v] + (long)(r - gen_rows) * a.win.ts1;
        side = 1;
      }
      src += in_plane;
      spell_item<W4, kFirst, kTimesInFlight<EC>>(a, v, EC, 0, is_map, below, plane, (long)rows, (long)r, side, in_plane, src, s_bins);
      if constexpr (kSecond > 0)
        spell_item<W4, kSecond, kTimesInFlight<EC>>(a, v, EC, kFirst, is_map, below, plane, (long)rows, (long)r, side, in_plane, src, s_bins);
    }
    __syncthreads();
    for (int w = threadIdx.x; w < words; w += kThreads) {
      const unsigned n = s_bins[w];
      s_bins[w] = 0u;
      const int es = w / SDY_SPELL_BINS, bin = w - es * SDY_SPELL_BINS;      // es = e * 2 + side
      if (n != 0u) a.durations[sdy_spell_duration_at(v, EC, es >> 1, es & 1, H, lat, bin)] += (double)n;
    }
  }
}

// everything that bounds an address or a counter, for the device and the host entry point alike
int check(const sdy_event_spell_args* a) {
  if (!a || a->struct_size != sizeof(sdy_event_spell_args)) return SDY_ERR_ARG;
  if (a->H < 1 || a->W < 1) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, (long)a->H * a->W));
  if (!a->state || !a->durations || ((uintptr_t)a->state & 7) || ((uintptr_t)a->durations & 7)) return SDY_ERR_ARG;
  if (a->t0 < 0 || a->t0 > a->win.T) return SDY_ERR_ARG;
  const long plane = (long)a->H * a->W;                                   // <= 2^30
  SDY_TRY(sdy_event_thresholds_check(&a->thr, a->win.nvars));
  SDY_TRY(sdy_event_thresholds_supported(&a->thr, a->win.nvars, plane));
  if (a->win.n0 > kMaxMembers) return SDY_ERR_UNSUPPORTED;
  // the 32-bit LDS words of a row and its 32-bit work items: one launch ends at most rows * W * T spells in a row
  const long rows = sdy_spell_rows(a->win.n0, a->win.n1);                 // <= 65 * 2^31
  // (a lane's item number goes up by kThreads until it leaves the row's items: room for one step past them)
  if (rows >= (1L << 32) || rows * a->W + kThreads > (1L << 32) || rows * a->W * a->win.T >= (1L << 32)) return SDY_ERR_UNSUPPORTED;
  // 64-bit flat indices: rows * plane < 2^62, nvars * E * 4 <= 3072 < 2^12
  const long E = a->thr.n_events;
  if (rows * plane >= (1L << 50) || (long)a->win.nvars * E * SDY_SPELL_WORDS * rows * plane >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  if ((long)a->win.nvars * E * 2 * a->H * SDY_SPELL_BINS >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

bool vec4(const sdy_event_spell_args* a) {
  return sdy_window_vec4(&a->win, a->W) && (((long)a->H * a->W) & 3) == 0 && sdy_event_thresholds_vec4(&a->thr) &&
         ((uintptr_t)a->state & 15) == 0;
}

template <int W4, int EC>
struct Launch {
  static void go(const sdy_event_spell_args& a, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((spell_kernel<W4, EC>), grid, dim3(kThreads), 0, stream, a);
  }
};

}  // namespace

extern "C" int sdy_event_spell_accumulate_host(const sdy_event_spell_args* a) {
  SDY_TRY(check(a));
  const sdy_window& w = a->win;
  const long plane = (long)a->H * a->W, rows = sdy_spell_rows(w.n0, w.n1), gen_rows = (long)w.n0 * w.n1;
  const int E = a->thr.n_events;
  for (int v = 0; v < w.nvars; ++v)
    for (int e = 0; e < E; ++e) {
      const bool below = (a->thr.below[v] >> e) & 1u;
      for (long r = 0; r < rows; ++r) {
        const int side = r < gen_rows ? 0 : 1;
        const float* src = side == 0 ? w.gen[v] + (r / w.n1) * w.gs0 + (r % w.n1) * w.gs1 : w.target[v] + (r - gen_rows) * w.ts1;
        for (long p = 0; p < plane; ++p) {
          const float c = sdy_event_threshold_host(&a->thr, v, e, plane, p);
          unsigned* st[SDY_SPELL_WORDS];
          for (int k = 0; k < SDY_SPELL_WORDS; ++k) st[k] = a->state + sdy_spell_state_at(v, E, e, k, rows, r, plane, p);
          for (long t = a->t0; t < w.T; ++t) {
            const unsigned ended = sdy_spell_step(*st[SDY_SPELL_RUN], *st[SDY_SPELL_LONGEST], *st[SDY_SPELL_SPELLS],
                                                  *st[SDY_SPELL_HITS], sdy_ev_in(src[t * plane + p], c, below) ? 1u : 0u);
            if (ended != 0u) a->durations[sdy_spell_duration_at(v, E, e, side, a->H, p / a->W, sdy_spell_bin(ended))] += 1.0;
          }
        }
      }
    }
  return SDY_OK;
}

extern "C" int sdy_event_spell_accumulate(const sdy_event_spell_args* a, void* stream) {
  SDY_TRY(check(a));
  if (a->win.T - a->t0 == 0) return SDY_OK;        // a window that holds the initial condition only
  const dim3 grid(sdy_grid_cap((unsigned long)a->H, a->win.nvars, kBlocksPerLaunch, kMinBlocksPerVar), a->win.nvars);
  dispatch<Launch>(vec4(a), a->thr.n_events, *a, grid, (hipStream_t)stream);
  return sdy_launch_status();
}

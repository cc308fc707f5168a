// Neighbourhood verification of threshold events (fractions skill score; no counterpart in the reference), gfx950: per
// variable, slot, event, radius and latitude the six integer sums over the counted centres of a row (count, K, O, K^2, K O,
// O^2 of the box sums of the members in the event, the truth in the event and the counted points).  Two launches, because a
// halo of r rows of M + 1 fp32 planes must not be re-read from HBM:
//   fss_encode_kernel: HBM-bound streaming, the traversal of event_frequency_kernel (event_verif.hip).  Every member value is
//     loaded once, in place, and tested against all E thresholds of its point; one 16-bit code (k, o, c) per (variable, sample,
//     time, event, point) goes to the workspace: 2 bytes written per 4 (M + 1) bytes read.
//   fss_sum_kernel: a block owns the accumulator rows of one (variable, slot, event) and one band of B latitudes.  Per radius,
//     sample and counted time it reads the codes of the band's rows and r halo rows (from L2: they were just written), forms
//     the horizontal periodic sums in LDS, then the vertical clipped sums, and adds the six terms of every counted centre to
//     64-bit integer sums; each row sum is added to the float64 accumulator once, with a plain load / add / store.
// No global atomics; no index comes from a value read from memory.  The sums are integers: the same bits in any layout, batch,
// band size, grouping of variables and run, and the _host twin's.  The event count is a template argument of the first kernel
// (event_count.h): nothing lands in scratch.  The arithmetic of a point and of a centre is events.h and fss.h.
#include "common.h"
#include "event_count.h"
#include "event_thresholds.h"
#include "events.h"
#include "fss.h"
#include "window.h"

#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr int kBlocksPerLaunch = 4096;  // of the first kernel, over all variables; a variable with more points strides over them
constexpr int kMinBlocksPerVar = 32;
constexpr long kMaxSumItems = (1L << 24) - 1;        // blocks of the second kernel per (variable, event): its grid's x extent
constexpr int kMaxBand = 16;            // latitudes of a block, a power of two (kThreads / band threads share a row)
constexpr int kChunkWords = 2048;       // spread codes a block stages per pass, in whole rows (at least one)
constexpr int kStage = kChunkWords / kThreads;       // codes a thread loads before it stores the first
constexpr int kLdsBytes = 64 * 1024;

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

template <int W4>
__device__ __forceinline__ void store_codes(unsigned short* at, const unsigned (&code)[W4]);
template <>
__device__ __forceinline__ void store_codes<4>(unsigned short* at, const unsigned (&code)[4]) {
  *reinterpret_cast<u32x2*>(at) = u32x2{code[0] | (code[1] << 16), code[2] | (code[3] << 16)};
}
template <>
__device__ __forceinline__ void store_codes<1>(unsigned short* at, const unsigned (&code)[1]) { *at = (unsigned short)code[0]; }

// Work item idx of variable blockIdx.y: the W4 grid points at point W4 * idx of the plane, every sample and counted time of
// the window.  Consecutive lanes touch consecutive addresses of every load and store.
// Bounds (entry point): W4 * idx < plane, T * plane <= 2^30; k <= M <= 64 (7 bits); code indices < 2^50, inside ws_bytes; with
// W4 = 4 the plane is a multiple of 4 and ws 8-byte aligned, so every 8-byte store is aligned.
template <int W4, int EC>
__global__ __launch_bounds__(kThreads) void fss_encode_kernel(const sdy_fss_args a, unsigned n_items) {
  const int v = blockIdx.y;
  const int M = a.win.n0, n1 = a.win.n1, T = a.win.T;
  const unsigned plane = (unsigned)a.H * (unsigned)a.W;
  const unsigned below = a.thr.below[v], is_map = a.thr.is_map[v];
  const long gs0 = a.win.gs0, gs1 = a.win.gs1, ts1 = a.win.ts1;
  unsigned short* codes = static_cast<unsigned short*>(a.ws);
  EventRegs<EC> r;
  event_regs<EC>(a.thr, v, is_map, below, r);
  for (unsigned idx = blockIdx.x * kThreads + threadIdx.x; idx < n_items; idx += gridDim.x * kThreads) {
    const unsigned p = idx * W4;
    float c[EC][W4];
    thresholds<W4, EC>(a.thr, is_map, r, plane, p, c);
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
        // the EC planes of codes of (v, s, t) follow one another: one running pointer
        unsigned short* out = codes + (sdy_fss_code_at(v, n1, s, T, t, EC, 0, plane) + p);
#pragma unroll
        for (int e = 0; e < EC; ++e) {
          unsigned code[W4];
#pragma unroll
          for (int q = 0; q < W4; ++q) {
            int o = 0;
            count_if_above(o, sdy_ev_signed(comp(y, q), r.sign[e]), c[e][q]);
            // (counted, without a comparison: as lane masks the EC * W4 tests of the thresholds would be hoisted out of the loops)
            const unsigned counted = sdy_ev_not_nan(comp(y, q)) & sdy_ev_not_nan(c[e][q]);
            code[q] = sdy_fss_code((unsigned)k[e][q], (unsigned)o, counted);
          }
          store_codes<W4>(out, code);
          out += plane;
        }
      }
    }
  }
}

// What the host fixes for the second kernel: the band of a block, the rows it stages per pass and its LDS
struct SumPlan {
  int band = 0, chunk_rows = 0, n_bands = 0;
  size_t lds = 0;
};

// LDS of a block: the band's row sums, (band + 2 r_max) rows of W horizontal sums and chunk_rows padded rows of spread codes
size_t sum_lds_bytes(int band, int chunk_rows, int W, int r_max) {
  return (size_t)band * SDY_FSS_TERMS * 8 + ((size_t)(band + 2 * r_max) * W + (size_t)chunk_rows * (W + 2 * r_max)) * 4;
}

// The widest band (a power of two, at most kMaxBand, no wider than the grid needs) whose rows fit; false when not even one
// latitude does
bool plan_sum(int H, int W, int r_max, SumPlan* plan) {
  int band = kMaxBand;
  while (band > 1 && band / 2 >= H) band >>= 1;
  while (band >= 1 && sum_lds_bytes(band, 1, W, r_max) > (size_t)kLdsBytes) band >>= 1;
  if (band < 1) return false;
  int chunk_rows = kChunkWords / (W + 2 * r_max);
  if (chunk_rows > band + 2 * r_max) chunk_rows = band + 2 * r_max;
  if (chunk_rows < 1) chunk_rows = 1;
  while (chunk_rows > 1 && sum_lds_bytes(band, chunk_rows, W, r_max) > (size_t)kLdsBytes) --chunk_rows;
  plan->band = band;
  plan->chunk_rows = chunk_rows;
  plan->n_bands = (H + band - 1) / band;
  plan->lds = sum_lds_bytes(band, chunk_rows, W, r_max);
  return true;
}

// radii[j] of the by-value arguments without a run-time index into them (which would copy the array to private memory)
__device__ __forceinline__ int radius(const sdy_fss_args& a, int j) {
  static_assert(SDY_FSS_MAX_RADII == 4, "one operand per radius");
  return j == 0 ? a.radii[0] : j == 1 ? a.radii[1] : j == 2 ? a.radii[2] : a.radii[3];
}

// Block blockIdx.x of variable blockIdx.y and event blockIdx.z: band (blockIdx.x % n_bands) of counted time tt = blockIdx.x /
// n_bands (one block per work item: what a block needs once dies before its loops).  The block's kThreads / band
// threads per latitude take every (kThreads / band)-th longitude of their latitude's centres.  Per radius: the six sums of a
// thread stay in registers over all samples and times, meet in the band's 64-bit LDS words (integer LDS atomics, once per
// radius) and go to the accumulator from there.  Every thread of a block runs the same loops around the barriers.
// Bounds (entry point): band * 6 <= kThreads; LDS as sum_lds_bytes(); rows first .. last - 1 of a pass lie in 0 .. H - 1, so code
// indices stay inside the plane of (v, s, t, e); a staged row has W + 2 r <= W + 2 r_max words; the horizontal sums of a pass go
// to rows < band + 2 r; box sums: M (2 r_max + 1)^2 <= 65535; a row sum < 2^53; slot < n_slots; flat accumulator indices < 2^50.
__global__ __launch_bounds__(kThreads) void fss_sum_kernel(const sdy_fss_args a, int band, int chunk_rows, unsigned n_bands) {
  extern __shared__ unsigned long long s_fss[];
  const int H = a.H, W = a.W, E = a.thr.n_events, R = a.n_radii, n1 = a.win.n1, T = a.win.T;
  const int r_max = radius(a, R - 1), v = blockIdx.y, e = blockIdx.z;
  unsigned long long* s_sum = s_fss;                                          // [band][6]
  unsigned* s_hs = reinterpret_cast<unsigned*>(s_sum + band * SDY_FSS_TERMS);  // [band + 2 r_max][W]
  unsigned* s_pk = s_hs + (band + 2 * r_max) * W;                              // [chunk_rows][W + 2 r]
  const unsigned short* codes = static_cast<const unsigned short*>(a.ws);
  const long plane = (long)H * W;
  const bool pool = a.slots.pool_times != 0;
  const int tid = threadIdx.x, per_row = kThreads / band, my_row = tid / per_row, lir = tid - my_row * per_row;
  // point tid of a pass as (row, lon), and the step to point tid + kThreads: no division inside the loops
  const int row0 = tid / W, lon0 = tid - row0 * W;
  int row_step = kThreads / W, lon_step = kThreads - row_step * W, lon_stride = per_row;
  // (block-uniform, but only ever added to a thread's own numbers: in vector registers they leave the scalar ones to the loops)
  asm volatile("" : "+v"(row_step), "+v"(lon_step), "+v"(lon_stride));
  const int tt = (int)(blockIdx.x / n_bands), b = (int)(blockIdx.x - (unsigned)tt * n_bands);
  const int lat0 = b * band, lat = lat0 + my_row;
  const int t_begin = a.slots.t0 + (pool ? 0 : tt), t_end = pool ? T : t_begin + 1;
  const long slot = sdy_lead_slot(a.slots, t_begin);                        // < n_slots
  // the band's first accumulator row of radius 0 (in vector registers: it is not looked at before the sums are done)
  double* out0 = a.acc + sdy_fss_at(v, a.slots.n_slots, slot, E, e, R, 0, H, lat0);
  asm volatile("" : "+v"(out0));
  for (int j = 0; j < R; ++j) {
    const int r = radius(a, j), padded = W + 2 * r;
    // the rows whose horizontal sums the band's centres need, clipped at the poles
    const int first = sdy_fss_row_first(lat0, r), last = sdy_fss_row_last(H, lat0 + band - 1, r) + 1;
    if (tid < band * SDY_FSS_TERMS) s_sum[tid] = 0ull;                      // (read again behind the barriers below)
    unsigned long long sum[SDY_FSS_TERMS];
#pragma unroll
    for (int q = 0; q < SDY_FSS_TERMS; ++q) sum[q] = 0ull;
    for (int s = 0; s < n1; ++s)
      for (int t = t_begin; t < t_end; ++t) {
        const unsigned short* src = codes + sdy_fss_code_at(v, n1, s, T, t, E, e, plane);
        for (int c0 = first; c0 < last; c0 += chunk_rows) {
          const int n = ((c0 + chunk_rows < last ? c0 + chunk_rows : last) - c0) * W;
          // the staged rows of the previous pass are read; before the first pass: so are the sums of the previous time
          __syncthreads();
          // a row as [lon W - r .. W - 1 | lon 0 .. W - 1 | lon 0 .. r - 1]: a centre's segment is 2r + 1 consecutive words
          // (kStage loads in flight per thread: one at a time each would wait out the way to the codes and back)
          for (int i0 = tid, row = row0, lon = lon0; i0 < n; i0 += kStage * kThreads) {
            unsigned code[kStage];
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
              // (past the end: the last code again, not stored -- a predicated load would keep kStage lane masks alive)
              const int i = i0 + u * kThreads;
              code[u] = src[(long)c0 * W + (i < n - 1 ? i : n - 1)];
            }
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
              if (i0 + u * kThreads < n) {
                const unsigned w = sdy_fss_spread(code[u]);
                unsigned* at = s_pk + row * padded + r + lon;
                at[0] = w;
                if (lon < r) at[W] = w;
                if (lon >= W - r) at[-W] = w;
              }
              row += row_step, lon += lon_step;
              if (lon >= W) ++row, lon -= W;
            }
          }
          __syncthreads();
          for (int i = tid, row = row0, lon = lon0; i < n; i += kThreads) {
            const unsigned* at = s_pk + row * padded + lon;
            unsigned hs = 0;
            for (int d = 0; d <= 2 * r; ++d) hs += at[d];
            s_hs[(c0 - first) * W + i] = hs;
            row += row_step, lon += lon_step;
            if (lon >= W) ++row, lon -= W;
          }
        }
        __syncthreads();
        if (lat < H) {
          const int lo = sdy_fss_row_first(lat, r) - first, hi = sdy_fss_row_last(H, lat, r) - first;
          const unsigned n = sdy_fss_size(H, lat, r);
          for (int lon = lir; lon < W; lon += lon_stride) {
            unsigned K = 0, O = 0, C = 0;
            for (int row = lo; row <= hi; ++row) {
              const unsigned w = s_hs[row * W + lon];
              K += sdy_fss_spread_k(w);
              O += sdy_fss_spread_o(w);
              C += sdy_fss_spread_c(w);
            }
            sdy_fss_add_centre(sum, K, O, C, n);
          }
        }
      }
    if (lat < H) {
#pragma unroll
      for (int q = 0; q < SDY_FSS_TERMS; ++q) atomicAdd(s_sum + my_row * SDY_FSS_TERMS + q, sum[q]);
    }
    __syncthreads();
    if (tid < band * SDY_FSS_TERMS) {
      const int row = tid / SDY_FSS_TERMS, q = tid - row * SDY_FSS_TERMS;
      if (lat0 + row < H) out0[((long)j * H + row) * SDY_FSS_TERMS + q] += (double)s_sum[tid];
    }
    __syncthreads();                                                        // before the words are cleared for the next radius
  }
}

long code_count(long nvars, long E, long n1, long T, long plane) { return nvars * n1 * T * E * plane; }   // callers bound it

// everything that bounds an address or a counter, for the device and the host entry points alike; the host twin needs no
// workspace (a NULL one is not looked at)
int check(const sdy_fss_args* a, bool device, SumPlan* plan) {
  if (!a) return SDY_ERR_ARG;
  if (a->H < 1 || a->W < 1) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, (long)a->H * a->W));
  if (!a->acc || ((uintptr_t)a->acc & 7)) return SDY_ERR_ARG;
  SDY_TRY(sdy_lead_slots_check(&a->slots, a->win.T));
  if (a->n_radii < 1 || a->n_radii > SDY_FSS_MAX_RADII) return SDY_ERR_ARG;
  for (int j = 0; j < a->n_radii; ++j) {
    if (a->radii[j] < 0 || (j > 0 && a->radii[j] <= a->radii[j - 1])) return SDY_ERR_ARG;
    if (2L * a->radii[j] + 1 > (long)a->W) return SDY_ERR_ARG;
  }
  const long plane = (long)a->H * a->W;                                   // <= 2^30
  SDY_TRY(sdy_event_thresholds_check(&a->thr, a->win.nvars));
  const int E = a->thr.n_events, M = a->win.n0, R = a->n_radii;
  if (device || a->ws) {
    // (a workspace whose codes pass 2^50 has no size: sdy_fss_workspace_bytes is 0, and the call is refused below)
    if (!a->ws || ((uintptr_t)a->ws & 7)) return SDY_ERR_ARG;
    if (a->ws_bytes < sdy_fss_workspace_bytes(a->win.nvars, E, a->win.n1, a->win.T, a->H, a->W)) return SDY_ERR_ARG;
  }
  if (M > SDY_EVENT_MAX_MEMBERS) return SDY_ERR_UNSUPPORTED;
  const long r_max = a->radii[R - 1], side = 2 * r_max + 1;               // side <= W < 2^31
  if (side > 255 || (long)M * side * side > 65535) return SDY_ERR_UNSUPPORTED;        // (255: no side above it can pass)
  SDY_TRY(sdy_event_thresholds_supported(&a->thr, a->win.nvars, plane));
  // the 64-bit row sums and one call's float64 additions: the largest term, (M n_max)^2 < 2^32, times the centres of a row,
  // n1 * W * T < 2^61
  const long n_max = side * (a->H < side ? a->H : side), term = (M * n_max) * (M * n_max);
  const long centres = (long)a->win.n1 * a->W * (a->slots.pool_times ? (long)(a->win.T - a->slots.t0) : 1L);
  if (centres > ((1L << 53) - 1) / term) return SDY_ERR_UNSUPPORTED;
  const long rows = (long)a->slots.n_slots * a->H;
  if (rows >= (1L << 40) || (long)a->win.nvars * rows * E * R * SDY_FSS_TERMS >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  if ((double)a->win.nvars * E * a->win.n1 * a->win.T * plane >= 0x1p50) return SDY_ERR_UNSUPPORTED;     // the codes
  SumPlan mine;
  if (!plan_sum(a->H, a->W, (int)r_max, &mine)) return SDY_ERR_UNSUPPORTED;
  if ((a->slots.pool_times ? 1L : (long)(a->win.T - a->slots.t0)) * mine.n_bands > kMaxSumItems) return SDY_ERR_UNSUPPORTED;
  if (plan) *plan = mine;
  return SDY_OK;
}

bool vec4(const sdy_fss_args* a) {
  const long plane = (long)a->H * a->W;
  return sdy_window_vec4(&a->win, plane) && sdy_event_thresholds_vec4(&a->thr);
}

template <int W4, int EC>
struct LaunchEncode {
  static void go(const sdy_fss_args& a, dim3 grid, hipStream_t stream, unsigned n_items) {
    hipLaunchKernelGGL((fss_encode_kernel<W4, EC>), grid, dim3(kThreads), 0, stream, a, n_items);
  }
};

int launch_encode(const sdy_fss_args* a, hipStream_t stream) {
  const long plane = (long)a->H * a->W;
  const bool vec = vec4(a);
  const unsigned n_items = (unsigned)(vec ? plane / 4 : plane);                                     // <= 2^30
  const dim3 grid(sdy_grid_cap(((unsigned long)n_items + kThreads - 1) / kThreads, a->win.nvars, kBlocksPerLaunch, kMinBlocksPerVar),
                  a->win.nvars);
  dispatch<LaunchEncode>(vec, a->thr.n_events, *a, grid, stream, n_items);
  return sdy_launch_status();
}

int launch_sum(const sdy_fss_args* a, const SumPlan& plan, hipStream_t stream) {
  const unsigned n_tt = a->slots.pool_times ? 1u : (unsigned)(a->win.T - a->slots.t0);
  const dim3 grid(n_tt * (unsigned)plan.n_bands, a->win.nvars, a->thr.n_events);  // x <= kMaxSumItems: check()
  hipLaunchKernelGGL(fss_sum_kernel, grid, dim3(kThreads), plan.lds, stream, *a, plan.band, plan.chunk_rows, (unsigned)plan.n_bands);
  return sdy_launch_status();
}

}  // namespace

extern "C" size_t sdy_fss_workspace_bytes(int nvars, int n_events, int n1, int T, int H, int W) {
  if (nvars < 1 || nvars > SDY_MAX_VARS || n_events < 1 || n_events > SDY_EVENT_MAX || n1 < 1 || T < 1 || H < 1 || W < 1) return 0;
  const long plane = (long)H * W;
  if ((long)T * plane > (1L << 30)) return 0;
  if ((double)nvars * n_events * n1 * T * plane >= 0x1p50) return 0;
  return ((size_t)code_count(nvars, n_events, n1, T, plane) * 2 + 7) & ~(size_t)7;
}

extern "C" int sdy_fss_accumulate_host(const sdy_fss_args* a) {
  SDY_TRY(check(a, false, nullptr));
  const sdy_window& w = a->win;
  const int H = a->H, W = a->W, M = w.n0, E = a->thr.n_events, R = a->n_radii;
  const long plane = (long)H * W;
  std::vector<unsigned> k(plane), o(plane), c(plane), hk(plane), ho(plane), hc(plane);
  for (int v = 0; v < w.nvars; ++v)
    for (long s = 0; s < w.n1; ++s)
      for (long t = a->slots.t0; t < w.T; ++t)
        for (int e = 0; e < E; ++e) {
          const long slot = sdy_lead_slot(a->slots, t);
          const float* tg = w.target[v] + s * w.ts1 + t * plane;
          const float* g = w.gen[v] + s * w.gs1 + t * plane;
          const bool below = (a->thr.below[v] >> e) & 1u;
          for (long p = 0; p < plane; ++p) {
            const float thr = sdy_event_threshold_host(&a->thr, v, e, plane, p);
            unsigned members = 0;
            for (long i0 = 0; i0 < M; ++i0) members += sdy_ev_in(g[i0 * w.gs0 + p], thr, below) ? 1u : 0u;
            const unsigned code = sdy_fss_code(members, sdy_ev_in(tg[p], thr, below) ? 1u : 0u, sdy_ev_counted(tg[p], thr) ? 1u : 0u);
            k[p] = sdy_fss_code_k(code);
            o[p] = sdy_fss_code_o(code);
            c[p] = sdy_fss_code_c(code);
          }
          for (int j = 0; j < R; ++j) {
            const int r = a->radii[j];
            for (int lat = 0; lat < H; ++lat)
              for (int lon = 0; lon < W; ++lon) {
                unsigned sk = 0, so = 0, sc = 0;
                for (int d = -r; d <= r; ++d) {
                  const long p = (long)lat * W + sdy_fss_wrap(lon + d, W);
                  sk += k[p], so += o[p], sc += c[p];
                }
                hk[(long)lat * W + lon] = sk, ho[(long)lat * W + lon] = so, hc[(long)lat * W + lon] = sc;
              }
            for (int lat = 0; lat < H; ++lat) {
              unsigned long long sum[SDY_FSS_TERMS] = {0, 0, 0, 0, 0, 0};
              const unsigned n = sdy_fss_size(H, lat, r);
              for (int lon = 0; lon < W; ++lon) {
                unsigned K = 0, O = 0, C = 0;
                for (int row = sdy_fss_row_first(lat, r); row <= sdy_fss_row_last(H, lat, r); ++row)
                  K += hk[(long)row * W + lon], O += ho[(long)row * W + lon], C += hc[(long)row * W + lon];
                sdy_fss_add_centre(sum, K, O, C, n);
              }
              double* out = a->acc + sdy_fss_at(v, a->slots.n_slots, slot, E, e, R, j, H, lat);
              for (int q = 0; q < SDY_FSS_TERMS; ++q) out[q] += (double)sum[q];
            }
          }
        }
  return SDY_OK;
}

extern "C" int sdy_fss_encode(const sdy_fss_args* a, void* stream) {
  SDY_TRY(check(a, true, nullptr));
  if (a->win.T - a->slots.t0 == 0) return SDY_OK;        // a window that holds the initial condition only
  return launch_encode(a, (hipStream_t)stream);
}

extern "C" int sdy_fss_sum(const sdy_fss_args* a, void* stream) {
  SumPlan plan;
  SDY_TRY(check(a, true, &plan));
  if (a->win.T - a->slots.t0 == 0) return SDY_OK;
  return launch_sum(a, plan, (hipStream_t)stream);
}

extern "C" int sdy_fss_accumulate(const sdy_fss_args* a, void* stream) {
  SumPlan plan;
  SDY_TRY(check(a, true, &plan));
  if (a->win.T - a->slots.t0 == 0) return SDY_OK;
  SDY_TRY(launch_encode(a, (hipStream_t)stream));
  return launch_sum(a, plan, (hipStream_t)stream);
}

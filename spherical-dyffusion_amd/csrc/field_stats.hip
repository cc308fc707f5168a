// Per-grid-point video statistics and zonal means of the inference aggregators, gfx950: all variables of one window in one
// launch, read in place through the strided views the window driver hands over, folded into float64 accumulators that stay on
// the device.  HBM-bound streaming: every input element is read once; exactly one thread owns an accumulator element, so
// there are no atomics and no LDS.  The arithmetic of a grid point is field_stats.h.
#include "common.h"
#include "field_stats.h"
#include "window.h"

namespace {

constexpr int kBlocksPerLaunch = 4096;  // over all variables; a variable with more work strides over its items
constexpr int kMinBlocksPerVar = 32;
constexpr int kRowsInFlight = 4;        // independent row loads a thread issues before it consumes the first

// Work item idx of variable blockIdx.y: W grid points (4 or 1) at point W * q of window time t, idx = t * (HW / W) + q, so
// consecutive lanes touch consecutive addresses of every row and of the accumulators.  idx < T * HW <= 2^30 (entry point).
template <int W, bool EXT>
__global__ __launch_bounds__(256) void video_kernel(const sdy_video_args a, unsigned n_items) {
  const int v = blockIdx.y;
  const unsigned per_time = (unsigned)(a.HW / W);
  const long HW = a.HW, gs0 = a.win.gs0, gs1 = a.win.gs1, ts1 = a.win.ts1;
  const int n0 = a.win.n0, n1 = a.win.n1;
  for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < n_items; idx += gridDim.x * 256u) {
    const unsigned t = idx / per_time, q = idx - t * per_time;
    const long in_row = (long)t * HW + (long)q * W;          // < T * HW
    const float* g = a.win.gen[v] + in_row;
    const float* tg = a.win.target[v] + in_row;
    sdy_fs_point<EXT> st[W];
#pragma unroll
    for (int c = 0; c < W; ++c) sdy_fs_init(st[c]);
    auto add_target = [&](Vec<W> tv) {
#pragma unroll
      for (int c = 0; c < W; ++c) sdy_fs_add_target(st[c], comp(tv, c));
    };
    auto add_gen = [&](Vec<W> gv, Vec<W> tv) {
#pragma unroll
      for (int c = 0; c < W; ++c) sdy_fs_add_gen(st[c], comp(gv, c), comp(tv, c));
    };
    if (n0 == 1) {   // flat rows: kRowsInFlight samples' generated and target rows at once
      int i1 = 0;
      for (; i1 + kRowsInFlight <= n1; i1 += kRowsInFlight) {
        Vec<W> gr[kRowsInFlight], tr[kRowsInFlight];
#pragma unroll
        for (int k = 0; k < kRowsInFlight; ++k) {
          gr[k] = ld<W>(g + (long)(i1 + k) * gs1);
          tr[k] = ld<W>(tg + (long)(i1 + k) * ts1);
        }
#pragma unroll
        for (int k = 0; k < kRowsInFlight; ++k) {
          add_target(tr[k]);
          add_gen(gr[k], tr[k]);
        }
      }
      for (; i1 < n1; ++i1) {
        const Vec<W> tv = ld<W>(tg + (long)i1 * ts1);
        add_target(tv);
        add_gen(ld<W>(g + (long)i1 * gs1), tv);
      }
    } else {         // member-stacked: a sample's target row once, its members' rows kRowsInFlight at a time
      for (int i1 = 0; i1 < n1; ++i1) {
        const Vec<W> tv = ld<W>(tg + (long)i1 * ts1);
        add_target(tv);
        const float* gm = g + (long)i1 * gs1;
        int i0 = 0;
        for (; i0 + kRowsInFlight <= n0; i0 += kRowsInFlight) {
          Vec<W> gr[kRowsInFlight];
#pragma unroll
          for (int k = 0; k < kRowsInFlight; ++k) gr[k] = ld<W>(gm + (long)(i0 + k) * gs0);
#pragma unroll
          for (int k = 0; k < kRowsInFlight; ++k) add_gen(gr[k], tv);
        }
        for (; i0 < n0; ++i0) add_gen(ld<W>(gm + (long)i0 * gs0), tv);
      }
    }
    // accumulator element: variable v, time t_start + t < n_timesteps (entry point), grid point W * q + c < HW
    const long at = ((long)v * a.n_timesteps + (a.t_start + (long)t)) * HW + (long)q * W;
#pragma unroll
    for (int c = 0; c < W; ++c)
      sdy_fs_store(st[c], at + c, n0 * n1, n1, a.gen_mean, a.target_mean, a.gen_sq, a.target_sq, a.err_var, a.err_min,
                   a.err_max);
  }
}

// G lanes (a power of two, <= 64) share one latitude row (sample s, window time t, latitude lat) of variable blockIdx.y: each
// takes every G-th unit (4 longitudes or 1) of the row of every member, the group's float64 partial sums meet in a butterfly
// of cross-lane moves, and lane 0 of the group owns the two accumulator elements.  Every lane of a block runs the same number
// of iterations (the loop is over the block's first row), so the butterfly never reads an idle lane.
template <int W4>
__global__ __launch_bounds__(256) void zonal_kernel(const sdy_zonal_args a, int G, unsigned long n_rows) {
  const int v = blockIdx.y;
  const int lig = threadIdx.x & (G - 1), group = threadIdx.x / G, rows_per_block = 256 / G;
  const int units = a.W / W4, n0 = a.win.n0;
  const unsigned long TH = (unsigned long)a.win.T * a.H;
  const long gs0 = a.win.gs0;
  for (unsigned long base = (unsigned long)blockIdx.x * rows_per_block; base < n_rows;
       base += (unsigned long)gridDim.x * rows_per_block) {
    const unsigned long row = base + group;
    const bool active = row < n_rows;
    double gsum = 0.0, tsum = 0.0;
    unsigned long s = 0, rem = 0;
    if (active) {
      s = row / TH;                       // < n1
      rem = row - s * TH;                 // t * H + lat < T * H
      const float* g = a.win.gen[v] + (long)s * a.win.gs1 + (long)rem * a.W;
      const float* tg = a.win.target[v] + (long)s * a.win.ts1 + (long)rem * a.W;
      for (int u = lig; u < units; u += G) {
        const Vec<W4> tv = ld<W4>(tg + u * W4);
#pragma unroll
        for (int c = 0; c < W4; ++c) tsum += (double)comp(tv, c);
        const float* gu = g + u * W4;
        int i0 = 0;
        for (; i0 + kRowsInFlight <= n0; i0 += kRowsInFlight) {
          Vec<W4> gr[kRowsInFlight];
#pragma unroll
          for (int k = 0; k < kRowsInFlight; ++k) gr[k] = ld<W4>(gu + (long)(i0 + k) * gs0);
#pragma unroll
          for (int k = 0; k < kRowsInFlight; ++k)
#pragma unroll
            for (int c = 0; c < W4; ++c) gsum += (double)comp(gr[k], c);
        }
        for (; i0 < n0; ++i0) {
          const Vec<W4> gv = ld<W4>(gu + (long)i0 * gs0);
#pragma unroll
          for (int c = 0; c < W4; ++c) gsum += (double)comp(gv, c);
        }
      }
    }
    for (int m = G >> 1; m >= 1; m >>= 1) {
      gsum += __shfl_xor(gsum, m);
      tsum += __shfl_xor(tsum, m);
    }
    if (active && lig == 0) {
      const unsigned long t = rem / (unsigned)a.H, lat = rem - t * (unsigned)a.H;
      // accumulator element: variable v, sample s < n1, time t_start + t < n_timesteps (entry point), latitude lat < H
      const long at = (((long)v * a.win.n1 + (long)s) * a.n_timesteps + (a.t_start + (long)t)) * a.H + (long)lat;
      a.gen_acc[at] += sdy_fs_zonal_mean(gsum, n0, a.W);
      a.target_acc[at] += sdy_fs_zonal_mean(tsum, 1, a.W);
    }
  }
}

// the time offset into the accumulators: window times t_start .. t_start + T - 1 must all exist (in 64 bits: no wrap)
bool times_fit(const sdy_window& w, int t_start, int n_timesteps) {
  return n_timesteps >= 1 && t_start >= 0 && (long)t_start + (long)w.T <= (long)n_timesteps;
}

// the window's own checks are sdy_window_check's; here what bounds an accumulator address
int check_video(const sdy_video_args* a) {
  if (!a) return SDY_ERR_ARG;
  if (!times_fit(a->win, a->t_start, a->n_timesteps)) return SDY_ERR_ARG;
  if (!a->gen_mean || !a->target_mean) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, a->HW));
  // flat accumulator indices are 64-bit
  if ((long)a->n_timesteps * a->HW >= (1L << 40)) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

int check_zonal(const sdy_zonal_args* a) {
  if (!a) return SDY_ERR_ARG;
  if (a->H < 1 || a->W < 1) return SDY_ERR_ARG;
  if (!times_fit(a->win, a->t_start, a->n_timesteps)) return SDY_ERR_ARG;
  if (!a->gen_acc || !a->target_acc) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, (long)a->H * a->W));
  // 64-bit flat accumulator indices: one sample's (n_timesteps, H) and a variable's n1 of them stay far inside the range
  if ((long)a->n_timesteps * a->H >= (1L << 40)) return SDY_ERR_UNSUPPORTED;
  if ((long)a->win.n1 * ((long)a->n_timesteps * a->H) >= (1L << 50)) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

bool extended(const sdy_video_args* a) { return a->gen_sq || a->target_sq || a->err_var || a->err_min || a->err_max; }

template <bool EXT>
void video_host(const sdy_video_args* a) {
  const sdy_window& w = a->win;
  const long HW = a->HW;
  for (int v = 0; v < w.nvars; ++v)
    for (int t = 0; t < w.T; ++t)
      for (long p = 0; p < HW; ++p) {
        const float* g = w.gen[v] + t * HW + p;
        const float* tg = w.target[v] + t * HW + p;
        sdy_fs_point<EXT> st;
        sdy_fs_init(st);
        for (long i1 = 0; i1 < w.n1; ++i1) {
          const float tv = tg[i1 * w.ts1];
          sdy_fs_add_target(st, tv);
          for (long i0 = 0; i0 < w.n0; ++i0) sdy_fs_add_gen(st, g[i0 * w.gs0 + i1 * w.gs1], tv);
        }
        const long at = ((long)v * a->n_timesteps + (a->t_start + t)) * HW + p;
        sdy_fs_store(st, at, w.n0 * w.n1, w.n1, a->gen_mean, a->target_mean, a->gen_sq, a->target_sq, a->err_var, a->err_min,
                     a->err_max);
      }
}

}  // namespace

extern "C" int sdy_video_accumulate_host(const sdy_video_args* a) {
  SDY_TRY(check_video(a));
  if (extended(a))
    video_host<true>(a);
  else
    video_host<false>(a);
  return SDY_OK;
}

extern "C" int sdy_video_accumulate(const sdy_video_args* a, void* stream) {
  SDY_TRY(check_video(a));
  const bool vec = sdy_window_vec4(&a->win, a->HW);
  const unsigned n_items = (unsigned)((long)a->win.T * (vec ? a->HW / 4 : a->HW));
  const dim3 grid(sdy_grid_cap((n_items + 255u) / 256u, a->win.nvars, kBlocksPerLaunch, kMinBlocksPerVar), a->win.nvars);
  const hipStream_t s = (hipStream_t)stream;
  if (extended(a)) {
    if (vec)
      hipLaunchKernelGGL((video_kernel<4, true>), grid, dim3(256), 0, s, *a, n_items);
    else
      hipLaunchKernelGGL((video_kernel<1, true>), grid, dim3(256), 0, s, *a, n_items);
  } else {
    if (vec)
      hipLaunchKernelGGL((video_kernel<4, false>), grid, dim3(256), 0, s, *a, n_items);
    else
      hipLaunchKernelGGL((video_kernel<1, false>), grid, dim3(256), 0, s, *a, n_items);
  }
  return sdy_launch_status();
}

extern "C" int sdy_zonal_accumulate_host(const sdy_zonal_args* a) {
  SDY_TRY(check_zonal(a));
  const sdy_window& w = a->win;
  const long W = a->W, TH = (long)w.T * a->H;
  for (int v = 0; v < w.nvars; ++v)
    for (long s = 0; s < w.n1; ++s)
      for (long rem = 0; rem < TH; ++rem) {
        const float* g = w.gen[v] + s * w.gs1 + rem * W;
        const float* tg = w.target[v] + s * w.ts1 + rem * W;
        double gsum = 0.0, tsum = 0.0;
        for (long p = 0; p < W; ++p) tsum += (double)tg[p];
        for (long i0 = 0; i0 < w.n0; ++i0)
          for (long p = 0; p < W; ++p) gsum += (double)g[i0 * w.gs0 + p];
        const long t = rem / a->H, lat = rem - t * a->H;
        const long at = (((long)v * w.n1 + s) * a->n_timesteps + (a->t_start + t)) * a->H + lat;
        a->gen_acc[at] += sdy_fs_zonal_mean(gsum, w.n0, a->W);
        a->target_acc[at] += sdy_fs_zonal_mean(tsum, 1, a->W);
      }
  return SDY_OK;
}

extern "C" int sdy_zonal_accumulate(const sdy_zonal_args* a, void* stream) {
  SDY_TRY(check_zonal(a));
  const bool vec = sdy_window_vec4(&a->win, a->W);
  const int units = vec ? a->W / 4 : a->W;
  int G = 1;                                       // lanes per latitude row: one wave, or a power-of-two part of one
  while (G < 64 && G < units) G <<= 1;
  const unsigned long n_rows = (unsigned long)a->win.n1 * a->win.T * a->H;
  const unsigned long rows_per_block = 256 / G;
  const dim3 grid(sdy_grid_cap((n_rows + rows_per_block - 1) / rows_per_block, a->win.nvars, kBlocksPerLaunch, kMinBlocksPerVar),
                  a->win.nvars);
  if (vec)
    hipLaunchKernelGGL(zonal_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, *a, G, n_rows);
  else
    hipLaunchKernelGGL(zonal_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, *a, G, n_rows);
  return sdy_launch_status();
}

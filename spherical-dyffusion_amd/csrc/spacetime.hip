// Wavenumber-frequency power of an equatorial band (no counterpart in the reference), gfx950.  Two entry points:
//   append: block (pair, window time; trajectory; variable) stages the pair's two rows in LDS (16-byte loads when the window
//     allows them) and thread c owns the chain of (fold, k) = (c / (K + 1), c % (K + 1)) over the W longitudes: a direct sum
//     with the caller's cos / sin table, any W, written into the ring slot of the time.
//   segment_power: block (variable, trajectory, pair, fold, tile of wavenumbers) stages the N ring values of the tile's columns
//     in LDS in time order, a thread per (column, part) takes the trend, all threads detrend and taper in place, then a thread
//     owns the frequencies f = thread, thread + 256, .. and walks the N times once per group of kColumns columns with the
//     time table in LDS (all lanes read the same column value: a broadcast).  P goes to the workspace; the second launch adds
//     the columns of every accumulator cell in (member, pair) order with sdy_sum_chunks and adds the sum to the cell.
// No atomics.  The per-thread state (kColumns complex sums) is indexed at compile time only.  The arithmetic is spacetime.h.
#include <initializer_list>
#include <vector>

#include "common.h"
#include "ordered_sum.h"
#include "spacetime.h"
#include "window.h"

namespace {

constexpr int kStoreThreads = 128;
constexpr int kPowerThreads = 256;
constexpr int kStaged = 2048;        // complex values of a tile in LDS (32 KiB)
constexpr int kMaxTile = 8;          // columns of a tile: min(kMaxTile, kStaged / N), at least 2
constexpr int kColumns = 4;          // columns a thread carries through one walk over the times
constexpr long kSumBlocks = 1L << 20;
constexpr long kIndexLimit = 1L << 50;

// the product of positive factors, or -1 when it reaches `limit`
long product_below(long limit, std::initializer_list<long> factors) {
  long p = 1;
  for (long f : factors) {
    if (p > (limit - 1) / f) return -1;
    p *= f;
  }
  return p;
}

int tile_columns(int N) { return kStaged / N < kMaxTile ? kStaged / N : kMaxTile; }

// ---- append ------------------------------------------------------------------------------------------------------------------
// Bounds (entry point): W <= SDY_ST_MAX_LON, row indices inside 0 .. H - 1, t0 <= t < t1 <= T, K <= W / 2, coef indices < 2^50.
template <int W4>
__global__ __launch_bounds__(kStoreThreads) void spacetime_store_kernel(const sdy_spacetime_append_args a) {
  __shared__ float rows[2][SDY_ST_MAX_LON];
  const int v = blockIdx.z;
  const int W = a.W, K1 = a.K + 1, R = a.R;
  const long plane = (long)a.H * W;
  const unsigned n1 = (unsigned)a.win.n1;
  const unsigned gen_rows = (unsigned)a.win.n0 * n1, n_traj = gen_rows + n1;
  const int tt = blockIdx.x / R, p = blockIdx.x - tt * R;
  const int slot = (int)((a.n_first + tt) % a.N);
  const long row_n = (long)(a.t0 + tt) * plane + (long)a.north[p] * W;
  const long row_s = (long)(a.t0 + tt) * plane + (long)a.south[p] * W;
  for (unsigned r = blockIdx.y; r < n_traj; r += gridDim.y) {
    const float* src;
    if (r < gen_rows) {
      const unsigned i0 = r / n1, i1 = r - i0 * n1;
      src = a.win.gen[v] + (long)i0 * a.win.gs0 + (long)i1 * a.win.gs1;
    } else {
      src = a.win.target[v] + (long)(r - gen_rows) * a.win.ts1;
    }
    __syncthreads();                           // the chains of the trajectory before are done with the rows
    for (int i = threadIdx.x; i < W / W4; i += kStoreThreads) {
      const Vec<W4> xn = ld<W4>(src + row_n + (long)i * W4), xs = ld<W4>(src + row_s + (long)i * W4);
#pragma unroll
      for (int c = 0; c < W4; ++c) {
        rows[0][i * W4 + c] = comp(xn, c);
        rows[1][i * W4 + c] = comp(xs, c);
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * K1; c += kStoreThreads) {
      const int fold = c / K1, k = c - fold * K1;
      double re = 0.0, im = 0.0;
      int i = 0;
      for (int j = 0; j < W; ++j) {
        const double y = sdy_st_fold(rows[0][j], rows[1][j], fold);
        sdy_st_lon_step(re, im, y, a.lon_table[2 * i], a.lon_table[2 * i + 1]);
        i = sdy_st_next(i, k, W);
      }
      double* const out = a.coef + sdy_st_coef_at(v, n_traj, r, a.N, slot, R, p, fold, K1, k);
      out[0] = sdy_st_lon_scale(re, W);
      out[1] = sdy_st_lon_scale(im, W);
    }
  }
}

int check(const sdy_spacetime_append_args* a) {
  if (!a || a->struct_size != sizeof(sdy_spacetime_append_args)) return SDY_ERR_ARG;
  if (a->H < 1 || a->W < 1 || a->R < 1) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, (long)a->H * a->W));
  if (!a->lon_table || !a->coef || ((uintptr_t)a->lon_table & 7) || ((uintptr_t)a->coef & 7)) return SDY_ERR_ARG;
  if (a->K < 0 || a->K > a->W / 2) return SDY_ERR_ARG;
  if (a->N < 4 || a->N > SDY_ST_MAX_SEGMENT) return SDY_ERR_ARG;
  if (a->t0 < 0 || a->t1 < a->t0 || a->t1 > a->win.T || a->t1 - a->t0 > a->N || a->n_first < 0) return SDY_ERR_ARG;
  if (a->R > SDY_ST_MAX_PAIRS || a->W > SDY_ST_MAX_LON) return SDY_ERR_UNSUPPORTED;
  for (int p = 0; p < a->R; ++p)
    if (a->north[p] < 0 || a->north[p] >= a->H || a->south[p] < 0 || a->south[p] >= a->H) return SDY_ERR_ARG;
  if (a->n_first >= kIndexLimit) return SDY_ERR_UNSUPPORTED;
  const long n_traj = (long)a->win.n0 * a->win.n1 + a->win.n1;          // n0 * n1 < 2^31 (sdy_window_check)
  if (product_below(kIndexLimit, {(long)a->win.nvars, n_traj, (long)a->N, (long)a->R, 2L, (long)a->K + 1, 2L}) < 0)
    return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

// ---- segment power -----------------------------------------------------------------------------------------------------------
// Bounds (entry point): 4 <= N <= SDY_ST_MAX_SEGMENT, kt = tile_columns(N) in 2 .. kMaxTile and N * kt <= kStaged, first_slot
// inside 0 .. N - 1, blocks < 2^31, coef and workspace indices < 2^50.
__global__ __launch_bounds__(kPowerThreads) void spacetime_power_kernel(const sdy_spacetime_segment_power_args a, int kt,
                                                                          int tiles) {
  __shared__ double z[kStaged * 2];                    // [n][column of the tile][re, im]
  __shared__ double table[SDY_ST_MAX_SEGMENT * 2];
  __shared__ double trend[kMaxTile * 2 * 2];           // per (column, part): mean, slope
  __shared__ double norm_shared;
  const int N = a.N, R = a.R, K1 = a.K + 1;
  const long n_traj = (long)a.M * a.B + a.B;
  long at = blockIdx.x;
  const int tile = (int)(at % tiles);
  at /= tiles;
  const int fold = (int)(at & 1);
  at >>= 1;
  const int p = (int)(at % R);
  at /= R;
  const long r = at % n_traj, v = at / n_traj;
  const int k0 = tile * kt;
  const int kn = K1 - k0 < kt ? K1 - k0 : kt;
  const int tid = threadIdx.x;
  const int parts = kn * 2;

  for (int i = tid; i < N * parts; i += kPowerThreads) {
    const int n = i / parts, rem = i - n * parts;
    z[n * kt * 2 + rem] = a.coef[sdy_st_coef_at(v, n_traj, r, N, sdy_st_slot(a.first_slot, n, N), R, p, fold, K1, k0) + rem];
  }
  for (int i = tid; i < 2 * N; i += kPowerThreads) table[i] = a.time_table[i];
  __syncthreads();
  if (tid < parts) {
    double mean, slope;
    sdy_st_trend(z + tid, (long)kt * 2, N, a.detrend, mean, slope);
    trend[tid * 2] = mean;
    trend[tid * 2 + 1] = slope;
  } else if (tid == 64) {
    norm_shared = sdy_st_norm(a.taper, N);
  }
  __syncthreads();
  for (int i = tid; i < N * parts; i += kPowerThreads) {
    const int n = i / parts, rem = i - n * parts;
    z[n * kt * 2 + rem] = sdy_st_value(z[n * kt * 2 + rem], n, N, a.detrend, trend[rem * 2], trend[rem * 2 + 1], a.taper[n]);
  }
  __syncthreads();
  const double norm = norm_shared;
  double* const out = reinterpret_cast<double*>(a.ws) + sdy_st_partial_at(v, a.M, a.B, r, R, p, fold, N, K1);
  for (int f = tid; f < N; f += kPowerThreads)
    for (int g = 0; g < kn; g += kColumns) {
      double re[kColumns], im[kColumns];
#pragma unroll
      for (int c = 0; c < kColumns; ++c) re[c] = im[c] = 0.0;
      int u = 0;
      for (int n = 0; n < N; ++n) {
        const double cs = table[2 * u], sn = table[2 * u + 1];
        const double* const zn = z + n * kt * 2;
#pragma unroll
        for (int c = 0; c < kColumns; ++c) {
          const int kk = g + c < kn ? g + c : kn - 1;      // a column past the tile repeats the last one and stores nothing
          sdy_st_time_step(re[c], im[c], zn[kk * 2], zn[kk * 2 + 1], cs, sn);
        }
        u = sdy_st_next(u, f, N);
      }
#pragma unroll
      for (int c = 0; c < kColumns; ++c)
        if (g + c < kn) out[(long)f * K1 + k0 + g + c] = sdy_st_power(re[c], im[c], norm);
    }
}

// acc[v][side][b][fold][f][k] += the chain over the cell's columns; one thread per cell, grid-strided
__global__ __launch_bounds__(kPowerThreads) void spacetime_sum_kernel(const sdy_spacetime_segment_power_args a) {
  const long fk = (long)a.N * (a.K + 1);
  const long cells = (long)a.nvars * 2 * a.B * 2 * fk;
  const double* const ws = reinterpret_cast<const double*>(a.ws);
  for (long i = (long)blockIdx.x * kPowerThreads + threadIdx.x; i < cells; i += (long)gridDim.x * kPowerThreads) {
    const long e = i % fk;
    long g = i / fk;
    const long fold = g & 1;
    g >>= 1;
    const long b = g % a.B;
    g /= a.B;
    const long side = g & 1, v = g >> 1;
    int chunks;
    const long base = sdy_st_cell_chunks(v, a.M, a.B, side, b, fold, a.R, a.N, a.K + 1, chunks);
    a.acc[i] = a.acc[i] + sdy_sum_chunks(ws + base, chunks, fk, e);
  }
}

int check(const sdy_spacetime_segment_power_args* a, bool device, long* blocks) {
  if (!a || a->struct_size != sizeof(sdy_spacetime_segment_power_args)) return SDY_ERR_ARG;
  if (!a->coef || !a->taper || !a->time_table || !a->acc) return SDY_ERR_ARG;
  if (((uintptr_t)a->coef | (uintptr_t)a->taper | (uintptr_t)a->time_table | (uintptr_t)a->acc) & 7) return SDY_ERR_ARG;
  if (a->nvars < 1 || a->M < 1 || a->B < 1 || a->R < 1 || a->K < 0) return SDY_ERR_ARG;
  if (a->N < 4 || a->N > SDY_ST_MAX_SEGMENT || a->first_slot < 0 || a->first_slot >= a->N) return SDY_ERR_ARG;
  if (a->detrend < 0 || a->detrend > 2) return SDY_ERR_ARG;
  const size_t need = sdy_spacetime_workspace_bytes(a->nvars, a->M, a->B, a->N, a->R, a->K);
  if (need == 0) return SDY_ERR_UNSUPPORTED;
  if ((device || a->ws) && !sdy_ws_ok(a->ws, a->ws_bytes, need)) return SDY_ERR_ARG;
  const long n_traj = (long)a->M * a->B + a->B;
  const int kt = tile_columns(a->N);
  const long n = product_below(1L << 31, {(long)a->nvars, n_traj, (long)a->R, 2L, (long)((a->K + 1 + kt - 1) / kt)});
  if (n < 0) return SDY_ERR_UNSUPPORTED;
  *blocks = n;
  return SDY_OK;
}

}  // namespace

extern "C" size_t sdy_spacetime_workspace_bytes(int nvars, int M, int B, int N, int R, int K) {
  if (nvars < 1 || M < 1 || B < 1 || N < 4 || N > SDY_ST_MAX_SEGMENT || R < 1 || K < 0) return 0;
  if (product_below(1L << 31, {(long)M, (long)R}) < 0) return 0;                       // the chunks of a cell: an int
  const long n_traj = (long)M * B + B;
  const long coef = product_below(kIndexLimit, {(long)nvars, n_traj, (long)N, (long)R, 2L, (long)K + 1, 2L});
  return coef < 0 ? 0 : (size_t)coef / 2 * sizeof(double);
}

extern "C" int sdy_spacetime_append_host(const sdy_spacetime_append_args* a) {
  SDY_TRY(check(a));
  const sdy_window& w = a->win;
  const int W = a->W, K1 = a->K + 1;
  const long plane = (long)a->H * W;
  const long gen_rows = (long)w.n0 * w.n1, n_traj = gen_rows + w.n1;
  for (int v = 0; v < w.nvars; ++v)
    for (long r = 0; r < n_traj; ++r) {
      const float* src = r < gen_rows ? w.gen[v] + (r / w.n1) * w.gs0 + (r % w.n1) * w.gs1 : w.target[v] + (r - gen_rows) * w.ts1;
      for (int t = a->t0; t < a->t1; ++t) {
        const int slot = (int)((a->n_first + (t - a->t0)) % a->N);
        for (int p = 0; p < a->R; ++p) {
          const float* const xn = src + t * plane + (long)a->north[p] * W;
          const float* const xs = src + t * plane + (long)a->south[p] * W;
          for (int fold = 0; fold < 2; ++fold)
            for (int k = 0; k < K1; ++k) {
              double re = 0.0, im = 0.0;
              int i = 0;
              for (int j = 0; j < W; ++j) {
                sdy_st_lon_step(re, im, sdy_st_fold(xn[j], xs[j], fold), a->lon_table[2 * i], a->lon_table[2 * i + 1]);
                i = sdy_st_next(i, k, W);
              }
              double* const out = a->coef + sdy_st_coef_at(v, n_traj, r, a->N, slot, a->R, p, fold, K1, k);
              out[0] = sdy_st_lon_scale(re, W);
              out[1] = sdy_st_lon_scale(im, W);
            }
        }
      }
    }
  return SDY_OK;
}

extern "C" int sdy_spacetime_append(const sdy_spacetime_append_args* a, void* stream) {
  SDY_TRY(check(a));
  if (a->t1 == a->t0) return SDY_OK;               // a window that holds the initial condition only
  const long n_traj = (long)a->win.n0 * a->win.n1 + a->win.n1;
  // R <= H and (t1 - t0) * H * W <= 2^30: the x extent fits
  const dim3 grid((unsigned)(a->R * (a->t1 - a->t0)), (unsigned)(n_traj < 65535 ? n_traj : 65535), a->win.nvars);
  if (sdy_window_vec4(&a->win, a->W))
    hipLaunchKernelGGL((spacetime_store_kernel<4>), grid, dim3(kStoreThreads), 0, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL((spacetime_store_kernel<1>), grid, dim3(kStoreThreads), 0, (hipStream_t)stream, *a);
  return sdy_launch_status();
}

extern "C" int sdy_spacetime_segment_power_host(const sdy_spacetime_segment_power_args* a) {
  long blocks;
  SDY_TRY(check(a, false, &blocks));
  const int N = a->N, R = a->R, K1 = a->K + 1;
  const long n_traj = (long)a->M * a->B + a->B;
  const long fk = (long)N * K1;
  const double norm = sdy_st_norm(a->taper, N);
  std::vector<double> partials((size_t)a->nvars * sdy_st_partials_per_var(a->M, a->B, R, N, K1));
  std::vector<double> zr(N), zi(N);
  for (long v = 0; v < a->nvars; ++v)
    for (long r = 0; r < n_traj; ++r)
      for (int p = 0; p < R; ++p)
        for (int fold = 0; fold < 2; ++fold) {
          double* const out = partials.data() + sdy_st_partial_at(v, a->M, a->B, r, R, p, fold, N, K1);
          for (int k = 0; k < K1; ++k) {
            for (int n = 0; n < N; ++n) {
              const double* const c = a->coef + sdy_st_coef_at(v, n_traj, r, N, sdy_st_slot(a->first_slot, n, N), R, p, fold, K1, k);
              zr[n] = c[0];
              zi[n] = c[1];
            }
            double mr, sr, mi, si;
            sdy_st_trend(zr.data(), 1, N, a->detrend, mr, sr);
            sdy_st_trend(zi.data(), 1, N, a->detrend, mi, si);
            for (int n = 0; n < N; ++n) {
              zr[n] = sdy_st_value(zr[n], n, N, a->detrend, mr, sr, a->taper[n]);
              zi[n] = sdy_st_value(zi[n], n, N, a->detrend, mi, si, a->taper[n]);
            }
            for (int f = 0; f < N; ++f) {
              double re = 0.0, im = 0.0;
              int u = 0;
              for (int n = 0; n < N; ++n) {
                sdy_st_time_step(re, im, zr[n], zi[n], a->time_table[2 * u], a->time_table[2 * u + 1]);
                u = sdy_st_next(u, f, N);
              }
              out[(long)f * K1 + k] = sdy_st_power(re, im, norm);
            }
          }
        }
  const long cells = (long)a->nvars * 2 * a->B * 2 * fk;
  for (long i = 0; i < cells; ++i) {
    const long e = i % fk;
    long g = i / fk;
    const long fold = g & 1;
    g >>= 1;
    const long b = g % a->B;
    g /= a->B;
    const long side = g & 1, v = g >> 1;
    int chunks;
    const long base = sdy_st_cell_chunks(v, a->M, a->B, side, b, fold, R, N, K1, chunks);
    a->acc[i] = a->acc[i] + sdy_sum_chunks(partials.data() + base, chunks, fk, e);
  }
  return SDY_OK;
}

extern "C" int sdy_spacetime_segment_power(const sdy_spacetime_segment_power_args* a, void* stream) {
  long blocks;
  SDY_TRY(check(a, true, &blocks));
  const int kt = tile_columns(a->N);
  const int tiles = (a->K + 1 + kt - 1) / kt;
  hipLaunchKernelGGL(spacetime_power_kernel, dim3((unsigned)blocks), dim3(kPowerThreads), 0, (hipStream_t)stream, *a, kt, tiles);
  const long cells = (long)a->nvars * 2 * a->B * 2 * a->N * (a->K + 1);
  const long want = (cells + kPowerThreads - 1) / kPowerThreads;
  hipLaunchKernelGGL(spacetime_sum_kernel, dim3((unsigned)(want < kSumBlocks ? want : kSumBlocks)), dim3(kPowerThreads), 0,
                     (hipStream_t)stream, *a);
  return sdy_launch_status();
}

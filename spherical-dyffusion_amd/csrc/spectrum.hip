// Per-degree power spectra of the generated, the target and the error coefficients, gfx950: a streaming reduction over the
// coefficient tensors sdy_legendre_fwd leaves in the internal layout Cs[l][m][ri][field] (one image, fields innermost), folded
// into float64 accumulators that stay on the device.  Every coefficient of a listed field is needed once (the target's again
// for the error).  One wave owns one accumulator element (variable, time, degree): its lanes take four consecutive rows each
// -- consecutive fields, 16 bytes per lane where the group starts on a 16-byte boundary -- walk the orders m = 0 .. min(l,
// mtr - 1) in order, and meet in a butterfly of cross-lane moves.  No LDS, no atomics.  The arithmetic and its order are
// spectrum.h.
// What this mapping costs: a wave's load of one plane covers the rows of ONE (variable, time), 4 * rows bytes.  With 256 or
// more rows every lane loads; with the 25 rows of the headline ensemble 7 lanes of 64 do (1 for its single target row), a load
// fetches 112 of a 128-byte line and the waves of neighbouring times fetch the rest of that line again (from L2 when they run
// close in time); with one row per element (sdy_amd.power_spectrum) one lane works and a line is shared by 32 waves.  The
// order of a row's sum (orders ascending) is what ties a lane to a row; a wave that spans several times of a plane would fill
// its lanes without changing that order and is the next step.
#include "common.h"
#include "spectrum.h"

namespace {

constexpr int kLanes = SDY_SP_SLOTS / 4;   // one wave
static_assert(kLanes == 64, "a wave holds the slots, four per lane");

struct Quad { float v[4]; };

// rows r0 .. r0 + 3 of a run that starts at p[0] and holds `rows` rows; rows past the end read as 0 and are never loaded
template <bool VEC>
__device__ __forceinline__ Quad ld_quad(const float* p, int r0, int rows) {
  Quad q;
  if (VEC && r0 + 4 <= rows) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(p + r0);
    q.v[0] = x.x; q.v[1] = x.y; q.v[2] = x.z; q.v[3] = x.w;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) q.v[c] = r0 + c < rows ? p[r0 + c] : 0.0f;
  }
  return q;
}

__device__ __forceinline__ double wave_butterfly(double x) {
#pragma clang fp contract(off)
  for (int m = 1; m < kLanes; m <<= 1) x = x + __shfl_xor(x, m);
  return x;
}

// blockIdx = (degree l, window time t, variable v); 64 threads
template <bool VEC_G, bool VEC_T, bool ERR>
__global__ __launch_bounds__(kLanes) void degree_power_kernel(const sdy_spectrum_args a) {
  const int l = blockIdx.x, t = blockIdx.y, v = blockIdx.z, lane = threadIdx.x;
  const int mlast = l < a.mtr - 1 ? l : a.mtr - 1;
  const int R = a.n0 * a.n1, n1 = a.n1;
  const long Fg = a.gen_fields, Ft = a.target_fields;
  // first field of the element's rows (entry point: every row's field is inside its buffer), and the planes of (l, m = 0)
  const long gf0 = (long)v * a.gen_var_stride + (long)t * a.gen_time_stride;
  const long tf0 = (long)v * a.target_var_stride + (long)t * a.target_time_stride;
  const float* g = a.gen + (long)l * a.mtr * 2 * Fg + gf0;
  const float* tg = a.target + (long)l * a.mtr * 2 * Ft + tf0;

  double gs[4] = {0.0, 0.0, 0.0, 0.0}, es[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r0 = 4 * lane; r0 < R; r0 += SDY_SP_SLOTS) {
    int i1[4];
    double gsc[4], tsc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      i1[c] = (r0 + c) % n1;
      gsc[c] = (a.gen_scale && r0 + c < R) ? (double)a.gen_scale[gf0 + r0 + c] : 1.0;
      tsc[c] = (ERR && a.target_scale) ? (double)a.target_scale[tf0 + i1[c]] : 1.0;
    }
    double p[4] = {0.0, 0.0, 0.0, 0.0}, e[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (int m = 0; m <= mlast; ++m) {
      const Quad re = ld_quad<VEC_G>(g + (long)(2 * m) * Fg, r0, R);
      const Quad im = ld_quad<VEC_G>(g + (long)(2 * m + 1) * Fg, r0, R);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        p[c] = sdy_sp_add(p[c], re.v[c], im.v[c], gsc[c], m);
        if (ERR && r0 + c < R) {
          const float tre = tg[(long)(2 * m) * Ft + i1[c]], tim = tg[(long)(2 * m + 1) * Ft + i1[c]];
          e[c] = sdy_sp_add_err(e[c], re.v[c], im.v[c], gsc[c], tre, tim, tsc[c], m);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      gs[c] += p[c];
      es[c] += e[c];
    }
  }
  double ts[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r0 = 4 * lane; r0 < n1; r0 += SDY_SP_SLOTS) {
    double p[4] = {0.0, 0.0, 0.0, 0.0}, tsc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) tsc[c] = (a.target_scale && r0 + c < n1) ? (double)a.target_scale[tf0 + r0 + c] : 1.0;
#pragma unroll 2
    for (int m = 0; m <= mlast; ++m) {
      const Quad re = ld_quad<VEC_T>(tg + (long)(2 * m) * Ft, r0, n1);
      const Quad im = ld_quad<VEC_T>(tg + (long)(2 * m + 1) * Ft, r0, n1);
#pragma unroll
      for (int c = 0; c < 4; ++c) p[c] = sdy_sp_add(p[c], re.v[c], im.v[c], tsc[c], m);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) ts[c] += p[c];
  }
  // every lane takes part in the butterfly (lanes without rows bring 0.0)
  const double gsum = wave_butterfly(sdy_sp_fold4(gs[0], gs[1], gs[2], gs[3]));
  const double tsum = wave_butterfly(sdy_sp_fold4(ts[0], ts[1], ts[2], ts[3]));
  double esum = 0.0;
  if (ERR) esum = wave_butterfly(sdy_sp_fold4(es[0], es[1], es[2], es[3]));
  if (lane == 0) {
    // accumulator element: variable v < nvars, time t_start + t < n_timesteps (entry point), degree l < lmax
    const long at = ((long)v * a.n_timesteps + (a.t_start + (long)t)) * a.lmax + l;
    a.gen_power[at] += sdy_sp_mean(gsum, R);
    a.target_power[at] += sdy_sp_mean(tsum, n1);
    if (ERR) a.err_power[at] += sdy_sp_mean(esum, R);
  }
}

// everything that bounds an address or an index, for the device and the host entry points alike
int check_spectrum(const sdy_spectrum_args* a) {
  if (!a) return SDY_ERR_ARG;
  if (!a->gen || !a->target || !a->gen_power || !a->target_power) return SDY_ERR_ARG;
  if (a->lmax < 1 || a->mtr < 1 || a->gen_fields < 1 || a->target_fields < 1) return SDY_ERR_ARG;
  if (a->nvars < 1 || a->n0 < 1 || a->n1 < 1 || a->T < 1 || a->n_timesteps < 1) return SDY_ERR_ARG;
  if (a->mtr > a->lmax) return SDY_ERR_ARG;                 // mtr = min(mmax, lmax) of the plan that wrote the coefficients
  if (a->gen_var_stride < 0 || a->gen_time_stride < 0 || a->target_var_stride < 0 || a->target_time_stride < 0)
    return SDY_ERR_ARG;
  // the time offset into the accumulators: window times t_start .. t_start + T - 1 must all exist (in 64 bits: no wrap)
  if (a->t_start < 0 || (long)a->t_start + (long)a->T > (long)a->n_timesteps) return SDY_ERR_ARG;
  // 32-bit row numbers, 16-bit grid extents for times and variables; flat indices are 64-bit
  if ((long)a->n0 * a->n1 >= (1L << 31) - SDY_SP_SLOTS) return SDY_ERR_UNSUPPORTED;
  if (a->T > 65535 || a->nvars > 65535) return SDY_ERR_UNSUPPORTED;
  const long cs_rows = (long)a->lmax * a->mtr * 2;
  if (cs_rows * a->gen_fields >= (1L << 40) || cs_rows * a->target_fields >= (1L << 40)) return SDY_ERR_UNSUPPORTED;
  if ((long)a->nvars * a->n_timesteps >= (1L << 40) / a->lmax) return SDY_ERR_UNSUPPORTED;
  // the last row of the last time of the last variable must be a field of its buffer
  const long R = (long)a->n0 * a->n1;
  const long g_last = (long)(a->nvars - 1) * a->gen_var_stride + (long)(a->T - 1) * a->gen_time_stride + R - 1;
  const long t_last = (long)(a->nvars - 1) * a->target_var_stride + (long)(a->T - 1) * a->target_time_stride + a->n1 - 1;
  if (g_last >= a->gen_fields || t_last >= a->target_fields) return SDY_ERR_ARG;
  return SDY_OK;
}

bool aligned16(const float* p, int fields, int var_stride, int time_stride) {
  return ((uintptr_t)p & 15) == 0 && ((fields | var_stride | time_stride) & 3) == 0;
}

template <bool VEC_G, bool VEC_T>
void launch(const sdy_spectrum_args* a, hipStream_t s) {
  const dim3 grid(a->lmax, a->T, a->nvars);
  if (a->err_power)
    hipLaunchKernelGGL((degree_power_kernel<VEC_G, VEC_T, true>), grid, dim3(kLanes), 0, s, *a);
  else
    hipLaunchKernelGGL((degree_power_kernel<VEC_G, VEC_T, false>), grid, dim3(kLanes), 0, s, *a);
}

}  // namespace

extern "C" int sdy_degree_power_host(const sdy_spectrum_args* a) {
  SDY_TRY(check_spectrum(a));
  const long Fg = a->gen_fields, Ft = a->target_fields;
  const int R = a->n0 * a->n1, n1 = a->n1;
  double gs[SDY_SP_SLOTS], ts[SDY_SP_SLOTS], es[SDY_SP_SLOTS];
  for (int v = 0; v < a->nvars; ++v)
    for (int t = 0; t < a->T; ++t)
      for (int l = 0; l < a->lmax; ++l) {
        const int mlast = l < a->mtr - 1 ? l : a->mtr - 1;
        const long gf0 = (long)v * a->gen_var_stride + (long)t * a->gen_time_stride;
        const long tf0 = (long)v * a->target_var_stride + (long)t * a->target_time_stride;
        const float* g = a->gen + (long)l * a->mtr * 2 * Fg + gf0;
        const float* tg = a->target + (long)l * a->mtr * 2 * Ft + tf0;
        for (int s = 0; s < SDY_SP_SLOTS; ++s) gs[s] = ts[s] = es[s] = 0.0;
        for (int r = 0; r < R; ++r) {
          const int i1 = r % n1;
          const double gsc = a->gen_scale ? (double)a->gen_scale[gf0 + r] : 1.0;
          const double tsc = a->target_scale ? (double)a->target_scale[tf0 + i1] : 1.0;
          double p = 0.0, e = 0.0;
          for (int m = 0; m <= mlast; ++m) {
            const float re = g[(long)(2 * m) * Fg + r], im = g[(long)(2 * m + 1) * Fg + r];
            p = sdy_sp_add(p, re, im, gsc, m);
            if (a->err_power)
              e = sdy_sp_add_err(e, re, im, gsc, tg[(long)(2 * m) * Ft + i1], tg[(long)(2 * m + 1) * Ft + i1], tsc, m);
          }
          gs[r % SDY_SP_SLOTS] += p;
          es[r % SDY_SP_SLOTS] += e;
        }
        for (int r = 0; r < n1; ++r) {
          const double tsc = a->target_scale ? (double)a->target_scale[tf0 + r] : 1.0;
          double p = 0.0;
          for (int m = 0; m <= mlast; ++m)
            p = sdy_sp_add(p, tg[(long)(2 * m) * Ft + r], tg[(long)(2 * m + 1) * Ft + r], tsc, m);
          ts[r % SDY_SP_SLOTS] += p;
        }
        const long at = ((long)v * a->n_timesteps + (a->t_start + (long)t)) * a->lmax + l;
        a->gen_power[at] += sdy_sp_mean(sdy_sp_fold_slots(gs), R);
        a->target_power[at] += sdy_sp_mean(sdy_sp_fold_slots(ts), n1);
        if (a->err_power) a->err_power[at] += sdy_sp_mean(sdy_sp_fold_slots(es), R);
      }
  return SDY_OK;
}

extern "C" int sdy_degree_power(const sdy_spectrum_args* a, void* stream) {
  SDY_TRY(check_spectrum(a));
  const bool vg = aligned16(a->gen, a->gen_fields, a->gen_var_stride, a->gen_time_stride);
  const bool vt = aligned16(a->target, a->target_fields, a->target_var_stride, a->target_time_stride);
  const hipStream_t s = (hipStream_t)stream;
  if (vg && vt) launch<true, true>(a, s);
  else if (vg) launch<true, false>(a, s);
  else if (vt) launch<false, true>(a, s);
  else launch<false, false>(a, s);
  return sdy_launch_status();
}

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
#include "coef_rows.h"
#include "spectrum.h"

namespace {

// rows r0 .. r0 + 3 of a run that starts at p[0] and holds `rows` rows; rows past the end read as 0 and are never loaded.
// (vector_spectrum.hip has a branch-free ld_quad of its own: there a branch per row multiplied the kernel's code past the
// instruction cache; here the branch keeps a quad past the end from being loaded at all.)
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

// blockIdx = (degree l, window time t, variable v); 64 threads
template <bool VEC_G, bool VEC_T, bool ERR>
__global__ __launch_bounds__(kLanes) void degree_power_kernel(const sdy_spectrum_args a) {
  const int l = blockIdx.x, t = blockIdx.y, v = blockIdx.z, lane = threadIdx.x;
  // sdy_coef_rows_element(a.rows, v, t, l), spelled out: with the helper, in every form tried, the compiler orders the loads of
  // the kernel's arguments differently and the kernel comes out as other code than it had before the descriptor
  const int mlast = l < a.rows.mtr - 1 ? l : a.rows.mtr - 1;
  const int R = a.rows.n0 * a.rows.n1, n1 = a.rows.n1;
  const long Fg = a.rows.gen_fields, Ft = a.rows.target_fields;
  const long gf0 = (long)v * a.rows.gen_var_stride + (long)t * a.rows.gen_time_stride;
  const long tf0 = (long)v * a.rows.target_var_stride + (long)t * a.rows.target_time_stride;
  const float* g = a.gen + (long)l * a.rows.mtr * 2 * Fg + gf0;
  const float* tg = a.target + (long)l * a.rows.mtr * 2 * Ft + tf0;

  double gs[4] = {0.0, 0.0, 0.0, 0.0}, es[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r0 = 4 * lane; r0 < R; r0 += SDY_SP_SLOTS) {
    int i1[4];
    double gsc[4], tsc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      i1[c] = (r0 + c) % n1;
      gsc[c] = (a.rows.gen_scale && r0 + c < R) ? (double)a.rows.gen_scale[gf0 + r0 + c] : 1.0;
      tsc[c] = (ERR && a.rows.target_scale) ? (double)a.rows.target_scale[tf0 + i1[c]] : 1.0;
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
    for (int c = 0; c < 4; ++c) tsc[c] = (a.rows.target_scale && r0 + c < n1) ? (double)a.rows.target_scale[tf0 + r0 + c] : 1.0;
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
    const long at = ((long)v * a.rows.n_timesteps + (a.rows.t_start + (long)t)) * a.rows.lmax + l;   // the element's `at`
    a.gen_power[at] += sdy_sp_mean(gsum, R);
    a.target_power[at] += sdy_sp_mean(tsum, n1);
    if (ERR) a.err_power[at] += sdy_sp_mean(esum, R);
  }
}

template <bool VEC_G, bool VEC_T, bool ERR>
struct Launch {
  static void go(const sdy_spectrum_args& a, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((degree_power_kernel<VEC_G, VEC_T, ERR>), grid, dim3(kLanes), 0, s, a);
  }
};

// the entry points' own checks in front of the descriptor's, for the device and the host entry points alike
int check_spectrum(const sdy_spectrum_args* a) {
  if (!a) return SDY_ERR_ARG;
  if (!a->gen || !a->target || !a->gen_power || !a->target_power) return SDY_ERR_ARG;
  return sdy_coef_rows_check(&a->rows, 0, 0);
}

}  // namespace

extern "C" int sdy_degree_power_host(const sdy_spectrum_args* a) {
  SDY_TRY(check_spectrum(a));
  const sdy_coef_rows& r = a->rows;
  const long Fg = r.gen_fields, Ft = r.target_fields;
  const int R = r.n0 * r.n1, n1 = r.n1;
  double gs[SDY_SP_SLOTS], ts[SDY_SP_SLOTS], es[SDY_SP_SLOTS];
  sdy_coef_rows_walk(r, [&](const sdy_coef_element el) {
    const float *g = a->gen + el.gl, *tg = a->target + el.tl;
    for (int s = 0; s < SDY_SP_SLOTS; ++s) gs[s] = ts[s] = es[s] = 0.0;
    for (int row = 0; row < R; ++row) {
      const int i1 = row % n1;
      const double gsc = r.gen_scale ? (double)r.gen_scale[el.gf0 + row] : 1.0;
      const double tsc = r.target_scale ? (double)r.target_scale[el.tf0 + i1] : 1.0;
      double p = 0.0, e = 0.0;
      for (int m = 0; m <= el.mlast; ++m) {
        const float re = g[(long)(2 * m) * Fg + row], im = g[(long)(2 * m + 1) * Fg + row];
        p = sdy_sp_add(p, re, im, gsc, m);
        if (a->err_power)
          e = sdy_sp_add_err(e, re, im, gsc, tg[(long)(2 * m) * Ft + i1], tg[(long)(2 * m + 1) * Ft + i1], tsc, m);
      }
      gs[row % SDY_SP_SLOTS] += p;
      es[row % SDY_SP_SLOTS] += e;
    }
    for (int row = 0; row < n1; ++row) {
      const double tsc = r.target_scale ? (double)r.target_scale[el.tf0 + row] : 1.0;
      double p = 0.0;
      for (int m = 0; m <= el.mlast; ++m)
        p = sdy_sp_add(p, tg[(long)(2 * m) * Ft + row], tg[(long)(2 * m + 1) * Ft + row], tsc, m);
      ts[row % SDY_SP_SLOTS] += p;
    }
    sdy_coef_rows_add(a->gen_power, el.at, gs, R);
    sdy_coef_rows_add(a->target_power, el.at, ts, n1);
    if (a->err_power) sdy_coef_rows_add(a->err_power, el.at, es, R);
  });
  return SDY_OK;
}

extern "C" int sdy_degree_power(const sdy_spectrum_args* a, void* stream) {
  SDY_TRY(check_spectrum(a));
  const sdy_coef_rows& r = a->rows;
  const bool vg = sdy_coef_rows_vec4(a->gen, nullptr, r.gen_fields, 0, r.gen_var_stride, r.gen_time_stride);
  const bool vt = sdy_coef_rows_vec4(a->target, nullptr, r.target_fields, 0, r.target_var_stride, r.target_time_stride);
  sdy_coef_rows_dispatch<Launch>(r, vg, vt, a->err_power != nullptr, *a, (hipStream_t)stream);
  return sdy_launch_status();
}

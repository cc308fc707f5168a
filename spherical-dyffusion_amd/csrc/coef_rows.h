// What the two entry points that embed an sdy_coef_rows (include/sdy_amd.h) share, spectrum.hip and vector_spectrum.hip, the
// kernels and the _host twins alike: the check of the descriptor, the 16-byte test of a side, the addressing of one
// accumulator element, the wave's lanes and their butterfly, the dispatch over the kernels' three switches and the walk of the
// host twins over the elements.  The arithmetic stays where it is defined: spectrum.h, vector_spectrum.h.
#pragma once
#include "common.h"
#include "spectrum.h"

// everything of the descriptor that bounds an address or an index, for the device and the host entry points alike.  The v
// offsets: how far behind a row's field its second field lies (vector_spectrum.hip; 0, 0 for one field per row).
inline int sdy_coef_rows_check(const sdy_coef_rows* a, int gen_v_offset, int target_v_offset) {
  if (a->lmax < 1 || a->mtr < 1 || a->gen_fields < 1 || a->target_fields < 1) return SDY_ERR_ARG;
  if (a->nvars < 1 || a->n0 < 1 || a->n1 < 1 || a->T < 1 || a->n_timesteps < 1) return SDY_ERR_ARG;
  if (a->mtr > a->lmax) return SDY_ERR_ARG;                 // mtr = min(mmax, lmax) of the plan that wrote the coefficients
  if (a->gen_var_stride < 0 || a->gen_time_stride < 0 || a->target_var_stride < 0 || a->target_time_stride < 0)
    return SDY_ERR_ARG;
  if (gen_v_offset < 0 || target_v_offset < 0) return SDY_ERR_ARG;
  // the time offset into the accumulators: window times t_start .. t_start + T - 1 must all exist (in 64 bits: no wrap)
  if (a->t_start < 0 || (long)a->t_start + (long)a->T > (long)a->n_timesteps) return SDY_ERR_ARG;
  // 32-bit row numbers, 16-bit grid extents for times and variables; flat indices are 64-bit
  if ((long)a->n0 * a->n1 >= (1L << 31) - SDY_SP_SLOTS) return SDY_ERR_UNSUPPORTED;
  if (a->T > 65535 || a->nvars > 65535) return SDY_ERR_UNSUPPORTED;
  const long cs_rows = (long)a->lmax * a->mtr * 2;
  if (cs_rows * a->gen_fields >= (1L << 40) || cs_rows * a->target_fields >= (1L << 40)) return SDY_ERR_UNSUPPORTED;
  if ((long)a->nvars * a->n_timesteps >= (1L << 40) / a->lmax) return SDY_ERR_UNSUPPORTED;
  // the last row of the last time of the last variable, and its second field, must be fields of their buffer
  const long R = (long)a->n0 * a->n1;
  const long g_last = (long)(a->nvars - 1) * a->gen_var_stride + (long)(a->T - 1) * a->gen_time_stride + R - 1;
  const long t_last = (long)(a->nvars - 1) * a->target_var_stride + (long)(a->T - 1) * a->target_time_stride + a->n1 - 1;
  if (g_last + gen_v_offset >= a->gen_fields || t_last + target_v_offset >= a->target_fields) return SDY_ERR_ARG;
  return SDY_OK;
}

// 16-byte loads of one side allowed?  p, q: its coefficient tensors (q may be NULL)
inline bool sdy_coef_rows_vec4(const float* p, const float* q, int fields, int v_offset, int var_stride, int time_stride) {
  return (((uintptr_t)p | (uintptr_t)q) & 15) == 0 && ((fields | v_offset | var_stride | time_stride) & 3) == 0;
}

// One accumulator element (variable v, window time t, degree l): its last order, the first field of its rows on either side
// (sdy_coef_rows_check: every row's field is inside its buffer), the offsets of the planes of (l, m = 0) at those fields, and
// the element's place in the accumulators (v < nvars, t_start + t < n_timesteps, l < lmax).
struct sdy_coef_element {
  int mlast;
  long gf0, tf0, gl, tl, at;
};

// The host twins call it (sdy_coef_rows_walk).  The two kernels spell the same expressions out, each with a comment that names
// this function: called from a kernel -- by value, by reference, whole or in parts -- it changes the order in which the
// compiler loads the kernel's arguments, degree_power_kernel comes out as other code than it had, and six of the eight
// instantiations of vector_degree_power_kernel take one more scalar register (NOTEBOOK.md 7zd).  By value all the same, so
// that it stays callable from a kernel (NOTEBOOK.md 7zc: what a reference into by-value kernel arguments costs).
SDY_SP_HD sdy_coef_element sdy_coef_rows_element(const sdy_coef_rows r, int v, int t, int l) {
  sdy_coef_element e;
  e.mlast = l < r.mtr - 1 ? l : r.mtr - 1;
  e.gf0 = (long)v * r.gen_var_stride + (long)t * r.gen_time_stride;
  e.tf0 = (long)v * r.target_var_stride + (long)t * r.target_time_stride;
  e.gl = (long)l * r.mtr * 2 * (long)r.gen_fields + e.gf0;
  e.tl = (long)l * r.mtr * 2 * (long)r.target_fields + e.tf0;
  e.at = ((long)v * r.n_timesteps + (r.t_start + (long)t)) * r.lmax + l;
  return e;
}

// the host twins: every element of the call in the order (v, t, l), handed to body(element)
template <class Body>
void sdy_coef_rows_walk(const sdy_coef_rows& r, Body body) {
  for (int v = 0; v < r.nvars; ++v)
    for (int t = 0; t < r.T; ++t)
      for (int l = 0; l < r.lmax; ++l) body(sdy_coef_rows_element(r, v, t, l));
}

// the host twins: the slots of one element meet, and their mean over `rows` rows is added to the accumulator
inline void sdy_coef_rows_add(double* acc, long at, double* slots, int rows) {
  acc[at] += sdy_sp_mean(sdy_sp_fold_slots(slots), rows);
}

constexpr int kLanes = SDY_SP_SLOTS / 4;   // one wave
static_assert(kLanes == 64, "a wave holds the slots, four per lane");

struct Quad { float v[4]; };

__device__ __forceinline__ double wave_butterfly(double x) {
#pragma clang fp contract(off)
  for (int m = 1; m < kLanes; m <<= 1) x = x + __shfl_xor(x, m);
  return x;
}

// Launch<VEC_G, VEC_T, ERR>::go(args, grid, stream) for the run-time switches: 16-byte loads of the generated side, of the
// target side, error accumulators.  grid = (degree l, window time t, variable v), one wave each.
template <template <bool, bool, bool> class Launch, bool VEC_G, bool VEC_T, class Args>
void sdy_coef_rows_launch(bool err, const Args& a, dim3 grid, hipStream_t s) {
  if (err)
    Launch<VEC_G, VEC_T, true>::go(a, grid, s);
  else
    Launch<VEC_G, VEC_T, false>::go(a, grid, s);
}

template <template <bool, bool, bool> class Launch, class Args>
void sdy_coef_rows_dispatch(const sdy_coef_rows& r, bool vec_g, bool vec_t, bool err, const Args& a, hipStream_t s) {
  const dim3 grid(r.lmax, r.T, r.nvars);
  if (vec_g && vec_t) sdy_coef_rows_launch<Launch, true, true>(err, a, grid, s);
  else if (vec_g) sdy_coef_rows_launch<Launch, true, false>(err, a, grid, s);
  else if (vec_t) sdy_coef_rows_launch<Launch, false, true>(err, a, grid, s);
  else sdy_coef_rows_launch<Launch, false, false>(err, a, grid, s);
}

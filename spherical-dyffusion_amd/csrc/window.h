// What the field aggregators that read a window in place share (field_stats.hip, member_mean.hip, rank_hist.hip,
// event_verif.hip, fss.hip, spells.hip, variability.hip, region_series.hip, member_gram.hip; coarsen.hip takes the grid cap):
// the 16-byte / 4-byte load helpers, the checks and the alignment test of an sdy_window (include/sdy_amd.h) and the grid cap
// of a launch that covers all variables.
#pragma once
#include "common.h"

template <int W>
using Vec = std::conditional_t<W == 4, f32x4, float>;
template <int W>
__device__ __forceinline__ Vec<W> ld(const float* p) { return *reinterpret_cast<const Vec<W>*>(p); }
__device__ __forceinline__ float comp(float v, int) { return v; }
__device__ __forceinline__ float comp(f32x4 v, int c) { return v[c]; }

// everything of a window that bounds an address, for the device and the host entry points alike; plane = the grid points of
// one time (sdy_window's contract)
inline int sdy_window_check(const sdy_window* w, long plane) {
  if (w->nvars < 1 || w->nvars > SDY_MAX_VARS) return SDY_ERR_ARG;
  if (w->n0 < 1 || w->n1 < 1 || w->T < 1 || plane < 1) return SDY_ERR_ARG;
  if (w->gs0 < 0 || w->gs1 < 0 || w->ts1 < 0) return SDY_ERR_ARG;
  for (int v = 0; v < w->nvars; ++v)
    if (!w->gen[v] || !w->target[v]) return SDY_ERR_ARG;
  // 32-bit work items within a variable, 32-bit row numbers
  if ((long)w->T * plane > (1L << 30) || (long)w->n0 * w->n1 >= (1L << 31)) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

// 16-byte loads allowed?  `inner`: the extent a thread's loads run along (the plane, or a latitude row)
inline bool sdy_window_vec4(const sdy_window* w, long inner) {
  bool vec = (inner & 3) == 0 && ((w->gs0 | w->gs1 | w->ts1) & 3) == 0;
  for (int v = 0; v < w->nvars; ++v) vec = vec && (((uintptr_t)w->gen[v] | (uintptr_t)w->target[v]) & 15) == 0;
  return vec;
}

// blocks per variable of a launch over all variables: a share of blocks_per_launch, at least min_per_var; a variable with more
// work strides over its items
inline unsigned sdy_grid_cap(unsigned long blocks, int nvars, int blocks_per_launch, int min_per_var) {
  const unsigned long cap = blocks_per_launch / nvars > min_per_var ? blocks_per_launch / nvars : min_per_var;
  return (unsigned)(blocks < cap ? blocks : cap);
}

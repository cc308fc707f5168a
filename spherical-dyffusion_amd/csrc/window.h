// What the field aggregators that read a window in place share (field_stats.hip, member_mean.hip, rank_hist.hip,
// event_verif.hip, fss.hip, spells.hip, variability.hip, region_series.hip, member_gram.hip; coarsen.hip takes the grid cap):
// the 16-byte / 4-byte load helpers, the checks and the alignment test of an sdy_window (include/sdy_amd.h), the grid cap
// of a launch that covers all variables and the lanes that share an accumulator row.
#pragma once
#include "common.h"

template <int W>
using Vec = std::conditional_t<W == 4, f32x4, float>;
template <int W>
__device__ __forceinline__ Vec<W> ld(const float* p) { return *reinterpret_cast<const Vec<W>*>(p); }
__device__ __forceinline__ float comp(float v, int) { return v; }
__device__ __forceinline__ float comp(f32x4 v, int c) { return v[c]; }

// A load of W4 floats as (wave-uniform 64-bit base) + (32-bit byte offset per lane), the SADDR form of global_load (see
// sdy_ld16s, common.h): a member's base is scalar arithmetic, and a thread keeps one offset for the target and every member
// of a unit instead of one 64-bit address per load in flight.
typedef float __attribute__((address_space(1))) gfloat;
template <int W4>
__device__ __forceinline__ Vec<W4> ld_u(const float* ubase, unsigned off_b);
template <>
__device__ __forceinline__ f32x4 ld_u<4>(const float* ubase, unsigned off_b) { return sdy_ld16s(ubase, off_b); }
template <>
__device__ __forceinline__ float ld_u<1>(const float* ubase, unsigned off_b) {
  sdy_gcptr_t b = (sdy_gcptr_t)ubase;
  asm volatile("" : "+s"(b), "+v"(off_b));
  return *reinterpret_cast<const gfloat*>(b + off_b);
}

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

// Lanes per accumulator row of the kernels whose lane groups own one (rank_hist.hip, event_verif.hip), a power of two in
// kMinLaneGroup .. 64 (units: the 16-byte or 4-byte loads of one latitude row).  A row of at most 16 units takes one pass of the
// narrowest group that covers it.  A longer row takes the group of 16, 32 or 64 lanes that leaves the fewest lane slots idle
// over its passes, the wider one of equals (longer contiguous runs per load): 90 units (360 longitudes) -> 32 lanes x 3
// passes, 90 of 96 slots busy, where one wave per row has 90 of 128.
constexpr int kMinLaneGroup = 4;
inline int lane_group(int units) {
  if (units <= 16) {
    int G = kMinLaneGroup;
    while (G < units) G <<= 1;
    return G;
  }
  int best = 16;
  long best_slots = 16L * ((units + 15) / 16);
  for (int G = 32; G <= 64; G <<= 1) {
    const long slots = (long)G * ((units + G - 1) / G);
    if (slots <= best_slots) {
      best = G;
      best_slots = slots;
    }
  }
  return best;
}

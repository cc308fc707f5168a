// Per-grid-point quantiles along time, as ONE definition for the device kernels (quantile.hip) and the host entry points
// sdy_time_quantile_append_host / sdy_time_quantile_select_host: the sortable key of an fp32 value and its inverse, the rank
// rule that turns (q, n) into the order statistics to find, the value of a quantile from them, and where a key and an output
// live.  The only floating-point arithmetic is the rank rule and the interpolation: float64, contraction off.
#pragma once
#include "../../include/sdy_amd.h"   // SDY_MAX_QUANTILES = 8
#include "events.h"                  // SDY_EV_HD

#define SDY_Q_NAN_KEY 0xFFFFFFFFu    // the key of every NaN, and the fill of a series: "nothing recorded here"
#define SDY_Q_LINEAR 0
#define SDY_Q_LOWER 1
#define SDY_Q_HIGHER 2

// The key of x: -0.0 is +0.0; the bits with the sign flipped when it is clear, all bits flipped when it is set.  Unsigned
// order of keys = order of values, -inf (0x007FFFFF) first and +inf (0xFF800000) last; no value has the NaN key.
SDY_EV_HD unsigned sdy_q_key(float x) {
  if (x != x) return SDY_Q_NAN_KEY;
  unsigned u = __builtin_bit_cast(unsigned, x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}

// the value of a key that is not the NaN key, bit for bit
SDY_EV_HD float sdy_q_value_of(unsigned key) {
  const unsigned u = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
  return __builtin_bit_cast(float, u);
}

// Rank rule for n >= 1 values: h = q (n - 1), one product; j = min(floor(h), n - 1) -> the 0-based rank of `lo`; g = h - j.
SDY_EV_HD unsigned sdy_q_rank(double q, unsigned n, double& g) {
#pragma clang fp contract(off)
  const double h = q * (double)(n - 1u);
  double f = __builtin_floor(h);
  const double top = (double)(n - 1u);
  if (f > top) f = top;
  g = h - f;
  return (unsigned)f;
}

// The rank of `hi` is min(j + 1, n - 1).  With `below_or_equal` = the number of values <= lo (at least j + 1) and `next` the
// smallest value above lo: hi is lo while that rank is still among the ties of lo, else `next`.
SDY_EV_HD unsigned sdy_q_hi_key(unsigned lo_key, unsigned j, unsigned n, unsigned below_or_equal, unsigned next_key) {
  const unsigned r = j + 1u < n - 1u ? j + 1u : n - 1u;
  return r < below_or_equal ? lo_key : next_key;
}

// The quantile from lo, hi (fp32 values, exact in float64) and g.  `linear` is numpy's _lerp, and returns lo when g == 0 or
// lo == hi, which keeps ties and equal infinities from producing inf - inf or 0 * inf.
SDY_EV_HD double sdy_q_quantile(double lo, double hi, double g, int method) {
#pragma clang fp contract(off)
  if (method == SDY_Q_LOWER) return lo;
  if (method == SDY_Q_HIGHER) return g > 0.0 ? hi : lo;
  if (g == 0.0 || lo == hi) return lo;
  const double d = hi - lo;
  if (g >= 0.5) {
    const double back = d * (1.0 - g);
    return hi - back;
  }
  const double step = d * g;
  return lo + step;
}

// the trajectories of a variable (spells.h): the generated ones member-major, then the targets; the targets alone without gen
SDY_EV_HD long sdy_q_trajectories(long n0, long n1, int store_gen) { return store_gen ? n0 * n1 + n1 : n1; }

// series[v, r, slot, p] of the contiguous (nvars, n_traj, capacity, plane) keys; the entry points bound the product below 2^50
SDY_EV_HD long sdy_q_series_at(long v, long n_traj, long r, long capacity, long slot, long plane, long p) {
  return (((v * n_traj + r) * capacity + slot) * plane) + p;
}

// Regional area-weighted metric sums (sdy_region_series, include/sdy_amd.h) as ONE definition for the device kernel
// (region_series.hip) and the host entry point sdy_region_series_host: what the members and the target of one grid point
// give (sdy_rs_point), and what that point adds to the eight sums of one region (sdy_rs_add).
//
// ZERO-WEIGHT RULE: a point whose weight in a region is exactly 0 contributes nothing to that region, whatever its values,
// NaN included (not IEEE's 0 x NaN = NaN: ocean-only fields with NaN over land stay usable, and a stretch of points in which
// a region has no weight can be skipped).  Anywhere else a NaN propagates.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_RS_HD __host__ __device__ inline
#else
#define SDY_RS_HD inline
#endif

// the partition of a plane: chunks of SDY_RS_CHUNK consecutive points (a rule of HW alone), a chunk's SDY_RS_QUARTERS quarters
// are summed one by one and added in ascending order, then the chunks in ascending order
enum { SDY_RS_CHUNK = 1024, SDY_RS_QUARTERS = 4, SDY_RS_QUARTER = SDY_RS_CHUNK / SDY_RS_QUARTERS };
// the eight sums, in the order of sdy_ensemble_series
enum { SDY_RS_MSE = 0, SDY_RS_VAR = 1, SDY_RS_CRPS = 2, SDY_RS_BIAS = 3, SDY_RS_GEN = 4, SDY_RS_GEN_SQ = 5, SDY_RS_TGT = 6,
       SDY_RS_TGT_SQ = 7, SDY_RS_SUMS = 8 };

SDY_RS_HD long sdy_rs_chunks(long HW) { return (HW + SDY_RS_CHUNK - 1) / SDY_RS_CHUNK; }

// W neighbouring grid points at once (W = 4 with 16-byte loads, else 1).  member(i, g) -> the W values of member i, widened
// (called more than once per member: the caller re-reads them, so nobody keeps a member array); y the targets.
//   e = em - y = mean_m (g_m - y)        fair CRPS: mean_m |g_m - y| - sum_{i<j} |g_i - g_j| / (M (M - 1))
//   member variance: sum_m ((g_m - y) - e)^2 / (M - 1)
// M == 1: CRPS = |g - y|, variance 0.  All float64, nothing contracted.
template <int W, class Member>
SDY_RS_HD void sdy_rs_point(int M, const double (&y)[W], Member member, double (&e)[W], double (&var)[W], double (&crps)[W]) {
#pragma clang fp contract(off)
  double sum_d[W], sum_abs[W], pairs[W], dev2[W];
#pragma unroll
  for (int c = 0; c < W; ++c) sum_d[c] = sum_abs[c] = pairs[c] = dev2[c] = 0.0;
  for (int i = 0; i < M; ++i) {
    double g[W];
    member(i, g);
#pragma unroll
    for (int c = 0; c < W; ++c) {
      const double d = g[c] - y[c];
      sum_d[c] += d;
      sum_abs[c] += fabs(d);
    }
  }
#pragma unroll
  for (int c = 0; c < W; ++c) e[c] = sum_d[c] / (double)M;
  for (int i = 0; i < M; ++i) {
    double gi[W];
    member(i, gi);
#pragma unroll
    for (int c = 0; c < W; ++c) {
      const double dev = (gi[c] - y[c]) - e[c];
      dev2[c] += dev * dev;
    }
    for (int j = i + 1; j < M; ++j) {
      double gj[W];
      member(j, gj);
#pragma unroll
      for (int c = 0; c < W; ++c) pairs[c] += fabs(gi[c] - gj[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < W; ++c) {
    crps[c] = sum_abs[c] / (double)M;
    var[c] = 0.0;
    if (M > 1) {
      crps[c] -= pairs[c] / ((double)M * (double)(M - 1));
      var[c] = dev2[c] / (double)(M - 1);
    }
  }
}

// One point into the eight sums of one region; the caller has applied the zero-weight rule (w != 0).  em = y + e.
SDY_RS_HD void sdy_rs_add(double w, double e, double var, double crps, double y, double (&acc)[SDY_RS_SUMS]) {
#pragma clang fp contract(off)
  const double em = y + e;
  acc[SDY_RS_MSE] += w * (e * e);
  acc[SDY_RS_VAR] += w * var;
  acc[SDY_RS_CRPS] += w * crps;
  acc[SDY_RS_BIAS] += w * e;
  acc[SDY_RS_GEN] += w * em;
  acc[SDY_RS_GEN_SQ] += w * (em * em);
  acc[SDY_RS_TGT] += w * y;
  acc[SDY_RS_TGT_SQ] += w * (y * y);
}

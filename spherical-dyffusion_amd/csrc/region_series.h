// Regional area-weighted metric sums (sdy_region_series, include/sdy_amd.h) as ONE definition for the device kernel
// (region_series.hip) and the host entry point sdy_region_series_host: the partition of a plane, and what one grid point adds
// to the eight sums of one region (sdy_rs_add).  What the members and the target of a point give is sdy_ens_point
// (ensemble_point.h).
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

// The float64 ensemble statistics of one grid point, as ONE definition for the member-mean statistics (member_mean.h) and the
// regional series (region_series.hip), device kernels and host entry points alike.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_EP_HD __host__ __device__ inline
#else
#define SDY_EP_HD inline
#endif

struct sdy_ens_stats {
  double e, var, crps;
};

// member(i) -> the value g_i of member i, widened (called more than once per member: the caller re-reads it, so nobody keeps a
// member array); y the target.  first(i, d) sees d = g_i - y of every member once, in member order, during the first pass.
//   e = em - y = mean_m (g_m - y)        fair CRPS: mean_m |g_m - y| - sum_{i<j} |g_i - g_j| / (M (M - 1))
//   member variance: sum_m ((g_m - y) - e)^2 / (M - 1), the deviations taken from the differences to y
// M == 1: CRPS = |g - y|, variance 0.  All float64, nothing contracted.
template <class Member, class First>
SDY_EP_HD sdy_ens_stats sdy_ens_point(int M, double y, Member member, First first) {
#pragma clang fp contract(off)
  double sum_d = 0.0, sum_abs = 0.0;
  for (int i = 0; i < M; ++i) {
    const double d = member(i) - y;
    sum_d += d;
    sum_abs += fabs(d);
    first(i, d);
  }
  const double e = sum_d / (double)M;
  double pairs = 0.0, dev2 = 0.0;
  for (int i = 0; i < M; ++i) {
    const double gi = member(i);
    const double dev = (gi - y) - e;
    dev2 += dev * dev;
    for (int j = i + 1; j < M; ++j) pairs += fabs(gi - member(j));
  }
  double crps = sum_abs / (double)M, var = 0.0;
  if (M > 1) {
    crps -= pairs / ((double)M * (double)(M - 1));
    var = dev2 / (double)(M - 1);
  }
  return {e, var, crps};
}

// Per-member time means of an ensemble rollout and the statistics of the reference's ensemble TimeMeanAggregator
// (src/evaluation/aggregators/time_mean.py, is_ensemble=True) on them, as ONE definition for the device kernels
// (member_mean.hip) and the host entry points sdy_member_time_sum_host / sdy_member_map_stats_host: what one accumulator
// element gains from one window, and what one grid point of one sample contributes to the 2 M + 4 weighted sums.
#pragma once

#include <math.h>

#include "ensemble_point.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_MM_HD __host__ __device__ inline
#else
#define SDY_MM_HD inline
#endif

// One accumulator element, one window: the float64 sum of the element's fp32 values over the counted times, in ascending
// time.  sdy_mm_add is the whole arithmetic: a widening and one float64 addition per time (nothing to contract).
SDY_MM_HD double sdy_mm_add(double sum, float x) { return sum + (double)x; }

// the window's sum joins the running one (exactly one caller owns the accumulator element and stores the result)
SDY_MM_HD double sdy_mm_fold(double acc, double window_sum) { return acc + window_sum; }

// Slots of one variable's 2 M + 4 sums: [0, M) sum_w (g_m - t)^2, [M, 2M) sum_w (g_m - t), then the four below.
SDY_MM_HD int sdy_mm_slots(int M) { return 2 * M + 4; }
enum { SDY_MM_ENS_SQ = 0, SDY_MM_ENS_BIAS = 1, SDY_MM_CRPS = 2, SDY_MM_VAR = 3 };

// One grid point of one sample.  member(i) -> the time mean g_i of member i (called more than once per member: the caller
// re-reads it), t the target's time mean, w the area weight.  emit(slot, x) receives the point's term of every slot, each
// slot exactly once, in the same order for every point (the device sums a slot over a wave inside emit, so every lane of a
// wave has to arrive with the same slot).  The ensemble mean (t + mean_m (g_m - t)), the fair CRPS and the member variance
// are sdy_ens_point's (ensemble_point.h).  All float64, nothing contracted.
template <class Member, class Emit>
SDY_MM_HD void sdy_mm_point(int M, double t, double w, Member member, Emit emit) {
#pragma clang fp contract(off)
  const sdy_ens_stats r = sdy_ens_point(M, t, member, [&](int i, double d) {
    emit(i, w * (d * d));
    emit(M + i, w * d);
  });
  emit(2 * M + SDY_MM_ENS_SQ, w * (r.e * r.e));   // r.e: ensemble mean minus target
  emit(2 * M + SDY_MM_ENS_BIAS, w * r.e);
  emit(2 * M + SDY_MM_CRPS, w * r.crps);
  emit(2 * M + SDY_MM_VAR, w * r.var);
}

// Per-member time means of an ensemble rollout and the statistics of the reference's ensemble TimeMeanAggregator
// (src/evaluation/aggregators/time_mean.py, is_ensemble=True) on them, as ONE definition for the device kernels
// (member_mean.hip) and the host entry points sdy_member_time_sum_host / sdy_member_map_stats_host: what one accumulator
// element gains from one window, and what one grid point of one sample contributes to the 2 M + 4 weighted sums.
#pragma once

#include <math.h>

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
// wave has to arrive with the same slot).  All float64, nothing contracted.
//   ensemble mean: t + mean_m (g_m - t)        fair CRPS: mean_m |g_m - t| - sum_{i<j} |g_i - g_j| / (M (M - 1))
//   member variance: sum_m (g_m - mean)^2 / (M - 1), the deviations taken from the differences to t
// M == 1: CRPS = |g - t|, variance 0.
template <class Member, class Emit>
SDY_MM_HD void sdy_mm_point(int M, double t, double w, Member member, Emit emit) {
#pragma clang fp contract(off)
  double sum_d = 0.0, sum_abs = 0.0;
  for (int i = 0; i < M; ++i) {
    const double d = member(i) - t;
    sum_d += d;
    sum_abs += fabs(d);
    emit(i, w * (d * d));
    emit(M + i, w * d);
  }
  const double em = sum_d / (double)M;          // ensemble mean minus target
  emit(2 * M + SDY_MM_ENS_SQ, w * (em * em));
  emit(2 * M + SDY_MM_ENS_BIAS, w * em);
  double pairs = 0.0, dev2 = 0.0;
  for (int i = 0; i < M; ++i) {
    const double gi = member(i);
    const double dev = (gi - t) - em;
    dev2 += dev * dev;
    for (int j = i + 1; j < M; ++j) pairs += fabs(gi - member(j));
  }
  double crps = sum_abs / (double)M, var = 0.0;
  if (M > 1) {
    crps -= pairs / ((double)M * (double)(M - 1));
    var = dev2 / (double)(M - 1);
  }
  emit(2 * M + SDY_MM_CRPS, w * crps);
  emit(2 * M + SDY_MM_VAR, w * var);
}

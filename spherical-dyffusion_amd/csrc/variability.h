// Per-trajectory time variance and lag-1 autocorrelation at every grid point (no counterpart in the reference), as ONE
// definition for the device kernels (variability.hip) and the host entry points sdy_time_variability_*_host: what one state
// element gains from one counted time, what the state gives at the end of a run, and what one grid point of one sample
// contributes to the six weighted sums.
//
// One trajectory (a member of a sample, or a sample's target) at one grid point, counted times x_1 .. x_n (fp32) in run order:
//   c = x_1 (fp32), d_t = (double)x_t - (double)c, S1 = sum d_t, S2 = sum d_t d_t, P = sum_{t >= 2} d_{t-1} d_t, last = x_n (fp32)
// S1, S2 and P are float64; every time's term is added to the running value in ascending time, so the bits do not depend on how
// a run is cut into windows.  The shift by the first value keeps the variance of a field like surface pressure (1e5 +- 50) to
// float64 rounding of the DEVIATIONS; unshifted sums of x and x^2 would lose seven digits of it.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_TV_HD __host__ __device__ inline
#else
#define SDY_TV_HD inline
#endif

// the deviation of a value from the trajectory's origin: exact in float64 unless the two are more than 2^29 apart in exponent
SDY_TV_HD double sdy_tv_dev(float x, float c) { return (double)x - (double)c; }

// One counted time.  d: its deviation, d_prev: its predecessor's (whatever, when has_prev is false: the first counted time of
// a trajectory forms no product).  Products are rounded before they are added (nothing contracted).
SDY_TV_HD void sdy_tv_step(double& s1, double& s2, double& p, double d, double d_prev, bool has_prev) {
#pragma clang fp contract(off)
  s1 = s1 + d;
  const double dd = d * d;
  s2 = s2 + dd;
  if (has_prev) {
    const double pd = d_prev * d;
    p = p + pd;
  }
}

struct sdy_tv_moments {
  double V;          // sum_t (d_t - m)^2, clamped at 0 (NaN stays NaN)
  double variance;   // V / n (population)
  double lag1;       // sum_{t >= 2} (d_{t-1} - m)(d_t - m) / V; NaN unless n >= 2 and V > 0
};

// End of a run: n counted times (n >= 1, an integer held as a double).
//   m = S1 / n, V = max(S2 - S1 m, 0), C = P - m ((S1 - d_n) + S1) + (n - 1) m m       (d_1 = 0)
SDY_TV_HD sdy_tv_moments sdy_tv_finish(double s1, double s2, double p, float c, float last, double n) {
#pragma clang fp contract(off)
  sdy_tv_moments r;
  const double m = s1 / n;
  const double s1m = s1 * m;
  const double v = s2 - s1m;
  r.V = v < 0.0 ? 0.0 : v;                       // (not fmax: a NaN must stay one)
  r.variance = r.V / n;
  const double dn = sdy_tv_dev(last, c);
  const double ends = (s1 - dn) + s1;
  const double mends = m * ends;
  const double nm = (n - 1.0) * m;
  const double nmm = nm * m;
  const double cov = (p - mends) + nmm;
  r.lag1 = (n >= 2.0 && r.V > 0.0) ? cov / r.V : (double)NAN;
  return r;
}

// Slots of one variable's weighted sums.
enum {
  SDY_TV_VAR_GEN = 0,    // sum_w mean_m variance_gen
  SDY_TV_VAR_TARGET = 1, // sum_w variance_target
  SDY_TV_SD_SQ = 2,      // sum_w (mean_m sqrt(variance_gen) - sqrt(variance_target))^2
  SDY_TV_LAG_GEN = 3,    // over the mask: sum_w mean_m lag1_gen
  SDY_TV_LAG_TARGET = 4, // over the mask: sum_w lag1_target
  SDY_TV_LAG_W = 5,      // over the mask: sum_w
  SDY_TV_SLOTS = 6
};

// One grid point of one sample.  member(i) -> the sdy_tv_moments of member i (called once per member, in order), t the
// target's, w the area weight, n the counted times.  The mask: n >= 2, and the target and every member have V > 0.
// emit(slot, x) receives the point's term of every slot, each slot exactly once and in slot order (the device sums a slot over
// a wave inside emit, so every lane of a wave has to arrive with the same slot).  All float64, nothing contracted.
template <class Member, class Emit>
SDY_TV_HD void sdy_tv_point(int M, double n, double w, const sdy_tv_moments& t, Member member, Emit emit) {
#pragma clang fp contract(off)
  double sum_var = 0.0, sum_sd = 0.0, sum_lag = 0.0;
  bool defined = n >= 2.0 && t.V > 0.0;
  for (int i = 0; i < M; ++i) {
    const sdy_tv_moments g = member(i);
    sum_var += g.variance;
    sum_sd += sqrt(g.variance);
    defined = defined && g.V > 0.0;
    sum_lag += g.lag1;                            // (NaN where undefined: not looked at below unless every member is defined)
  }
  const double mean_var = sum_var / (double)M;
  const double sd_diff = sum_sd / (double)M - sqrt(t.variance);
  const double mean_lag = sum_lag / (double)M;
  emit(SDY_TV_VAR_GEN, w * mean_var);
  emit(SDY_TV_VAR_TARGET, w * t.variance);
  emit(SDY_TV_SD_SQ, w * (sd_diff * sd_diff));
  emit(SDY_TV_LAG_GEN, defined ? w * mean_lag : 0.0);
  emit(SDY_TV_LAG_TARGET, defined ? w * t.lag1 : 0.0);
  emit(SDY_TV_LAG_W, defined ? w : 0.0);
}

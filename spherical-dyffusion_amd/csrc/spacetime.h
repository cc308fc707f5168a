// Wavenumber-frequency power of an equatorial band (sdy_spacetime_append, sdy_spacetime_segment_power, include/sdy_amd.h), as ONE
// definition for the device kernels (spacetime.hip) and their _host twins: the fold of a row pair into its symmetric and
// antisymmetric part, a step of the longitude chain and its scaling, the trend of a column, the detrended and tapered value, a
// step of the time chain, the power of a frequency, and where a coefficient and a partial live.
//
// Everything is float64 and never contracted to FMA: a step of a chain is one rounded product and one rounded sum (the time
// chain: two of each per part), in the order written here.  No libm call: cos and sin come from the caller's tables.
#pragma once
#include "../../include/sdy_amd.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_ST_HD __host__ __device__ inline
#else
#define SDY_ST_HD inline
#endif

// (x_N + x_S) / 2 (fold 0) or (x_N - x_S) / 2 (fold 1): exact in float64 for fp32 inputs; an equator row (x_N == x_S) gives x and 0
SDY_ST_HD double sdy_st_fold(float xn, float xs, int fold) {
#pragma clang fp contract(off)
  const double n = (double)xn, s = (double)xs;
  return (fold ? n - s : n + s) * 0.5;
}

// one longitude of a (fold, k) chain: (re, im) += y (cos - i sin)
SDY_ST_HD void sdy_st_lon_step(double& re, double& im, double y, double c, double s) {
#pragma clang fp contract(off)
  const double yc = y * c, ys = y * s;
  re = re + yc;
  im = im - ys;
}

// the stored coefficient of a finished chain
SDY_ST_HD double sdy_st_lon_scale(double sum, int W) { return sum / (double)W; }

// (k j) mod W for the next j, without a division: i < W, k < W
SDY_ST_HD int sdy_st_next(int i, int k, int W) {
  const int n = i + k;
  return n >= W ? n - W : n;
}

// coef[v][r][slot][p][fold][k][part] of the contiguous (nvars, n_traj, N, R, 2, K + 1, 2) ring; the entry points bound the
// product below 2^50
SDY_ST_HD long sdy_st_coef_at(long v, long n_traj, long r, long N, long slot, long R, long p, long fold, long K1, long k) {
  return ((((((v * n_traj + r) * N + slot) * R + p) * 2 + fold) * K1 + k) * 2);
}

// the slot of a segment's time n
SDY_ST_HD int sdy_st_slot(int first_slot, int n, int N) {
  const int s = first_slot + n;
  return s >= N ? s - N : s;
}

// Mean and slope of one part (re or im) of a column: z[n * stride], n = 0 .. N - 1 in time order.  detrend 0 leaves both 0.
SDY_ST_HD void sdy_st_trend(const double* z, long stride, int N, int detrend, double& mean, double& slope) {
#pragma clang fp contract(off)
  mean = 0.0;
  slope = 0.0;
  if (detrend == 0) return;
  double s = 0.0;
  for (int n = 0; n < N; ++n) s = s + z[n * stride];
  mean = s / (double)N;
  if (detrend != 2) return;
  const double mid = 0.5 * (double)(N - 1);      // d_n = n - (N - 1) / 2: exact
  double sd = 0.0, dd = 0.0;
  for (int n = 0; n < N; ++n) {
    const double d = (double)n - mid;
    const double dz = d * z[n * stride], d2 = d * d;
    sd = sd + dz;
    dd = dd + d2;
  }
  slope = sd / dd;
}

// the detrended, tapered value of time n
SDY_ST_HD double sdy_st_value(double z, int n, int N, int detrend, double mean, double slope, double w) {
#pragma clang fp contract(off)
  double y = z;
  if (detrend != 0) y = y - mean;
  if (detrend == 2) {
    const double d = (double)n - 0.5 * (double)(N - 1);
    const double ds = d * slope;
    y = y - ds;
  }
  return y * w;
}

// N * sum_n w_n^2
SDY_ST_HD double sdy_st_norm(const double* w, int N) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int n = 0; n < N; ++n) {
    const double w2 = w[n] * w[n];
    s = s + w2;
  }
  return (double)N * s;
}

// one time of a frequency's chain: (re, im) += (a + i b)(cos - i sin)
SDY_ST_HD void sdy_st_time_step(double& re, double& im, double a, double b, double c, double s) {
#pragma clang fp contract(off)
  const double ac = a * c, bs = b * s, bc = b * c, as = a * s;
  re = (re + ac) + bs;
  im = (im + bc) - as;
}

SDY_ST_HD double sdy_st_power(double re, double im, double norm) {
#pragma clang fp contract(off)
  const double r2 = re * re, i2 = im * im;
  return (r2 + i2) / norm;
}

// The partial P of every column, ordered so that the columns one accumulator cell adds are chunks at one stride (sdy_sum_chunks):
// per variable the generated block (B, 2, M, R, N, K + 1), then the target block (B, 2, 1, R, N, K + 1).
SDY_ST_HD long sdy_st_partials_per_var(long M, long B, long R, long N, long K1) { return B * 2 * (M + 1) * R * N * K1; }
// the first element (f = 0, k = 0) of trajectory r's pair p and fold; r < M*B generated (member r / B, sample r % B), else target
SDY_ST_HD long sdy_st_partial_at(long v, long M, long B, long r, long R, long p, long fold, long N, long K1) {
  const long var = v * sdy_st_partials_per_var(M, B, R, N, K1);
  if (r < M * B) {
    const long m = r / B, b = r - m * B;
    return var + ((((b * 2 + fold) * M + m) * R + p) * N) * K1;
  }
  const long b = r - M * B;
  return var + (B * 2 * M * R * N * K1) + (((b * 2 + fold) * R + p) * N) * K1;
}
// the first chunk of an accumulator cell's (side, sample, fold), and the number of its chunks; the chunk stride is N * (K + 1)
SDY_ST_HD long sdy_st_cell_chunks(long v, long M, long B, long side, long b, long fold, long R, long N, long K1, int& chunks) {
  const long var = v * sdy_st_partials_per_var(M, B, R, N, K1);
  if (side == 0) {
    chunks = (int)(M * R);
    return var + ((b * 2 + fold) * M * R * N) * K1;
  }
  chunks = (int)R;
  return var + (B * 2 * M * R * N * K1) + ((b * 2 + fold) * R * N) * K1;
}

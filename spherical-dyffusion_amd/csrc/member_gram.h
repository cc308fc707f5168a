// The area-weighted Gram matrix of the member errors and the truth anomaly (sdy_member_gram, include/sdy_amd.h) as ONE
// definition for the device kernel (member_gram.hip) and the host entry point sdy_member_gram_host: the partition of a plane,
// the value of vector i at a grid point (sdy_gram_value) and the place of entry (i, j) in the packed triangle
// (sdy_gram_index; sdy_amd/field_scores.py restates the same formula).
//
// For one (variable, sample, time) with members g_0 .. g_{M-1}, target y, weights w and climatology c (absent: 0), N = M + 2:
//   a_0 = 1      a_{1+m} = (double)g_m - (double)y      a_{M+1} = (double)y - (double)c      Gamma[i][j] = sum_p w a_i a_j
// The differences of two fp32 values are exact in float64.
//
// ZERO-WEIGHT RULE (as region_series.h): a point with w == 0 contributes nothing, NaN and Inf included: every a_i of that point
// READS as 0, it is not multiplied by 0.  Anywhere else a NaN propagates into the entries of its own row and column only.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_GRAM_HD __host__ __device__ inline
#else
#define SDY_GRAM_HD inline
#endif

// The partition of a plane: chunks of SDY_GRAM_CHUNK consecutive points (a rule of HW alone).  A chunk's quarters are staged one
// after the other; wave k of SDY_GRAM_WAVES takes points 64 k .. 64 k + 63 of every quarter, four points (one matrix
// instruction per tile) at a time in ascending order, into one accumulator per entry.  A chunk's sum is wave 0 + wave 1 + wave 2
// + wave 3 in that order, a plane's sum its chunks in ascending order.
enum { SDY_GRAM_CHUNK = 1024, SDY_GRAM_QUARTERS = 4, SDY_GRAM_QUARTER = SDY_GRAM_CHUNK / SDY_GRAM_QUARTERS, SDY_GRAM_WAVES = 4,
       SDY_GRAM_WAVE_POINTS = SDY_GRAM_QUARTER / SDY_GRAM_WAVES, SDY_GRAM_STEP = 4 };

SDY_GRAM_HD long sdy_gram_chunks(long HW) { return (HW + SDY_GRAM_CHUNK - 1) / SDY_GRAM_CHUNK; }

// entries of the packed upper triangle of an N x N matrix
SDY_GRAM_HD long sdy_gram_entries(long N) { return N * (N + 1) / 2; }

// entry (i, j), 0 <= i <= j < N, of the packed upper triangle, row-major in (i, j >= i)
SDY_GRAM_HD long sdy_gram_index(long i, long j, long N) { return i * N - i * (i - 1) / 2 + (j - i); }

// a_i at a point.  x: the row's own fp32 value at the point (g_{i-1} for 1 <= i <= M; not looked at otherwise), y the target, c
// the climatology, w the weight.  Rows i >= N = M + 2 (the padding of the last 16-row block) are 0.
SDY_GRAM_HD double sdy_gram_value(int i, int M, float x, float y, float c, float w) {
  double a = 0.0;
  if (i == 0) a = 1.0;
  else if (i <= M) a = (double)x - (double)y;
  else if (i == M + 1) a = (double)y - (double)c;
  return w != 0.0f ? a : 0.0;       // the zero-weight rule: a select, not a product
}

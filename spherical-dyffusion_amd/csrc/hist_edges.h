// Bin edges, bin search and range doubling of the dynamic value histograms (src/ace_inference/core/histogram.py), as ONE
// definition for the device kernels (histogram.hip), the host entry points (sdy_hist_plan_host, sdy_hist_edges_host,
// sdy_hist_bins_host) and, through those, Python.  Everything is fp32, operation by operation as numpy 2.x evaluates it for
// float32 scalars, and never contracted to FMA.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_HIST_HD __host__ __device__ inline
#else
#define SDY_HIST_HD inline
#endif

constexpr int SDY_HIST_DOUBLING_CAP = 320;     // more doublings than fp32's exponent range can take (2^277 at most)
constexpr float SDY_HIST_EPSILON = 1.0e-6f;    // histogram.py:6, as the fp32 it becomes next to a float32 scalar
constexpr float SDY_HIST_F32_MAX = 3.402823466e+38f;

SDY_HIST_HD bool sdy_hist_finite(float v) { return v >= -SDY_HIST_F32_MAX && v <= SDY_HIST_F32_MAX; }   // false for NaN

// np.linspace(start, stop, n_bins + 1) for float32 scalars: step = fl32(fl32(stop - start) / n_bins),
// edge(i) = fl32(fl32(i * step) + start), edge(n_bins) = stop.
SDY_HIST_HD float sdy_hist_step(float start, float stop, int n_bins) {
#pragma clang fp contract(off)
  const float delta = stop - start;
  return delta / (float)n_bins;
}
SDY_HIST_HD float sdy_hist_edge(float start, float stop, float step, int n_bins, int i) {
#pragma clang fp contract(off)
  if (i >= n_bins) return stop;
  const float y = (float)i * step;
  return y + start;
}
// a range the bins can stand on: finite ends and a finite step above zero
SDY_HIST_HD bool sdy_hist_range_ok(float start, float stop, int n_bins) {
  const float step = sdy_hist_step(start, stop, n_bins);
  return sdy_hist_finite(start) && sdy_hist_finite(stop) && sdy_hist_finite(step) && step > 0.f;
}

// np.histogram(x, bins=edges): bin k holds [edge(k), edge(k+1)), the last bin is closed on the right, i.e. the LARGEST k in
// [0, n_bins) with edge(k) <= x.  -1 for a value outside [start, stop] or a NaN.  The guess from the bin width is corrected
// against the edges themselves (two steps each way), and where that does not settle it (steps below the spacing of fp32 at
// |start|: runs of equal edges) by a bisection of fixed length.  The result never leaves [0, n_bins).
SDY_HIST_HD int sdy_hist_bin(float x, float start, float stop, float step, float inv_step, int n_bins) {
#pragma clang fp contract(off)
  if (!(x >= start && x <= stop)) return -1;
  const float top = (float)(n_bins - 1);
  float g = (x - start) * inv_step;
  g = g < top ? g : top;            // NaN (0 * inf) lands on top as well
  g = g > 0.f ? g : 0.f;
  int k = (int)g;
#pragma unroll
  for (int s = 0; s < 2; ++s)
    if (k > 0 && x < sdy_hist_edge(start, stop, step, n_bins, k)) --k;
#pragma unroll
  for (int s = 0; s < 2; ++s)
    if (k < n_bins - 1 && x >= sdy_hist_edge(start, stop, step, n_bins, k + 1)) ++k;
  const bool settled = x >= sdy_hist_edge(start, stop, step, n_bins, k) &&
                       (k == n_bins - 1 || x < sdy_hist_edge(start, stop, step, n_bins, k + 1));
  if (!settled) {
    int lo = 0, hi = n_bins - 1;    // edge(0) = start <= x
    for (int s = 0; s < 16; ++s) {  // n_bins <= 2^16
      const int mid = (lo + hi + 1) >> 1;
      if (lo < hi) {
        if (x >= sdy_hist_edge(start, stop, step, n_bins, mid)) lo = mid; else hi = mid - 1;
      }
    }
    k = lo;
  }
  return k < 0 ? 0 : (k > n_bins - 1 ? n_bins - 1 : k);
}

struct SdyHistPlan {
  float start, stop;       // the range after this add (unchanged when flags != 0)
  int n_left, n_right;     // doublings to the left, then to the right
  unsigned flags;          // SDY_HIST_FLAG_RANGE
};

// DynamicHistogram.add's range rules (histogram.py:43-55) for one (vmin, vmax): widen a constant sample by +-1e-6, take the
// first sample's range as it is, otherwise double to the left while vmin < start, then to the right while vmax > stop.  Both
// loops stop at SDY_HIST_DOUBLING_CAP; a non-finite vmin / vmax, a cap that is hit (a zero-width range never grows) or a
// range the bins cannot stand on set `flags` = 1 and leave the range as it was.
SDY_HIST_HD SdyHistPlan sdy_hist_plan(float start, float stop, int initialised, float vmin, float vmax, int n_bins) {
#pragma clang fp contract(off)
  SdyHistPlan keep = {start, stop, 0, 0, 1u};
  if (!sdy_hist_finite(vmin) || !sdy_hist_finite(vmax) || vmin > vmax) return keep;
  if (vmin == vmax) {
    vmin = vmin - SDY_HIST_EPSILON;
    vmax = vmax + SDY_HIST_EPSILON;
  }
  SdyHistPlan p = {start, stop, 0, 0, 0u};
  if (!initialised) {
    p.start = vmin;
    p.stop = vmax;
  } else {
    while (vmin < p.start) {
      if (p.n_left == SDY_HIST_DOUBLING_CAP) return keep;
      const float range = p.stop - p.start;
      p.start = p.stop - 2.f * range;
      ++p.n_left;
    }
    while (vmax > p.stop) {
      if (p.n_right == SDY_HIST_DOUBLING_CAP) return keep;
      const float range = p.stop - p.start;
      p.stop = p.start + 2.f * range;
      ++p.n_right;
    }
  }
  return sdy_hist_range_ok(p.start, p.stop, n_bins) ? p : keep;
}

// Where old bin j lands after n_left doublings to the left and then n_right to the right: one doubling to the left sends j to
// n_bins/2 + j/2, one to the right to j/2 (histogram.py:63-99).  Either map reaches its fixed point (n_bins - 1, 0) within
// log2(n_bins) + 1 applications, so 17 of each are as good as any larger count (n_bins <= 2^16).
SDY_HIST_HD int sdy_hist_rebin(int j, int n_left, int n_right, int n_bins) {
  const int half = n_bins >> 1;
  n_left = n_left < 17 ? n_left : 17;
  n_right = n_right < 17 ? n_right : 17;
  for (int s = 0; s < n_left; ++s) j = half + (j >> 1);
  for (int s = 0; s < n_right; ++s) j >>= 1;
  return j;
}

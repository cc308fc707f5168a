// Per-grid-point video statistics and zonal means of the inference aggregators (VideoAggregator,
// src/ace_inference/core/aggregator/inference/video.py; ZonalMeanAggregator, .../zonal_mean.py), as ONE definition for the
// device kernels (field_stats.hip) and the host entry points sdy_video_accumulate_host / sdy_zonal_accumulate_host: what one
// grid point collects over the rows of one window time, and how that is folded into the float64 accumulators.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_FS_HD __host__ __device__ inline
#else
#define SDY_FS_HD inline
#endif

// One grid point at one window time.  Generated rows (i0, i1) are pooled; the error of row (i0, i1) is taken against target
// row i1: e = fl32(gen - target), the reference's single fp32 subtraction, widened to float64.  Everything else is float64.
// The variance of e is collected around the first row's e (a shift leaves a variance unchanged and keeps the one-pass form
// sum(d^2) - sum(d)^2 / n from cancelling when the error is mostly bias).  EXT = false collects the two means only.
template <bool EXT>
struct sdy_fs_point {
  double g, t;            // sums over the generated / the target rows
  double g2, t2;          // sums of squares
  double d, d2, e_ref;    // sums of (e - e_ref) and of its square; e_ref = e of the first row
  float emin, emax;
  int rows;               // generated rows so far
};

template <bool EXT>
SDY_FS_HD void sdy_fs_init(sdy_fs_point<EXT>& s) {
  s.g = s.t = s.g2 = s.t2 = s.d = s.d2 = s.e_ref = 0.0;
  s.emin = s.emax = 0.0f;
  s.rows = 0;
}

template <bool EXT>
SDY_FS_HD void sdy_fs_add_target(sdy_fs_point<EXT>& s, float tv) {
  const double x = (double)tv;
  s.t += x;
  if (EXT) s.t2 += x * x;
}

// min / max as torch's: a NaN wins
SDY_FS_HD float sdy_fs_min(float m, float x) { return (x < m || x != x) ? x : m; }
SDY_FS_HD float sdy_fs_max(float m, float x) { return (x > m || x != x) ? x : m; }
SDY_FS_HD double sdy_fs_min(double m, double x) { return (x < m || x != x) ? x : m; }
SDY_FS_HD double sdy_fs_max(double m, double x) { return (x > m || x != x) ? x : m; }

template <bool EXT>
SDY_FS_HD void sdy_fs_add_gen(sdy_fs_point<EXT>& s, float gv, float tv) {
  const double x = (double)gv;
  s.g += x;
  if (EXT) {
    s.g2 += x * x;
    const float e = gv - tv;
    if (s.rows == 0) {
      s.e_ref = (double)e;
      s.emin = s.emax = e;
    } else {
      s.emin = sdy_fs_min(s.emin, e);
      s.emax = sdy_fs_max(s.emax, e);
    }
    const double d = (double)e - s.e_ref;
    s.d += d;
    s.d2 += d * d;
  }
  s.rows += 1;
}

// unbiased variance of e over the rows; one row gives 0 / 0 = NaN, as torch.var of one sample does
template <bool EXT>
SDY_FS_HD double sdy_fs_err_var(const sdy_fs_point<EXT>& s) {
  const double n = (double)s.rows;
  const double v = (s.d2 - s.d * s.d / n) / (n - 1.0);
  return v < 0.0 ? 0.0 : v;
}

// fold one grid point into the accumulators at flat index `at`; n_gen / n_tgt = generated / target rows; a NULL accumulator
// is skipped.  Exactly one caller owns `at`: plain read-modify-write.
template <bool EXT>
SDY_FS_HD void sdy_fs_store(const sdy_fs_point<EXT>& s, long at, int n_gen, int n_tgt, double* gen_mean, double* target_mean,
                            double* gen_sq, double* target_sq, double* err_var, double* err_min, double* err_max) {
  gen_mean[at] += s.g / (double)n_gen;
  target_mean[at] += s.t / (double)n_tgt;
  if (EXT) {
    if (gen_sq) gen_sq[at] += s.g2 / (double)n_gen;
    if (target_sq) target_sq[at] += s.t2 / (double)n_tgt;
    if (err_var) err_var[at] += sdy_fs_err_var(s);
    if (err_min) err_min[at] = sdy_fs_min(err_min[at], (double)s.emin);
    if (err_max) err_max[at] = sdy_fs_max(err_max[at], (double)s.emax);
  }
}

// zonal mean of a latitude row from the float64 sum over members of the per-member sums over longitudes:
// mean over the n0 members of the mean over the W longitudes
SDY_FS_HD double sdy_fs_zonal_mean(double sum, int n0, int W) { return sum / (double)W / (double)n0; }

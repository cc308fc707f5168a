// Transient-eddy covariances of groups of variables at every grid point (no counterpart in the reference), as ONE definition for
// the device kernels (time_covariance.hip) and the host entry points sdy_time_covariance_*_host: what the state of a group gains
// from one counted time, what it gives at the end of a run, and what one grid point of one sample contributes to the six
// weighted sums of every pair.
//
// A group is an ordered set of K variables (2 <= K <= SDY_TC_MAX_K) on one grid.  One trajectory (a member of a sample, or a
// sample's target) at one grid point, counted times x_k,1 .. x_k,n (fp32) in run order:
//   c_k = x_k,1 (fp32), d_k,t = (double)x_k,t - (double)c_k, S_k = sum_t d_k,t, P_ij = sum_t d_i,t d_j,t for i <= j
// in the pair order (0,0), (0,1), .., (0,K-1), (1,1), ..  S and P are float64; every product is rounded once before it is added,
// and every time's term is added to the running value in ascending time, so the bits do not depend on how a run is cut into
// windows.  The shift by the first value keeps the covariance of fields with large means (T = 280 +- 3 K) to float64 rounding of
// the DEVIATIONS; unshifted sums of x y would lose seven digits of it.  A NaN in variable k reaches S_k and the P_ij with i == k
// or j == k of its trajectory and point, and nothing else.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_TC_HD __host__ __device__ inline
#else
#define SDY_TC_HD inline
#endif

constexpr int sdy_tc_pairs(int K) { return K * (K + 1) / 2; }
// the place of (i, j), i <= j, in the pair order
constexpr int sdy_tc_pair_index(int K, int i, int j) { return i * K - i * (i - 1) / 2 + (j - i); }

// the deviation of a value from the trajectory's origin: exact in float64 unless the two are more than 2^29 apart in exponent
SDY_TC_HD double sdy_tc_dev(float x, float c) { return (double)x - (double)c; }

// One counted time: d[k] the deviations of the K variables.  Products are rounded before they are added (nothing contracted).
template <int K>
SDY_TC_HD void sdy_tc_step(double (&s)[K], double (&p)[sdy_tc_pairs(K)], const double (&d)[K]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < K; ++i) s[i] = s[i] + d[i];
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int j = i; j < K; ++j) {
      const double dd = d[i] * d[j];
      p[sdy_tc_pair_index(K, i, j)] = p[sdy_tc_pair_index(K, i, j)] + dd;
    }
}

struct sdy_tc_moments {
  double cov;    // C_ij / n (population); on the diagonal C is clamped at 0
  double corr;   // C_ij / sqrt(V_i V_j), clamped to [-1, 1]; NaN unless n >= 2, V_i > 0 and V_j > 0
};

// sum_t (d_t - m)^2 = P - S m with m = S / n, clamped at 0 (not fmax: a NaN must stay one): sdy_tv_finish's rule
SDY_TC_HD double sdy_tc_V(double s, double pp, double n) {
#pragma clang fp contract(off)
  const double m = s / n;
  const double sm = s * m;
  const double v = pp - sm;
  return v < 0.0 ? 0.0 : v;
}

// End of a run, one pair i <= j: n counted times (n >= 1, an integer held as a double); si, sj the sums, pii, pjj, pij the
// products.  C_ij = P_ij - S_i m_j, always with the lower index as S; diagonal: i == j.
SDY_TC_HD sdy_tc_moments sdy_tc_finish(double si, double sj, double pii, double pjj, double pij, double n, bool diagonal) {
#pragma clang fp contract(off)
  sdy_tc_moments r;
  const double vi = sdy_tc_V(si, pii, n);
  const double vj = sdy_tc_V(sj, pjj, n);
  const double mj = sj / n;
  const double smj = si * mj;
  const double c = diagonal ? vi : pij - smj;
  r.cov = c / n;
  const double vv = vi * vj;
  double rho = c / sqrt(vv);
  if (rho > 1.0) rho = 1.0;                      // (comparisons, not fmin / fmax: a NaN must stay one)
  if (rho < -1.0) rho = -1.0;
  r.corr = (n >= 2.0 && vi > 0.0 && vj > 0.0) ? rho : (double)NAN;
  return r;
}

// the sums of one trajectory and grid point
template <int K>
struct sdy_tc_state {
  double s[K];
  double p[sdy_tc_pairs(K)];
};

template <int K>
SDY_TC_HD sdy_tc_moments sdy_tc_finish_pair(const sdy_tc_state<K>& st, int i, int j, double n) {
  return sdy_tc_finish(st.s[i], st.s[j], st.p[sdy_tc_pair_index(K, i, i)], st.p[sdy_tc_pair_index(K, j, j)],
                       st.p[sdy_tc_pair_index(K, i, j)], n, i == j);
}

// Slots of one pair's weighted sums.
enum {
  SDY_TC_COV_GEN = 0,     // sum_w mean_m cov_gen
  SDY_TC_COV_TARGET = 1,  // sum_w cov_target
  SDY_TC_COV_SQ = 2,      // sum_w (mean_m cov_gen - cov_target)^2
  SDY_TC_CORR_GEN = 3,    // over the mask: sum_w mean_m corr_gen
  SDY_TC_CORR_TARGET = 4, // over the mask: sum_w corr_target
  SDY_TC_CORR_W = 5,      // over the mask: sum_w
};

// One grid point of one sample, every pair of a group.  member(i) -> the sdy_tc_state<K> of member i (called once per member,
// in order: the state is read once), t the target's, w the area weight, n the counted times.  The mask of a pair: n >= 2, and
// the target and every member have a correlation that is not NaN.  emit(pair, slot, x) receives the point's term of every slot
// of every pair, each exactly once, pairs in pair order and slots in slot order (the device sums a slot over a wave inside emit,
// so every lane of a wave has to arrive with the same slot).  All float64, nothing contracted.
template <int K, class Member, class Emit>
SDY_TC_HD void sdy_tc_point(int M, double n, double w, const sdy_tc_state<K>& t, Member member, Emit emit) {
#pragma clang fp contract(off)
  constexpr int NP = sdy_tc_pairs(K);
  double sum_cov[NP], sum_corr[NP];
  bool defined[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    sum_cov[q] = sum_corr[q] = 0.0;
    defined[q] = n >= 2.0;
  }
  for (int m = 0; m < M; ++m) {
    const sdy_tc_state<K> g = member(m);
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int j = i; j < K; ++j) {
        const int q = sdy_tc_pair_index(K, i, j);
        const sdy_tc_moments r = sdy_tc_finish_pair<K>(g, i, j, n);
        sum_cov[q] += r.cov;
        sum_corr[q] += r.corr;                   // (NaN where undefined: not looked at below unless every member is defined)
        defined[q] = defined[q] && r.corr == r.corr;
      }
  }
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int j = i; j < K; ++j) {
      const int q = sdy_tc_pair_index(K, i, j);
      const sdy_tc_moments r = sdy_tc_finish_pair<K>(t, i, j, n);
      const bool ok = defined[q] && r.corr == r.corr;
      const double mean_cov = sum_cov[q] / (double)M;
      const double diff = mean_cov - r.cov;
      const double mean_corr = sum_corr[q] / (double)M;
      emit(q, SDY_TC_COV_GEN, w * mean_cov);
      emit(q, SDY_TC_COV_TARGET, w * r.cov);
      emit(q, SDY_TC_COV_SQ, w * (diff * diff));
      emit(q, SDY_TC_CORR_GEN, ok ? w * mean_corr : 0.0);
      emit(q, SDY_TC_CORR_TARGET, ok ? w * r.corr : 0.0);
      emit(q, SDY_TC_CORR_W, ok ? w : 0.0);
    }
}

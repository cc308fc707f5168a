// Rotational and divergent kinetic-energy spectra of a wind (sdy_vector_degree_power, include/sdy_amd.h), as ONE definition for
// the device kernel (vector_spectrum.hip) and the host entry point sdy_vector_degree_power_host: how the four products of the
// vector Legendre analysis combine into the spheroidal and toroidal coefficients, what one order adds to a row's E(l), and --
// through spectrum.h -- in which order the rows of one accumulator element meet.
//
// With V_theta = -v, V_lambda = u and A_D, A_M the analyses by the two tables (derivative, m / sin theta):
//   s(l,m) = A_D[V_theta] - i A_M[V_lambda] = -A_D[v] - i A_M[u]        (spheroidal: the divergent part)
//   t(l,m) = A_D[V_lambda] + i A_M[V_theta] =  A_D[u] - i A_M[v]        (toroidal: the rotational part)
//   E(l)   = 1/2 |x(l,0)|^2 + sum_{m = 1 .. min(l, mtr - 1)} |x(l,m)|^2   orders added in ascending m, starting from 0.0
//
// Everything is float64 and never contracted to FMA.  Each of the eight fp32 values is first multiplied by its own field's scale
// (exact for a power of two); a component of s or t is then one rounded sum of two such products, its square one more rounding,
// the sum of the two squares a third and the addition to the row's E(l) a fourth.  The halving of order 0 is exact.  The error
// spectra take the float64 difference of the generated row's s (t) and its target row's (one more rounding per component).
// Rows of one accumulator element meet as in spectrum.h: 256 slots, a butterfly, divided by the row count.
#pragma once

#include "spectrum.h"

struct sdy_vs_coef { double s_re, s_im, t_re, t_im; };

// (re, im) of A_D[u], A_D[v], A_M[u], A_M[v] of one row and order, su / sv the scales of its u and v fields
SDY_SP_HD sdy_vs_coef sdy_vs_combine(float du_re, float du_im, float dv_re, float dv_im, float mu_re, float mu_im, float mv_re,
                                     float mv_im, double su, double sv) {
#pragma clang fp contract(off)
  const double Du_re = (double)du_re * su, Du_im = (double)du_im * su, Mu_re = (double)mu_re * su, Mu_im = (double)mu_im * su;
  const double Dv_re = (double)dv_re * sv, Dv_im = (double)dv_im * sv, Mv_re = (double)mv_re * sv, Mv_im = (double)mv_im * sv;
  sdy_vs_coef c;
  c.s_re = Mu_im - Dv_re;       // -i (a + i b) = b - i a
  c.s_im = -Dv_im - Mu_re;
  c.t_re = Du_re + Mv_im;
  c.t_im = Du_im - Mv_re;
  return c;
}

// e + w_m (re^2 + im^2), w_0 = 1/2, w_m = 1 otherwise
SDY_SP_HD double sdy_vs_add(double e, double re, double im, int m) {
#pragma clang fp contract(off)
  const double q = re * re + im * im;
  return e + (m == 0 ? 0.5 * q : q);
}

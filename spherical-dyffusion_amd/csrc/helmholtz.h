// Vorticity, divergence, streamfunction and velocity potential of a wind from the products of the vector Legendre analysis
// (sdy_helmholtz_coefficients, include/sdy_amd.h), as ONE definition for the device kernel (helmholtz.hip) and the host entry
// point sdy_helmholtz_coefficients_host: what one output plane holds at (l, m) for one wind, which quads of fields of the output
// tensor an item of work owns, and which of them are exact zeros.
//
// s(l,m) and t(l,m) are sdy_vs_combine of vector_spectrum.h (float64, never contracted; the eight fp32 values times their
// field's scale first).  Output q takes part[q] (0: s, 1: t), multiplies both components by factor[q][l] in float64 and rounds
// ONCE to fp32:
//   out(l, m, ri, q * out_stride + i) = (float)(x_ri(l,m) * factor[q][l]),   x = s or t of wind i
// With the factors of sdy_helmholtz_factors_host that is, for a sphere of radius a and the wind V = grad chi + r x grad psi,
//   zeta = -sqrt(l (l + 1)) t / a    delta = -sqrt(l (l + 1)) s / a    psi = a t / sqrt(l (l + 1))    chi = a s / sqrt(l (l + 1))
// Exact zeros, whatever the inputs and the factors hold: row l = 0, every entry with m > l, and every field of `out` that no
// output names (the fields of a plane's last quad past its last wind, and whole quads between and behind the planes).
//
// Work is cut into items of one quad of fields at one (l, m): X = W + Z items per (l, m), W = ceil(n_winds / 4) wind quads (item
// w < W owns winds 4 w .. 4 w + 3 in every plane: eight 16-byte loads, 2 n_out 16-byte stores) and Z = out_fields / 4 - n_out W
// quads that no plane covers (item W + z stores two quads of zeros).  Field offsets and out_stride are multiples of four and
// out_stride >= 4 W, so a quad belongs to one plane or to none.
#pragma once

#include "vector_spectrum.h"

#define SDY_HH_MAX_OUT 4

// one component of one output: the product in float64, one rounding to fp32
SDY_SP_HD float sdy_hh_round(double x, double factor) {
#pragma clang fp contract(off)
  return (float)(x * factor);
}

// (re, im) of output plane `part` (0: s, 1: t) of the combined coefficients c
SDY_SP_HD void sdy_hh_plane(const sdy_vs_coef c, int part, double factor, float* re, float* im) {
  *re = sdy_hh_round(part ? c.t_re : c.s_re, factor);
  *im = sdy_hh_round(part ? c.t_im : c.s_im, factor);
}

// wind quads per (l, m)
SDY_SP_HD int sdy_hh_wind_quads(int n_winds) { return (n_winds + 3) / 4; }

// quads of `out` per (l, m) that no plane covers
SDY_SP_HD int sdy_hh_zero_quads(int out_fields, int n_out, int n_winds) {
  return out_fields / 4 - n_out * sdy_hh_wind_quads(n_winds);
}

// first field of the z-th uncovered quad: the gaps behind planes 0 .. n_out - 2 hold out_stride / 4 - W quads each, the rest
// lie behind the last plane
SDY_SP_HD int sdy_hh_zero_field(int z, int out_stride, int n_out, int n_winds) {
  const int W = sdy_hh_wind_quads(n_winds), gap = out_stride / 4 - W;
  const int q = (gap > 0 && z < (n_out - 1) * gap) ? z / gap : n_out - 1;
  const int before = q < n_out - 1 ? q * gap : (n_out - 1) * gap;
  return q * out_stride + 4 * (W + (z - before));
}

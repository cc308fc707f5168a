// Per-degree power of spherical-harmonic coefficients (sdy_degree_power, include/sdy_amd.h), as ONE definition for the device
// kernel (spectrum.hip) and the host entry point sdy_degree_power_host: what one coefficient adds to a row's P(l), in which
// order a row's orders are summed, and in which order the rows of one accumulator element meet.
//
//   P(l) = |a[l,0]|^2 + 2 * sum_{m = 1 .. min(l, mtr - 1)} |a[l,m]|^2      orders added in ascending m, starting from 0.0
//
// Everything is float64 and never contracted to FMA.  The square of an fp32 value is exact in float64, so a row's P(l) of the
// generated or the target coefficients carries one rounding per addition; the error spectrum squares the float64 difference of
// the two fp32 coefficients (one more rounding per product).
//
// Rows of one accumulator element: row r belongs to slot r % SDY_SP_SLOTS; a slot adds its rows' P(l) in ascending r, starting
// from 0.0; the slots meet in a butterfly over the slot number's bits in ascending order (slot s takes s ^ 1, then s ^ 2, ...,
// s ^ 128); the total is divided by the row count.  A row's own P(l) therefore depends on nothing but its coefficients, and an
// element's value on nothing but its rows' values and their order.  On the device a lane holds slots 4 * lane .. 4 * lane + 3.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_SP_HD __host__ __device__ inline
#else
#define SDY_SP_HD inline
#endif

#define SDY_SP_SLOTS 256

// s + w_m * ((sc re)^2 + (sc im)^2), w_0 = 1, w_m = 2 otherwise (the doubling is exact).  sc is the field's scale (1 without
// a scale array): what the stored coefficient has to be multiplied with; for a power of two the product is exact too.
SDY_SP_HD double sdy_sp_add(double s, float re, float im, double sc, int m) {
#pragma clang fp contract(off)
  const double a = (double)re * sc, b = (double)im * sc;
  const double q = a * a + b * b;
  return s + (m == 0 ? q : 2.0 * q);
}

// the same of the coefficient difference gen - target, subtracted in float64
SDY_SP_HD double sdy_sp_add_err(double s, float gre, float gim, double gsc, float tre, float tim, double tsc, int m) {
#pragma clang fp contract(off)
  const double a = (double)gre * gsc - (double)tre * tsc, b = (double)gim * gsc - (double)tim * tsc;
  const double q = a * a + b * b;
  return s + (m == 0 ? q : 2.0 * q);
}

// one lane's four slots, bits 0 and 1 of the butterfly
SDY_SP_HD double sdy_sp_fold4(double s0, double s1, double s2, double s3) {
#pragma clang fp contract(off)
  return (s0 + s1) + (s2 + s3);
}

// the whole butterfly on the host: x[0] is what every lane of the device's butterfly ends with
inline double sdy_sp_fold_slots(double* x) {
#pragma clang fp contract(off)
  for (int bit = 1; bit < SDY_SP_SLOTS; bit <<= 1)
    for (int s = 0; s < SDY_SP_SLOTS; s += 2 * bit) x[s] = x[s] + x[s + bit];
  return x[0];
}

SDY_SP_HD double sdy_sp_mean(double sum, int rows) { return sum / (double)rows; }

// Threshold events of an ensemble (Brier score, reliability, ROC, exceedance frequency), as ONE definition for the device
// kernels (event_verif.hip) and the host entry points sdy_event_table_accumulate_host / sdy_event_frequency_accumulate_host:
// when a value is in an event, when a point is counted, where a variable's map thresholds live and where a count lives in the
// accumulators.  Integers and comparisons only: nothing here rounds.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_EV_HD __host__ __device__ inline
#else
#define SDY_EV_HD inline
#endif

// x against the threshold c of an event: strictly above, or strictly below.  A NaN on either side compares false: a NaN value
// is never in the event.
SDY_EV_HD bool sdy_ev_in(float x, float c, bool below) { return below ? x < c : x > c; }

// The same test with the direction folded into the operands: with sign = sdy_ev_sign(below), x < c exactly when -x > -c (a
// sign flip is exact and keeps a NaN a NaN), so sdy_ev_in(x, c, below) == (sdy_ev_signed(x, sign) > sdy_ev_signed(c, sign)).
// The kernels flip a point's thresholds once and each member value once per event, and compare one way only.
SDY_EV_HD unsigned sdy_ev_sign(bool below) { return below ? 0x80000000u : 0u; }
SDY_EV_HD float sdy_ev_signed(float x, unsigned sign) {
  return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) ^ sign);
}

// 1 when x is not NaN, else 0 -- (x == x) without a comparison: |x|'s bits minus those of the first NaN are negative exactly
// for a number or an infinity.  The kernels take the NaN rules through it where a comparison's lane mask would have to be
// kept across a loop.
SDY_EV_HD unsigned sdy_ev_not_nan(float x) {
  return ((__builtin_bit_cast(unsigned, x) & 0x7FFFFFFFu) - 0x7F800001u) >> 31;
}

// a point is counted for an event when neither its target nor its threshold is NaN (a NaN in a threshold map masks the point)
SDY_EV_HD bool sdy_ev_counted(float y, float c) { return y == y && c == c; }

// The plane of `maps` that holds the threshold of event e of a variable: the variable's map events follow one another from
// plane map_first on, in event order (is_map: bit e set when event e has a map threshold).  Formed from arguments only.
SDY_EV_HD int sdy_ev_map_plane(int map_first, unsigned is_map, int e) {
  return map_first + __builtin_popcount(is_map & ((1u << e) - 1u));
}

// table[v, slot, e, lat, o, k] of the contiguous (nvars, n_slots, E, H, 2, M + 1) accumulator; the entry points bound the
// product below 2^50
SDY_EV_HD long sdy_ev_table_at(long v, long n_slots, long slot, long E, long e, long H, long lat, long M, long o, long k) {
  return (((((v * n_slots + slot) * E + e) * H + lat) * 2 + o) * (M + 1)) + k;
}

// maps[v, e, q, p] of the contiguous (nvars, E, 3, plane) accumulator: q = 0 member hits, 1 target hits, 2 counted points
SDY_EV_HD long sdy_ev_freq_at(long v, long E, long e, long q, long plane, long p) { return ((v * E + e) * 3 + q) * plane + p; }

// Neighbourhood verification of threshold events (fractions skill score), as ONE definition for the device kernels (fss.hip)
// and the host entry point sdy_fss_accumulate_host: the 16-bit code of a point, the neighbourhood of a centre, when a centre is
// counted, its six terms and where they live in the accumulators.  When a value is in an event and when a point is counted is
// events.h; nothing is restated here.  Integers and comparisons only: nothing here rounds.
#pragma once
#include "events.h"

#define SDY_FSS_HD SDY_EV_HD

// The code of a point for one event: k (the members in the event, 0 .. 64) in bits 0-6, o (the target in the event) in bit 7,
// c (the point is counted) in bit 8; 0 where the point is not counted, so that k and o are 0 there.
SDY_FSS_HD unsigned sdy_fss_code(unsigned k, unsigned o, unsigned c) { return (k | (o << 7) | (c << 8)) & (0u - c); }
SDY_FSS_HD unsigned sdy_fss_code_k(unsigned code) { return code & 127u; }
SDY_FSS_HD unsigned sdy_fss_code_o(unsigned code) { return (code >> 7) & 1u; }
SDY_FSS_HD unsigned sdy_fss_code_c(unsigned code) { return (code >> 8) & 1u; }

// A code spread for adding along a row: k in bits 0-15, o in bits 16-23, c in bits 24-31.  The sum of the 2r + 1 <= 255 words
// of a centre's row segment carries nowhere: sum k <= M (2r + 1) < 2^16, sum o and sum c <= 2r + 1 < 2^8 (M (2r + 1)^2 <= 65535).
SDY_FSS_HD unsigned sdy_fss_spread(unsigned code) {
  return sdy_fss_code_k(code) | (sdy_fss_code_o(code) << 16) | (sdy_fss_code_c(code) << 24);
}
SDY_FSS_HD unsigned sdy_fss_spread_k(unsigned w) { return w & 0xFFFFu; }
SDY_FSS_HD unsigned sdy_fss_spread_o(unsigned w) { return (w >> 16) & 0xFFu; }
SDY_FSS_HD unsigned sdy_fss_spread_c(unsigned w) { return w >> 24; }

// The rows lat' of the neighbourhood of radius r around latitude lat: clipped at the poles, the window does not cross them.
SDY_FSS_HD int sdy_fss_row_first(int lat, int r) { return lat - r > 0 ? lat - r : 0; }
SDY_FSS_HD int sdy_fss_row_last(int H, int lat, int r) { return lat + r < H - 1 ? lat + r : H - 1; }
// Longitude wraps: lon + d for |d| <= r < W, brought back into 0 .. W - 1
SDY_FSS_HD int sdy_fss_wrap(int lon, int W) { return lon < 0 ? lon + W : (lon >= W ? lon - W : lon); }
// n(lat, r): the grid points of the neighbourhood, a function of (lat, r) alone
SDY_FSS_HD unsigned sdy_fss_size(int H, int lat, int r) {
  return (unsigned)(2 * r + 1) * (unsigned)(sdy_fss_row_last(H, lat, r) - sdy_fss_row_first(lat, r) + 1);
}

// The six integers a row keeps, in accumulator order
enum { SDY_FSS_COUNT = 0, SDY_FSS_K = 1, SDY_FSS_O = 2, SDY_FSS_KK = 3, SDY_FSS_KO = 4, SDY_FSS_OO = 5, SDY_FSS_TERMS = 6 };

// What a centre with the box sums K, O, C adds to its row: nothing unless every point of its neighbourhood is counted.
// K <= 65535: K * K fits 32 bits unsigned, the sums are 64-bit.
SDY_FSS_HD void sdy_fss_add_centre(unsigned long long (&sum)[SDY_FSS_TERMS], unsigned K, unsigned O, unsigned C, unsigned n) {
  if (C != n) return;
  sum[SDY_FSS_COUNT] += 1ull;
  sum[SDY_FSS_K] += K;
  sum[SDY_FSS_O] += O;
  sum[SDY_FSS_KK] += (unsigned long long)K * K;
  sum[SDY_FSS_KO] += (unsigned long long)K * O;
  sum[SDY_FSS_OO] += (unsigned long long)O * O;
}

// acc[v, slot, e, j, lat, 0] of the contiguous (nvars, n_slots, E, R, H, 6) accumulator; the entry points bound the product
// below 2^50
SDY_FSS_HD long sdy_fss_at(long v, long n_slots, long slot, long E, long e, long R, long j, long H, long lat) {
  return (((((v * n_slots + slot) * E + e) * R + j) * H + lat) * SDY_FSS_TERMS);
}

// codes[v, s, t, e, 0] of the contiguous (nvars, n1, T, E, H*W) 16-bit workspace
SDY_FSS_HD long sdy_fss_code_at(long v, long n1, long s, long T, long t, long E, long e, long plane) {
  return (((v * n1 + s) * T + t) * E + e) * plane;
}

// Rank (Talagrand) histogram of an ensemble, as ONE definition for the device kernel (rank_hist.hip) and the host entry point
// sdy_rank_hist_accumulate_host: what one member adds to the two running counters of a grid point, whether the point is
// counted at all, and where a row's bins and tie count live in the accumulators.  Integers only: nothing here rounds.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_RH_HD __host__ __device__ inline
#else
#define SDY_RH_HD inline
#endif

// One member g against the target y of a grid point: `below` counts the members strictly below the target (the point's rank
// once every member has been seen, 0 .. M), `equal` is set once a member equals it (the point is a tie; ties do not move the
// rank).  A NaN on either side compares false both times: a NaN member is simply not below.
SDY_RH_HD void sdy_rh_member(int& below, int& equal, float g, float y) {
  below += g < y ? 1 : 0;
  equal |= g == y ? 1 : 0;
}

// a point whose target is NaN is counted nowhere
SDY_RH_HD bool sdy_rh_counted(float y) { return y == y; }

// Accumulator places of the row (variable v, slot, latitude lat): its M + 1 bins at counts[sdy_rh_row(...) * (M + 1) + rank],
// its tie count at ties[sdy_rh_row(...)].  The entry points bound nvars * n_slots * H * (M + 1) below 2^50.
SDY_RH_HD long sdy_rh_row(long v, long n_slots, long slot, long H, long lat) { return (v * n_slots + slot) * H + lat; }

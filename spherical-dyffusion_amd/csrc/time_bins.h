// Time sums and extremes per time bin (no counterpart in the reference) as ONE definition for the device kernel
// (time_bins.hip) and the host entry point sdy_binned_time_accumulate_host: what one accumulator element of one bin gains from
// one counted value, and where the groups of a call begin.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_TB_HD __host__ __device__ inline
#else
#define SDY_TB_HD inline
#endif

// The sum of one (bin, element) is one sequential float64 chain over its counted values in the order given: a widening and one
// float64 addition per value (nothing to contract), applied to the accumulator itself -- no partial sum of a window.
SDY_TB_HD double sdy_tb_add(double acc, float x) { return acc + (double)x; }

// The extremes: a value replaces the kept one when it compares beyond it, or when it is a NaN; a kept NaN stays (nothing
// compares beyond it, and only a NaN replaces it).  An empty bin keeps what the caller filled in: -inf / +inf.
SDY_TB_HD float sdy_tb_max(float kept, float x) { return (x > kept || x != x) ? x : kept; }
SDY_TB_HD float sdy_tb_min(float kept, float x) { return (x < kept || x != x) ? x : kept; }

// the first entry of group g in the list of times
template <class Args>
SDY_TB_HD int sdy_tb_group_begin(const Args& a, int g) { return g == 0 ? 0 : (int)a.group_end[g - 1]; }

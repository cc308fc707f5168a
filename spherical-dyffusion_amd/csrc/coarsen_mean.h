// Time coarsening of the inference loop's data writer (TimeCoarsen, src/ace_inference/inference/data_writer/time_coarsen.py:
// `unfold(dimension=time, size=f, step=f).mean(dim=-1)`), as ONE definition for the device kernel (coarsen.hip) and the host
// entry point sdy_time_coarsen_host.  Which input times an output time takes, and the arithmetic of a group.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDY_COARSEN_HD __host__ __device__ inline
#else
#define SDY_COARSEN_HD inline
#endif

// output times of T input times: the first t_first are kept, the rest form whole groups of `factor` (a tail is dropped)
SDY_COARSEN_HD int sdy_coarsen_t_out(int T, int t_first, int factor) { return t_first + (T - t_first) / factor; }

// output time `to` reads input times first .. first + count - 1
SDY_COARSEN_HD void sdy_coarsen_span(int to, int t_first, int factor, int* first, int* count) {
  if (to < t_first) {
    *first = to;
    *count = 1;
  } else {
    *first = t_first + (to - t_first) * factor;
    *count = factor;
  }
}

// Mean of a group: fp32 sum of load(0) .. load(count - 1) in time order, then a true division (sum / count, as torch's mean; no
// reciprocal).  A group of one is handed back untouched -- bit for bit, signed zeros and NaN payloads included.  V is float or
// a vector of floats.
template <class V, class Load>
SDY_COARSEN_HD V sdy_coarsen_group(Load&& load, int count) {
  V s = load(0);
  if (count == 1) return s;
  for (int k = 1; k < count; ++k) s = s + load(k);
  return s / (float)count;
}

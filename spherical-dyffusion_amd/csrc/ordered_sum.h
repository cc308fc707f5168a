// The ordered float64 sum of the aggregators, as ONE definition (corrector.hip, conservation.hip, member_mean.hip,
// variability.hip, region_series.hip, member_gram.hip).  "The same bits in any batch, load path and run" rests on every one of
// them adding in this tree and no other:
//   the 64 lanes of a wave by the xor butterfly 32, 16, 8, 4, 2, 1        sdy_wave_sum (device), sdy_wave_sum_host (its twin)
//   the waves of a block, ascending (then a chunk's quarters, ascending)  sdy_fold_rows
//   the chunks of a row, ascending, from 0.0                              sdy_sum_chunks, sdy_combine_chunks_launch
// Additions only: there is nothing for the compiler to contract.
#pragma once
#include "common.h"

// in place: every lane of the wave ends up with the sum; several values go through the masks side by side
template <class... D>
__device__ __forceinline__ void sdy_wave_sum(D&... x) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) ((x += __shfl_xor(x, m, 64)), ...);
}

// what lane 0 holds after sdy_wave_sum when lane i came with lane[i]: every lane adds its partner's value, mask after mask
inline double sdy_wave_sum_host(const double* lane) {
  double v[64], nxt[64];
  for (int i = 0; i < 64; ++i) v[i] = lane[i];
  for (int m = 32; m > 0; m >>= 1) {
    for (int i = 0; i < 64; ++i) nxt[i] = v[i] + v[i ^ m];
    for (int i = 0; i < 64; ++i) v[i] = nxt[i];
  }
  return v[0];
}

// rows[0][k] + rows[1][k] + ...: what lane 0 of every wave (or every quarter of a chunk) left for slot k
template <int N, int S>
__device__ __forceinline__ double sdy_fold_rows(const double (&rows)[N][S], int k) {
  double s = rows[0][k];
#pragma unroll
  for (int r = 1; r < N; ++r) s += rows[r][k];
  return s;
}

// chunk c's partial of element k at partials[c * stride + k].  s[j] <- element k + j: N neighbouring elements side by side in
// one pass over the chunks, each in the same order as alone (a thread that adds them one after the other waits for every load
// N times over: NOTEBOOK.md 7w)
template <int N>
__host__ __device__ inline void sdy_sum_chunks(const double* partials, int chunks, long stride, long k, double (&s)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) s[j] = 0.0;
  for (int c = 0; c < chunks; ++c)
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] += partials[(long)c * stride + k + j];
}
__host__ __device__ inline double sdy_sum_chunks(const double* partials, int chunks, long stride, long k) {
  double s[1];
  sdy_sum_chunks(partials, chunks, stride, k, s);
  return s[0];
}

// out (groups, stride) <- partials (groups, chunks, stride), one thread per element of out, sdy_sum_chunks each
// (ordered_sum.hip).  The caller has checked the pointers and bounded the flat indices (groups * chunks * stride below 2^50;
// stride is a slot or entry count of a few thousand at most: ceil(stride / 256) blocks per group).
int sdy_combine_chunks_launch(const double* partials, long groups, int chunks, long stride, double* out, hipStream_t stream);

// a workspace of at least `need` bytes that takes 8-byte accesses
inline bool sdy_ws_ok(const void* ws, size_t ws_bytes, size_t need) {
  return ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= need;
}

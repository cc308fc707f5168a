// The combine launch of the aggregators (ordered_sum.h): a row's chunks in ascending order -> out.
#include "ordered_sum.h"

namespace {

constexpr int kThreads = 256;

// grid (groups, ceil(stride / kThreads)): one thread per element of out (groups, stride); partials (groups, chunks, stride).
// A group's elements have blocks of their own, however few they are: the loads of a wave stay inside one group's partials.
// (A block takes a second group only past 2^31 - 1 of them.)
__global__ __launch_bounds__(kThreads) void combine_chunks_kernel(const double* partials, long groups, int chunks, long stride,
                                                                  double* out) {
  const long k = (long)blockIdx.y * kThreads + threadIdx.x;
  if (k >= stride) return;
  for (long g = blockIdx.x; g < groups; g += gridDim.x)
    out[g * stride + k] = sdy_sum_chunks(partials + g * chunks * stride, chunks, stride, k);
}

}  // namespace

int sdy_combine_chunks_launch(const double* partials, long groups, int chunks, long stride, double* out, hipStream_t stream) {
  const dim3 grid((unsigned)(groups < 0x7fffffffL ? groups : 0x7fffffffL), (unsigned)((stride + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(combine_chunks_kernel, grid, dim3(kThreads), 0, stream, partials, groups, chunks, stride, out);
  return sdy_launch_status();
}

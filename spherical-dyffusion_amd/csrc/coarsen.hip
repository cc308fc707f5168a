// Time coarsening of the inference loop's data writer (TimeCoarsen, src/ace_inference/inference/data_writer/time_coarsen.py),
// gfx950: all variables of one dict in one launch, read in place through the strided views the window driver hands over,
// written contiguously.  HBM-bound streaming: every input element of a kept group is read once, every output written once; no
// LDS, no atomics.  With factor 1 the same kernel is the gather that packs a dict into one staging buffer.  The arithmetic of
// a group is coarsen_mean.h.
#include "common.h"
#include "coarsen_mean.h"
#include "window.h"

namespace {

constexpr int kItemsPerBlock = 512;     // 256 threads x 2 work items in flight per thread
constexpr int kBlocksPerLaunch = 4096;  // over all variables; a variable with more work strides over its items

// two work items of one thread as one value: sdy_coarsen_group sums both chains side by side (two loads in flight per step)
template <class V>
struct Two {
  V a, b;
};
template <class V>
__device__ __forceinline__ Two<V> operator+(Two<V> x, Two<V> y) { return {x.a + y.a, x.b + y.b}; }
template <class V>
__device__ __forceinline__ Two<V> operator/(Two<V> x, float d) { return {x.a / d, x.b / d}; }

// idx / d and idx % d for a 64-bit flat index: almost every launch stays below 2^32, where the division is a 32-bit one
__device__ __forceinline__ void divmod(unsigned long idx, unsigned d, unsigned long* q, unsigned* r) {
  if ((idx >> 32) == 0) {
    const unsigned lo = (unsigned)idx;
    *q = lo / d;
    *r = lo % d;
  } else {
    *q = idx / d;
    *r = (unsigned)(idx % d);
  }
}

struct Item {
  const float* src;   // first input time of the group, at the item's grid point(s)
  float* dst;
  int count;
};

// work item idx of variable v: W floats (4 or 1) at grid point W * q of output time `to` of row (i0, i1);
// idx = (row * T_out + to) * (HW / W) + q, so consecutive lanes touch consecutive addresses on both sides
template <int W>
__device__ __forceinline__ Item item_of(const sdy_coarsen_args& a, int v, unsigned long idx, int T_out, unsigned per_time) {
  unsigned long row_time, row;
  unsigned q, to;
  divmod(idx, per_time, &row_time, &q);
  divmod(row_time, (unsigned)T_out, &row, &to);
  const unsigned long i0 = row / (unsigned)a.n1, i1 = row - i0 * (unsigned)a.n1;   // rows < 2^31 (checked by the entry point)
  int first, count;
  sdy_coarsen_span((int)to, a.t_first, a.factor, &first, &count);
  Item it;
  it.src = a.data[v] + (long)i0 * a.s0[v] + (long)i1 * a.s1[v] + (long)first * a.HW + (long)q * W;
  it.dst = a.out[v] + (long)row_time * a.HW + (long)q * W;
  it.count = count;
  return it;
}

template <bool VEC>
__global__ __launch_bounds__(256) void time_coarsen_kernel(const sdy_coarsen_args a, int T_out, unsigned long n_items) {
  constexpr int W = VEC ? 4 : 1;
  using V = std::conditional_t<VEC, f32x4, float>;
  const int v = blockIdx.y;
  const unsigned per_time = (unsigned)(a.HW / W);
  const long HW = a.HW;
  for (unsigned long base = (unsigned long)blockIdx.x * kItemsPerBlock + threadIdx.x; base < n_items;
       base += (unsigned long)gridDim.x * kItemsPerBlock) {
    const unsigned long second = base + 256;
    const bool two = second < n_items;
    const Item A = item_of<W>(a, v, base, T_out, per_time);
    const Item B = item_of<W>(a, v, two ? second : base, T_out, per_time);   // (no second item: the first again, not stored)
    if (A.count == B.count) {
      const Two<V> r = sdy_coarsen_group<Two<V>>(
          [&](int k) { return Two<V>{*reinterpret_cast<const V*>(A.src + k * HW), *reinterpret_cast<const V*>(B.src + k * HW)}; },
          A.count);
      *reinterpret_cast<V*>(A.dst) = r.a;
      if (two) *reinterpret_cast<V*>(B.dst) = r.b;
    } else {   // one item in the copied initial times, the other in a group
      *reinterpret_cast<V*>(A.dst) =
          sdy_coarsen_group<V>([&](int k) { return *reinterpret_cast<const V*>(A.src + k * HW); }, A.count);
      *reinterpret_cast<V*>(B.dst) =
          sdy_coarsen_group<V>([&](int k) { return *reinterpret_cast<const V*>(B.src + k * HW); }, B.count);
    }
  }
}

// everything that bounds an address, for the device and the host entry point alike; *T_out on success
int check_args(const sdy_coarsen_args* a, int* T_out) {
  if (!a || a->nvars < 1 || a->nvars > SDY_MAX_VARS) return SDY_ERR_ARG;
  if (a->n0 < 1 || a->n1 < 1 || a->T < 1 || a->HW < 1 || a->factor < 1) return SDY_ERR_ARG;
  if (a->t_first < 0 || a->t_first > a->T) return SDY_ERR_ARG;
  for (int v = 0; v < a->nvars; ++v)
    if (!a->data[v] || !a->out[v] || a->s0[v] < 0 || a->s1[v] < 0) return SDY_ERR_ARG;
  *T_out = sdy_coarsen_t_out(a->T, a->t_first, a->factor);
  if (*T_out < 1) return SDY_ERR_ARG;
  // 32-bit grid points within a row's times, 32-bit row numbers; the flat work index itself is 64-bit
  if ((long)a->T * a->HW > (1L << 30) || (long)a->n0 * a->n1 >= (1L << 31)) return SDY_ERR_UNSUPPORTED;
  return SDY_OK;
}

}  // namespace

extern "C" int sdy_time_coarsen_host(const sdy_coarsen_args* a) {
  int T_out = 0;
  SDY_TRY(check_args(a, &T_out));
  const long HW = a->HW;
  for (int v = 0; v < a->nvars; ++v)
    for (long row = 0; row < (long)a->n0 * a->n1; ++row) {
      const long i0 = row / a->n1, i1 = row - i0 * a->n1;
      const float* in = a->data[v] + i0 * a->s0[v] + i1 * a->s1[v];
      float* out = a->out[v] + row * T_out * HW;
      for (int to = 0; to < T_out; ++to) {
        int first, count;
        sdy_coarsen_span(to, a->t_first, a->factor, &first, &count);
        for (long p = 0; p < HW; ++p) {
          const float* src = in + first * HW + p;
          out[to * HW + p] = sdy_coarsen_group<float>([&](int k) { return src[k * HW]; }, count);
        }
      }
    }
  return SDY_OK;
}

extern "C" int sdy_time_coarsen(const sdy_coarsen_args* a, void* stream) {
  int T_out = 0;
  SDY_TRY(check_args(a, &T_out));
  bool vec = (a->HW & 3) == 0;
  for (int v = 0; v < a->nvars; ++v)
    vec = vec && (((uintptr_t)a->data[v] | (uintptr_t)a->out[v]) & 15) == 0 && (a->s0[v] & 3) == 0 && (a->s1[v] & 3) == 0;
  const unsigned long n_items = (unsigned long)a->n0 * a->n1 * T_out * (vec ? a->HW / 4 : a->HW);
  const dim3 grid(sdy_grid_cap((n_items + kItemsPerBlock - 1) / kItemsPerBlock, a->nvars, kBlocksPerLaunch, 32), a->nvars);
  if (vec)
    hipLaunchKernelGGL(time_coarsen_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *a, T_out, n_items);
  else
    hipLaunchKernelGGL(time_coarsen_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *a, T_out, n_items);
  return sdy_launch_status();
}

// Per-variable, per-lead-time value histograms of the inference loop's data writer (HistogramDataWriter,
// src/ace_inference/inference/data_writer/histograms.py; DynamicHistogram, src/ace_inference/core/histogram.py), gfx950.
// Three launches per dict, all variables at once: min / max, range doubling, counting.  The range, the counts and the
// bookkeeping live on the device; the host reads them when it wants the result.  The edge arithmetic is hist_edges.h.
#include "common.h"
#include "hist_edges.h"

namespace {

// state of one variable: SDY_HIST_STATE_WORDS 32-bit words (zeroed = "nothing added yet")
enum { ST_START = 0, ST_STOP = 1, ST_INIT = 2, ST_FLAGS = 3, ST_OUTSIDE = 4 /* and 5: one 64-bit counter */, ST_MAX = 6, ST_MIN = 7 };
constexpr int kStateWords = 8;

constexpr int kMinMaxChunk = 16384;   // floats of one row a block of the min / max pass reads
constexpr int kCountChunk = 32768;    // values a block of the counting pass bins before it flushes (far below 2^32 per bin)

// order-preserving map of fp32 onto unsigned: key(a) < key(b) <=> a < b (-0 below +0, NaNs outside the infinities).
// ST_MAX holds the largest key seen, ST_MIN the largest COMPLEMENT of a key: both grow from the zeroed state by atomicMax.
__host__ __device__ __forceinline__ unsigned key_of(float x) {
  unsigned b;
  __builtin_memcpy(&b, &x, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float float_of(unsigned key) {
  const unsigned b = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
  float x;
  __builtin_memcpy(&x, &b, 4);
  return x;
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// blockIdx.x = row * chunks_per_row + chunk; row (i0, i1) of variable v starts at data[v] + i0*s0 + i1*s1
__device__ __forceinline__ const float* row_base(const sdy_hist_args& a, int v, int row) {
  const int i0 = row / a.n1, i1 = row - i0 * a.n1;
  return a.data[v] + (long)i0 * a.s0[v] + (long)i1 * a.s1[v];
}

// ---- 1. min / max of every variable: T*HW contiguous floats per row, block reduce, two atomics per block
template <bool VEC>
__global__ __launch_bounds__(256) void hist_minmax_kernel(const sdy_hist_args a, int chunks_per_row, int chunk) {
  __shared__ unsigned s_max, s_min;
  const int v = blockIdx.y, tid = threadIdx.x;
  const int row = blockIdx.x / chunks_per_row, c = blockIdx.x - row * chunks_per_row;
  const float* base = row_base(a, v, row);
  const int L = a.T * a.HW, begin = c * chunk, end = min(L, begin + chunk);
  if (tid == 0) s_max = s_min = 0u;
  __syncthreads();
  unsigned kmax = 0u, cmax = 0u;
  if (VEC) {
    for (int j = begin + tid * 4; j < end; j += 1024) {       // chunk, L multiples of 4: j + 3 < end
      const f32x4 x = *reinterpret_cast<const f32x4*>(base + j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned k = key_of(x[e]);
        kmax = k > kmax ? k : kmax;
        cmax = ~k > cmax ? ~k : cmax;
      }
    }
  } else {
    for (int j = begin + tid; j < end; j += 256) {
      const unsigned k = key_of(base[j]);
      kmax = k > kmax ? k : kmax;
      cmax = ~k > cmax ? ~k : cmax;
    }
  }
  kmax = wave_max(kmax);
  cmax = wave_max(cmax);
  if ((tid & 63) == 0) {
    atomicMax(&s_max, kmax);
    atomicMax(&s_min, cmax);
  }
  __syncthreads();
  if (tid == 0 && begin < end) {
    unsigned* st = reinterpret_cast<unsigned*>(a.state) + v * kStateWords;
    atomicMax(st + ST_MAX, s_max);
    atomicMax(st + ST_MIN, s_min);
  }
}

// ---- 2. range rules and the doubling of the counts: one workgroup per variable
__global__ __launch_bounds__(256) void hist_rebin_kernel(unsigned* state, unsigned long long* counts, int n_times, int n_bins) {
  extern __shared__ unsigned long long s_row[];
  __shared__ int s_left, s_right, s_go;
  const int v = blockIdx.x, tid = threadIdx.x;
  unsigned* st = state + v * kStateWords;
  if (tid == 0) {
    const float vmax = float_of(st[ST_MAX]), vmin = float_of(~st[ST_MIN]);
    const SdyHistPlan p = sdy_hist_plan(__uint_as_float(st[ST_START]), __uint_as_float(st[ST_STOP]), (int)st[ST_INIT], vmin, vmax,
                                        n_bins);
    if (p.flags) {
      st[ST_FLAGS] |= p.flags;
    } else {
      st[ST_START] = __float_as_uint(p.start);
      st[ST_STOP] = __float_as_uint(p.stop);
      st[ST_INIT] = 1u;
    }
    st[ST_MAX] = 0u;
    st[ST_MIN] = 0u;
    s_left = p.n_left;
    s_right = p.n_right;
    s_go = !p.flags && (p.n_left + p.n_right) > 0;
  }
  __syncthreads();
  if (!s_go) return;
  const int n_left = s_left, n_right = s_right;
  for (int t = 0; t < n_times; ++t) {
    unsigned long long* c = counts + ((long)v * n_times + t) * n_bins;
    for (int b = tid; b < n_bins; b += 256) s_row[b] = 0ull;
    __syncthreads();
    for (int b = tid; b < n_bins; b += 256) {
      const unsigned long long n = c[b];
      int k = sdy_hist_rebin(b, n_left, n_right, n_bins);
      k = k < 0 ? 0 : (k > n_bins - 1 ? n_bins - 1 : k);
      if (n) atomicAdd(&s_row[k], n);
    }
    __syncthreads();
    for (int b = tid; b < n_bins; b += 256) c[b] = s_row[b];
    __syncthreads();
  }
}

// ---- 3. counting: grid (row x chunk of HW, variable, time); one uint32 histogram per wave in LDS, flushed to the 64-bit
// counts with one atomic per non-empty bin and block.  Integer adds: the result does not depend on any order.
template <bool VEC>
__global__ __launch_bounds__(256) void hist_count_kernel(const sdy_hist_args a, int chunks_per_row, int chunk) {
  extern __shared__ unsigned s_hist[];          // 4 x n_bins
  __shared__ unsigned s_outside;
  const int v = blockIdx.y, t = blockIdx.z, tid = threadIdx.x, n_bins = a.n_bins;
  const int row = blockIdx.x / chunks_per_row, c = blockIdx.x - row * chunks_per_row;
  const float* base = row_base(a, v, row) + (long)t * a.HW;
  const int begin = c * chunk, end = min(a.HW, begin + chunk);
  unsigned* st = reinterpret_cast<unsigned*>(a.state) + v * kStateWords;
  // a variable whose very first range was refused has no bins: every value counts as outside
  const bool ready = st[ST_INIT] != 0u;
  const float start = ready ? __uint_as_float(st[ST_START]) : __builtin_nanf("");
  const float stop = ready ? __uint_as_float(st[ST_STOP]) : __builtin_nanf("");
  const float step = sdy_hist_step(start, stop, n_bins), inv_step = 1.f / step;
  for (int b = tid; b < 4 * n_bins; b += 256) s_hist[b] = 0u;
  if (tid == 0) s_outside = 0u;
  __syncthreads();
  unsigned* h = s_hist + (tid >> 6) * n_bins;
  unsigned outside = 0u;
  auto add = [&](int k, unsigned n) {           // k is -1 or inside [0, n_bins): sdy_hist_bin clamps
    if (k >= 0) atomicAdd(h + k, n); else outside += n;
  };
  if (VEC) {
    for (int j = begin + tid * 4; j < end; j += 1024) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(base + j);
      // neighbouring grid points mostly share a bin: one LDS atomic per run of equal bins
      int prev = sdy_hist_bin(x[0], start, stop, step, inv_step, n_bins);
      unsigned n = 1u;
#pragma unroll
      for (int e = 1; e < 4; ++e) {
        const int k = sdy_hist_bin(x[e], start, stop, step, inv_step, n_bins);
        if (k == prev) {
          ++n;
        } else {
          add(prev, n);
          prev = k;
          n = 1u;
        }
      }
      add(prev, n);
    }
  } else {
    for (int j = begin + tid; j < end; j += 256) add(sdy_hist_bin(base[j], start, stop, step, inv_step, n_bins), 1u);
  }
  outside = wave_sum(outside);
  if ((tid & 63) == 0 && outside) atomicAdd(&s_outside, outside);
  __syncthreads();
  unsigned long long* dst = a.counts + ((long)v * a.n_times + a.t_start + t) * n_bins;
  for (int b = tid; b < n_bins; b += 256) {
    const unsigned n = s_hist[b] + s_hist[n_bins + b] + s_hist[2 * n_bins + b] + s_hist[3 * n_bins + b];
    if (n) atomicAdd(dst + b, (unsigned long long)n);
  }
  if (tid == 0 && s_outside)
    atomicAdd(reinterpret_cast<unsigned long long*>(st + ST_OUTSIDE), (unsigned long long)s_outside);
}

// rows are cut into equal chunks of at most `cap` values, each a multiple of 4
void chunking(int len, int cap, int* per_row, int* chunk) {
  *per_row = (len + cap - 1) / cap;
  *chunk = ((len + *per_row - 1) / *per_row + 3) & ~3;
}

}  // namespace

extern "C" size_t sdy_hist_state_bytes(int nvars) { return nvars > 0 ? (size_t)nvars * kStateWords * 4 : 0; }

extern "C" int sdy_hist_state_unpack_host(const void* state_host, int v, float* start, float* stop, int* initialised,
                                          unsigned* flags, unsigned long long* outside) {
  if (!state_host || v < 0) return SDY_ERR_ARG;
  const unsigned* st = reinterpret_cast<const unsigned*>(state_host) + (size_t)v * kStateWords;
  if (start) __builtin_memcpy(start, st + ST_START, 4);
  if (stop) __builtin_memcpy(stop, st + ST_STOP, 4);
  if (initialised) *initialised = (int)st[ST_INIT];
  if (flags) *flags = st[ST_FLAGS];
  if (outside) __builtin_memcpy(outside, st + ST_OUTSIDE, 8);
  return SDY_OK;
}

extern "C" int sdy_hist_plan_host(float start, float stop, int initialised, float vmin, float vmax, int n_bins, float* new_start,
                                  float* new_stop, int* n_left, int* n_right, unsigned* flags) {
  if (n_bins < 2 || (n_bins & 1) || n_bins > SDY_HIST_MAX_BINS || !new_start || !new_stop || !n_left || !n_right || !flags)
    return SDY_ERR_ARG;
  const SdyHistPlan p = sdy_hist_plan(start, stop, initialised, vmin, vmax, n_bins);
  *new_start = p.start;
  *new_stop = p.stop;
  *n_left = p.n_left;
  *n_right = p.n_right;
  *flags = p.flags;
  return SDY_OK;
}

extern "C" int sdy_hist_edges_host(float start, float stop, int n_bins, float* edges) {
  if (n_bins < 1 || n_bins > SDY_HIST_MAX_BINS || !edges) return SDY_ERR_ARG;
  const float step = sdy_hist_step(start, stop, n_bins);
  for (int i = 0; i <= n_bins; ++i) edges[i] = sdy_hist_edge(start, stop, step, n_bins, i);
  return SDY_OK;
}

extern "C" int sdy_hist_bins_host(const float* x, long n, float start, float stop, int n_bins, int* bins) {
  if (!x || !bins || n < 0 || n_bins < 1 || n_bins > SDY_HIST_MAX_BINS) return SDY_ERR_ARG;
  const float step = sdy_hist_step(start, stop, n_bins), inv_step = 1.f / step;
  for (long i = 0; i < n; ++i) bins[i] = sdy_hist_bin(x[i], start, stop, step, inv_step, n_bins);
  return SDY_OK;
}

extern "C" int sdy_hist_add(const sdy_hist_args* a, void* stream) {
  // everything that bounds an address is checked here, before anything is launched
  if (!a || a->nvars < 1 || a->nvars > SDY_MAX_VARS || !a->state || !a->counts) return SDY_ERR_ARG;
  if (a->n0 < 1 || a->n1 < 1 || a->T < 1 || a->HW < 1 || a->n_times < 1) return SDY_ERR_ARG;
  if (a->t_start < 0 || (long)a->t_start + a->T > a->n_times) return SDY_ERR_ARG;
  if (a->n_bins < 2 || (a->n_bins & 1) || a->n_bins > SDY_HIST_MAX_BINS) return SDY_ERR_ARG;
  bool vec = (a->HW & 3) == 0;
  for (int v = 0; v < a->nvars; ++v) {
    if (!a->data[v] || a->s0[v] < 0 || a->s1[v] < 0) return SDY_ERR_ARG;
    vec = vec && ((uintptr_t)a->data[v] & 15) == 0 && (a->s0[v] & 3) == 0 && (a->s1[v] & 3) == 0;
  }
  const long rows = (long)a->n0 * a->n1, L = (long)a->T * a->HW;
  if (L > (1L << 30) || a->T > 65535) return SDY_ERR_UNSUPPORTED;   // 32-bit element indices within a row, grid.z
  int mm_per_row, mm_chunk, ct_per_row, ct_chunk;
  chunking((int)L, kMinMaxChunk, &mm_per_row, &mm_chunk);
  chunking(a->HW, kCountChunk, &ct_per_row, &ct_chunk);
  if (rows * mm_per_row >= (1L << 31) || rows * ct_per_row >= (1L << 31)) return SDY_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(256);
  const dim3 mm_grid((unsigned)(rows * mm_per_row), a->nvars), ct_grid((unsigned)(rows * ct_per_row), a->nvars, a->T);
  const size_t count_lds = (size_t)4 * a->n_bins * sizeof(unsigned), rebin_lds = (size_t)a->n_bins * sizeof(unsigned long long);
  if (vec)
    hipLaunchKernelGGL(hist_minmax_kernel<true>, mm_grid, block, 0, s, *a, mm_per_row, mm_chunk);
  else
    hipLaunchKernelGGL(hist_minmax_kernel<false>, mm_grid, block, 0, s, *a, mm_per_row, mm_chunk);
  SDY_TRY(sdy_launch_status());
  hipLaunchKernelGGL(hist_rebin_kernel, dim3(a->nvars), block, rebin_lds, s, reinterpret_cast<unsigned*>(a->state), a->counts,
                     a->n_times, a->n_bins);
  SDY_TRY(sdy_launch_status());
  if (vec)
    hipLaunchKernelGGL(hist_count_kernel<true>, ct_grid, block, count_lds, s, *a, ct_per_row, ct_chunk);
  else
    hipLaunchKernelGGL(hist_count_kernel<false>, ct_grid, block, count_lds, s, *a, ct_per_row, ct_chunk);
  return sdy_launch_status();
}

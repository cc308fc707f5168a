// The area-weighted Gram matrix of the member errors and the truth anomaly (sdy_member_gram, include/sdy_amd.h), gfx950: the
// (M + 2) x (M + 2) x HW float64 contraction behind the energy score, the field distances and the anomaly correlation, all
// variables of one window in one launch, on v_mfma_f64_16x16x4_f64.
//   member_gram_kernel<NB, W>: one block per (variable, sample, time, chunk of SDY_GRAM_CHUNK grid points), one quarter of the
//     chunk (256 points) after the other.  Stage: the quarter's M member rows (16-byte loads where the window allows them),
//     the target, the weights and the climatology go to LDS as fp32.  Contract: wave k takes points 64 k .. 64 k + 63 of the
//     quarter, four at a time.  For row block I lane l forms a_i (member_gram.h) of row i = 16 I + (l & 15) at point 4 q +
//     (l >> 4) from LDS; A operand w a_i, B operand a_j: for a diagonal tile both come from the same LDS word.  The NB (NB +
//     1) / 2 upper tiles are compile-time-indexed accumulators that live through the four quarters.  The LDS row stride is 260
//     words: the 16 rows x 4 points of a fragment read fall into 64 different banks.  Last: the waves' tiles are added in wave
//     order through LDS, and wave 0 writes the chunk's packed triangle to ws.
//     C/D of the f64 instruction: col = lane & 15, row = (lane >> 4) + 4 * reg (NOT the f32 map).
//   combine_chunks_kernel (ordered_sum.hip): a plane's chunks in ascending order -> out.
// No atomics; what a block adds, and in which order, depends on its plane, the weights and the climatology alone.
#include <vector>

#include "common.h"
#include "member_gram.h"
#include "ordered_sum.h"
#include "window.h"

namespace {

constexpr int kThreads = SDY_GRAM_QUARTER;                 // 256: one thread per grid point of a quarter when staging
constexpr int kWaves = kThreads / 64;
constexpr int kMaxMembers = SDY_GRAM_MAX_MEMBERS;
constexpr int kStride = SDY_GRAM_QUARTER + 4;              // LDS words per staged row: row * 260 + point, 16 x 4 -> 64 banks
constexpr int kSteps = SDY_GRAM_WAVE_POINTS / SDY_GRAM_STEP;   // matrix instructions per tile, wave and quarter
static_assert(kWaves == SDY_GRAM_WAVES && kSteps * SDY_GRAM_STEP * kWaves == SDY_GRAM_QUARTER, "the partition of member_gram.h");

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int tiles_of(int nb) { return nb * (nb + 1) / 2; }
constexpr int tile_at(int I, int J, int nb) { return I * nb - I * (I - 1) / 2 + (J - I); }

// dynamic LDS: the staged rows (M members and the target), or the tiles of one wave on their way to wave 0
inline size_t lds_bytes(int M, int nb) {
  const size_t rows = (size_t)(M + 1) * kStride * sizeof(float), red = (size_t)tiles_of(nb) * 256 * sizeof(double);
  return rows > red ? rows : red;
}

// Block blockIdx.x of variable blockIdx.y: chunk = x % chunks of plane x / chunks = sample * T + time.  Every index is bounded
// by the entry point: x < 2^31, a point p < HW before any global access (HW % 4 == 0 on the 16-byte path, so 4 points are
// inside or outside together), partial indices < 2^50.  LDS: a point past the plane has weight 0 and is never looked at.
template <int NB, int W>
__global__ __launch_bounds__(kThreads) void member_gram_kernel(const sdy_member_gram_args a, int chunks, double* partials) {
  extern __shared__ __align__(16) float sh_x[];            // [M + 1][kStride]: the members' rows, then the target's
  __shared__ float sh_w[SDY_GRAM_QUARTER], sh_c[SDY_GRAM_QUARTER];
  const int v = blockIdx.y, M = a.win.n0, T = a.win.T, N = M + 2;
  const long HW = a.HW;
  const int chunk = blockIdx.x % chunks, plane = blockIdx.x / chunks;
  const int s = plane / T, t = plane - s * T;
  const float* gen = a.win.gen[v] + (long)s * a.win.gs1 + (long)t * HW;
  const float* tgt = a.win.target[v] + (long)s * a.win.ts1 + (long)t * HW;
  const float* clim = a.climatology[v];
  const long gs0 = a.win.gs0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frag_row = lane & 15, frag_pt = lane >> 4;

  f64x4 acc[tiles_of(NB)];
  sdy_static_for<0, tiles_of(NB)>([&](auto k) { acc[k.value] = f64x4{0.0, 0.0, 0.0, 0.0}; });
  // the LDS row of vector i: member i - 1, or the target's (whose value sdy_gram_value does not look at)
  int row_at[NB];
  sdy_static_for<0, NB>([&](auto I) {
    const int i = 16 * I.value + frag_row;
    row_at[I.value] = (i >= 1 && i <= M ? i - 1 : M) * kStride;
  });

  for (int quarter = 0; quarter < SDY_GRAM_QUARTERS; ++quarter) {
    const long q0 = (long)chunk * SDY_GRAM_CHUNK + (long)quarter * SDY_GRAM_QUARTER;   // the quarter's first point
    if (q0 >= HW) break;                                                 // (the same for the whole block)
    __syncthreads();                                                     // the previous quarter's readers are done
    if (W == 4) {
      const int at = lane * 4;
      if (q0 + at < HW) {
#pragma unroll 4
        for (int i = wave; i < M; i += kWaves)
          *reinterpret_cast<f32x4*>(sh_x + i * kStride + at) = ld<4>(gen + (long)i * gs0 + q0 + at);
      }
    } else if (q0 + tid < HW) {
#pragma unroll 4
      for (int i = 0; i < M; ++i) sh_x[i * kStride + tid] = gen[(long)i * gs0 + q0 + tid];
    }
    {
      const long p = q0 + tid;
      const bool inside = p < HW;
      sh_x[M * kStride + tid] = inside ? tgt[p] : 0.0f;
      sh_w[tid] = inside ? a.weights[p] : 0.0f;                           // past the plane: weight 0, nothing is looked at
      sh_c[tid] = inside && clim ? clim[p] : 0.0f;
    }
    __syncthreads();
#pragma unroll 2
    for (int q = 0; q < kSteps; ++q) {
      const int pt = wave * SDY_GRAM_WAVE_POINTS + q * SDY_GRAM_STEP + frag_pt;
      const float y = sh_x[M * kStride + pt], w = sh_w[pt], c = sh_c[pt];
      double ai[NB], wa[NB];
      sdy_static_for<0, NB>([&](auto I) {
        ai[I.value] = sdy_gram_value(16 * I.value + frag_row, M, sh_x[row_at[I.value] + pt], y, c, w);
        wa[I.value] = (double)w * ai[I.value];
      });
      sdy_static_for<0, NB>([&](auto I) {
        sdy_static_for<I.value, NB>([&](auto J) {
          constexpr int k = tile_at(I.value, J.value, NB);
          acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[I.value], ai[J.value], acc[k], 0, 0, 0);
        });
      });
    }
  }

  // wave 0 + wave 1 + wave 2 + wave 3, in that order, through LDS (over the staged rows: their readers are done)
  double* red = reinterpret_cast<double*>(sh_x);
  for (int k = 1; k < kWaves; ++k) {
    __syncthreads();
    if (wave == k)
      sdy_static_for<0, tiles_of(NB)>([&](auto n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(n.value * 4 + r) * 64 + lane] = acc[n.value][r];
      });
    __syncthreads();
    if (wave == 0)
      sdy_static_for<0, tiles_of(NB)>([&](auto n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[n.value][r] += red[(n.value * 4 + r) * 64 + lane];
      });
  }
  if (wave != 0) return;
  double* out = partials + ((long)v * gridDim.x + blockIdx.x) * sdy_gram_entries(N);
  sdy_static_for<0, NB>([&](auto I) {
    sdy_static_for<I.value, NB>([&](auto J) {
      constexpr int k = tile_at(I.value, J.value, NB);
      const int j = 16 * J.value + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * I.value + (lane >> 4) + 4 * r;
        if (i <= j && j < N) out[sdy_gram_index(i, j, N)] = acc[k][r];
      }
    });
  });
}

int check(const sdy_member_gram_args* a, bool need_ws) {
  if (!a) return SDY_ERR_ARG;
  if (a->HW < 1) return SDY_ERR_ARG;
  if (!a->weights || ((uintptr_t)a->weights & 3) || !a->out || ((uintptr_t)a->out & 7)) return SDY_ERR_ARG;
  SDY_TRY(sdy_window_check(&a->win, a->HW));
  for (int v = 0; v < a->win.nvars; ++v)
    if ((uintptr_t)a->climatology[v] & 3) return SDY_ERR_ARG;
  if (a->win.n0 > kMaxMembers) return SDY_ERR_UNSUPPORTED;
  const long planes = (long)a->win.n1 * a->win.T, entries = sdy_gram_entries(a->win.n0 + 2);
  // 32-bit block numbers within a variable
  if (planes * sdy_gram_chunks(a->HW) > 0x7fffffffL) return SDY_ERR_UNSUPPORTED;
  // ... and flat indices of out below 2^38.  Those of ws then stay below 2^50: nvars * entries <= 96 * 2211 < 2^18 times
  // planes * chunks < 2^31
  if ((long)a->win.nvars * entries * planes >= (1L << 38)) return SDY_ERR_UNSUPPORTED;
  if (need_ws && !sdy_ws_ok(a->ws, a->ws_bytes,
                            sdy_member_gram_workspace_bytes(a->win.nvars, a->win.n0, a->win.n1, a->win.T, a->HW)))
    return SDY_ERR_ARG;
  return SDY_OK;
}

template <int NB>
int launch(const sdy_member_gram_args* a, const dim3 grid, int chunks, double* partials, hipStream_t stream) {
  const size_t smem = lds_bytes(a->win.n0, NB);
  if (sdy_window_vec4(&a->win, a->HW))
    hipLaunchKernelGGL((member_gram_kernel<NB, 4>), grid, dim3(kThreads), smem, stream, *a, chunks, partials);
  else
    hipLaunchKernelGGL((member_gram_kernel<NB, 1>), grid, dim3(kThreads), smem, stream, *a, chunks, partials);
  return sdy_launch_status();
}

template <int NB>
int raise_lds() {
  const int max_smem = (int)lds_bytes(16 * NB - 2 < kMaxMembers ? 16 * NB - 2 : kMaxMembers, NB);
  SDY_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&member_gram_kernel<NB, 4>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, max_smem));
  SDY_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&member_gram_kernel<NB, 1>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, max_smem));
  return SDY_OK;
}

}  // namespace

extern "C" size_t sdy_member_gram_workspace_bytes(int nvars, int n0, int n1, int T, int HW) {
  if (nvars < 1 || nvars > SDY_MAX_VARS || n0 < 1 || n0 > kMaxMembers || n1 < 1 || T < 1 || HW < 1) return 0;
  return (size_t)nvars * (size_t)n1 * (size_t)T * (size_t)sdy_gram_chunks(HW) * (size_t)sdy_gram_entries(n0 + 2) * sizeof(double);
}

// The device's partition: chunks, quarters, the four waves' shares of a quarter, each wave's points in point order into one
// accumulator per entry; then the waves and the chunks in order.  The matrix instruction adds its four products in an order
// of its own: equal to the rounding of a float64 sum, not to the bit.
extern "C" int sdy_member_gram_host(const sdy_member_gram_args* a) {
#pragma clang fp contract(off)
  SDY_TRY(check(a, false));
  const sdy_window& w = a->win;
  const int M = w.n0, N = M + 2, chunks = (int)sdy_gram_chunks(a->HW);
  const long HW = a->HW, entries = sdy_gram_entries(N);
  std::vector<double> partials((size_t)chunks * entries), waves((size_t)SDY_GRAM_WAVES * entries), vec((size_t)N);
  for (int v = 0; v < w.nvars; ++v)
    for (long s = 0; s < w.n1; ++s)
      for (int t = 0; t < w.T; ++t) {
        const float* gen = w.gen[v] + s * w.gs1 + (long)t * HW;
        const float* tgt = w.target[v] + s * w.ts1 + (long)t * HW;
        const float* clim = a->climatology[v];
        for (int c = 0; c < chunks; ++c) {
          for (double& x : waves) x = 0.0;
          const long base = (long)c * SDY_GRAM_CHUNK;
          const int n = (int)(HW - base < SDY_GRAM_CHUNK ? HW - base : SDY_GRAM_CHUNK);
          for (int at = 0; at < n; ++at) {
            const long p = base + at;
            const float wt = a->weights[p];
            if (wt == 0.0f) continue;                                     // every a_i reads as 0: nothing is added
            double* acc = waves.data() + (size_t)((at % SDY_GRAM_QUARTER) / SDY_GRAM_WAVE_POINTS) * entries;
            for (int i = 0; i < N; ++i)
              vec[i] = sdy_gram_value(i, M, i >= 1 && i <= M ? gen[(long)(i - 1) * w.gs0 + p] : 0.0f, tgt[p],
                                      clim ? clim[p] : 0.0f, wt);
            for (int i = 0; i < N; ++i) {
              const double wa = (double)wt * vec[i];
              for (int j = i; j < N; ++j) acc[sdy_gram_index(i, j, N)] += wa * vec[j];
            }
          }
          for (long e = 0; e < entries; ++e) {
            double x = waves[e];
            for (int k = 1; k < SDY_GRAM_WAVES; ++k) x += waves[(size_t)k * entries + e];
            partials[(size_t)c * entries + e] = x;
          }
        }
        double* out = a->out + (((long)v * w.n1 + s) * w.T + t) * entries;
        for (long e = 0; e < entries; ++e) out[e] = sdy_sum_chunks(partials.data(), chunks, entries, e);
      }
  return SDY_OK;
}

extern "C" int sdy_member_gram(const sdy_member_gram_args* a, void* stream) {
  SDY_TRY(check(a, true));
  const int chunks = (int)sdy_gram_chunks(a->HW), N = a->win.n0 + 2, nb = (N + 15) / 16;
  const long planes = (long)a->win.n1 * a->win.T, entries = sdy_gram_entries(N);
  const dim3 grid((unsigned)(planes * chunks), a->win.nvars);
  double* partials = static_cast<double*>(a->ws);
  // 65 rows x 260 words x 4 bytes of dynamic LDS at the member bound, and 63 rows with the 2 KB of static LDS at the top of
  // four blocks: more than the 64 KB a kernel gets unasked
  static SdyOncePerDevice once;
  std::atomic<bool>* attr_done = nullptr;
  SDY_TRY(once.slot(&attr_done));
  if (!*attr_done) {
    SDY_TRY(raise_lds<4>());
    SDY_TRY(raise_lds<5>());
    *attr_done = true;
  }
  int rc = SDY_ERR_UNSUPPORTED;
  switch (nb) {
    case 1: rc = launch<1>(a, grid, chunks, partials, (hipStream_t)stream); break;
    case 2: rc = launch<2>(a, grid, chunks, partials, (hipStream_t)stream); break;
    case 3: rc = launch<3>(a, grid, chunks, partials, (hipStream_t)stream); break;
    case 4: rc = launch<4>(a, grid, chunks, partials, (hipStream_t)stream); break;
    case 5: rc = launch<5>(a, grid, chunks, partials, (hipStream_t)stream); break;
  }
  SDY_TRY(rc);
  return sdy_combine_chunks_launch(partials, (long)a->win.nvars * planes, chunks, entries, a->out, (hipStream_t)stream);
}

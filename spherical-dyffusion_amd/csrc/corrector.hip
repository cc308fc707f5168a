// Post-step state corrector of the stepper (src/ace_inference/core/corrector.py), gfx950: reduce -> solve -> apply, three
// launches per step whatever the batch, the level count and the switches.  HBM-bound streaming: the reduce pass reads every
// needed plane once, the apply pass re-reads what the rewritten fields depend on and writes only those.  The arithmetic of a
// column and the scalar solve are corrector_math.h, shared with the host entry point.  Sums: float64, one partial per
// (sample, 1024-column chunk) in the workspace, added in chunk order by one thread per sample; no atomics.
#include "common.h"
#include "corrector_math.h"
#include "ordered_sum.h"

namespace {

constexpr int kThreads = 256;
constexpr int kColsPerThread = 4;
constexpr int kChunk = kThreads * kColsPerThread;   // columns of one workgroup: the partition of the sums, fixed

int n_chunks(int HW) { return (HW + kChunk - 1) / kChunk; }
size_t partial_doubles(int B, int HW) { return (size_t)B * n_chunks(HW) * SDY_CORR_NSUMS; }

// the thread's 4 neighbouring columns p .. p+3 of sample b: one 16-byte load when the entry point found every plane aligned
// (then HW % 4 == 0 and p < HW covers all four), otherwise four bounds-checked 4-byte loads; columns past HW read as 0
__device__ __forceinline__ f32x4 load_cols(const sdy_corrector_var& v, int b, int p, int HW, bool vec) {
  const float* src = v.base + (long)b * v.stride + p;
  f32x4 x = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    x = *reinterpret_cast<const f32x4*>(src);
  } else {
#pragma unroll
    for (int c = 0; c < kColsPerThread; ++c)
      if (p + c < HW) x[c] = src[c];
  }
#pragma unroll
  for (int c = 0; c < kColsPerThread; ++c) x[c] = sdy_corr_denorm(x[c], v.mean, v.std);
  return x;
}
__device__ __forceinline__ f32x4 load_weights(const float* area, int p, int HW, bool vec) {
  f32x4 x = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    x = *reinterpret_cast<const f32x4*>(area + p);
  } else {
#pragma unroll
    for (int c = 0; c < kColsPerThread; ++c)
      if (p + c < HW) x[c] = area[p + c];
  }
  return x;
}
__device__ __forceinline__ void store_cols(const sdy_corrector_out& o, const sdy_corrector_var& like, int b, int p, int HW,
                                           bool vec, f32x4 y) {
  float* dst = o.base + (long)b * o.stride + p;
#pragma unroll
  for (int c = 0; c < kColsPerThread; ++c) y[c] = sdy_corr_norm(y[c], like.mean, like.std);
  if (vec) {
    *reinterpret_cast<f32x4*>(dst) = y;
  } else {
#pragma unroll
    for (int c = 0; c < kColsPerThread; ++c)
      if (p + c < HW) dst[c] = y[c];
  }
}

struct Needs {
  bool water, zero_adv, budget;
};
__host__ __device__ inline Needs needs_of(int flags, int budget) {
  return {(flags & SDY_CORRECTOR_DRY_AIR) != 0 || budget != 0, (flags & SDY_CORRECTOR_ZERO_ADV) != 0, budget != 0};
}

// grid (chunks, B).  Every variable's planes have been moved to their channel by the entry point (channel == 0 here).
template <int K>
__global__ __launch_bounds__(kThreads) void corrector_reduce_kernel(const sdy_corrector_args a, bool vec, double* partials) {
  const int b = blockIdx.y, HW = a.HW;
  const int p = (blockIdx.x * kThreads + threadIdx.x) * kColsPerThread;
  const Needs need = needs_of(a.flags, a.budget);
  double acc[SDY_CORR_NSUMS];
#pragma unroll
  for (int j = 0; j < SDY_CORR_NSUMS; ++j) acc[j] = 0.0;
  if (p < HW) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 w = load_weights(a.area, p, HW, vec);
    f32x4 qg[K], qi[K];
    f32x4 psg = zero, psi = zero, adv = zero, lhf = zero, prate = zero;
    if (need.water) {
#pragma unroll
      for (int k = 0; k < K; ++k) qg[k] = load_cols(a.gen_q[k], b, p, HW, vec);
#pragma unroll
      for (int k = 0; k < K; ++k) qi[k] = load_cols(a.in_q[k], b, p, HW, vec);
      psg = load_cols(a.gen_ps, b, p, HW, vec);
      psi = load_cols(a.in_ps, b, p, HW, vec);
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) qg[k] = qi[k] = zero;
    }
    if (need.zero_adv) adv = load_cols(a.gen_adv, b, p, HW, vec);
    if (need.budget) {
      lhf = load_cols(a.gen_lhf, b, p, HW, vec);
      prate = load_cols(a.gen_prate, b, p, HW, vec);
    }
#pragma unroll
    for (int c = 0; c < kColsPerThread; ++c)
      if (p + c < HW)
        sdy_corr_accumulate(K, a.ak, a.bk, need.water, need.zero_adv, need.budget, w[c], psg[c],
                            [&](int k) { return qg[k][c]; }, psi[c], [&](int k) { return qi[k][c]; }, adv[c], lhf[c],
                            prate[c], acc);
  }
  // wave butterfly, then the four waves in order: the same tree for every chunk of every sample
  __shared__ double sh[kThreads / 64][SDY_CORR_NSUMS];
#pragma unroll
  for (int j = 0; j < SDY_CORR_NSUMS; ++j) {
    double v = acc[j];
    sdy_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < SDY_CORR_NSUMS)
    partials[((size_t)b * gridDim.x + blockIdx.x) * SDY_CORR_NSUMS + threadIdx.x] = sdy_fold_rows(sh, threadIdx.x);
}

// one thread per sample: the chunks' partials in chunk order, then the scalar solve
__global__ __launch_bounds__(64) void corrector_solve_kernel(const double* partials, int B, int chunks, int flags, int budget,
                                                             sdy_corr_scalars* scalars) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s[SDY_CORR_NSUMS];
  sdy_sum_chunks(partials + (size_t)b * chunks * SDY_CORR_NSUMS, chunks, SDY_CORR_NSUMS, 0, s);
  scalars[b] = sdy_corr_solve(s, (flags & SDY_CORRECTOR_DRY_AIR) != 0, budget);
}

template <int K>
__global__ __launch_bounds__(kThreads) void corrector_apply_kernel(const sdy_corrector_args a, bool vec,
                                                                   const sdy_corr_scalars* scalars) {
  const int b = blockIdx.y, HW = a.HW;
  const int p = (blockIdx.x * kThreads + threadIdx.x) * kColsPerThread;
  if (p >= HW) return;
  const bool dry = (a.flags & SDY_CORRECTOR_DRY_AIR) != 0, zero_adv = (a.flags & SDY_CORRECTOR_ZERO_ADV) != 0;
  const bool re_adv = sdy_corr_recomputes_adv(a.budget);
  const bool s_prate = sdy_corr_scales_prate(a.budget), s_evap = sdy_corr_scales_evap(a.budget);
  const sdy_corr_scalars sc = scalars[b];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 qg[K], qi[K];
  f32x4 psg = zero, psi = zero, adv = zero, lhf = zero, prate = zero;
  if (dry || re_adv) {
#pragma unroll
    for (int k = 0; k < K; ++k) qg[k] = load_cols(a.gen_q[k], b, p, HW, vec);
    psg = load_cols(a.gen_ps, b, p, HW, vec);
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) qg[k] = zero;
  }
  if (re_adv) {
#pragma unroll
    for (int k = 0; k < K; ++k) qi[k] = load_cols(a.in_q[k], b, p, HW, vec);
    psi = load_cols(a.in_ps, b, p, HW, vec);
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) qi[k] = zero;
  }
  if (zero_adv && !re_adv) adv = load_cols(a.gen_adv, b, p, HW, vec);   // (recomputed: the old value does not enter)
  if (s_evap || re_adv) lhf = load_cols(a.gen_lhf, b, p, HW, vec);
  if (s_prate || re_adv) prate = load_cols(a.gen_prate, b, p, HW, vec);
  f32x4 o_ps, o_adv, o_lhf, o_prate;
#pragma unroll
  for (int c = 0; c < kColsPerThread; ++c) {
    const sdy_corr_column r =
        sdy_corr_apply(K, a.ak, a.bk, dry, zero_adv, a.budget, sc, psg[c], [&](int k) { return qg[k][c]; }, psi[c],
                       [&](int k) { return qi[k][c]; }, adv[c], lhf[c], prate[c]);
    o_ps[c] = r.ps;
    o_adv[c] = r.adv;
    o_lhf[c] = r.lhf;
    o_prate[c] = r.prate;
  }
  if (dry) store_cols(a.out_ps, a.gen_ps, b, p, HW, vec, o_ps);
  if (zero_adv || re_adv) store_cols(a.out_adv, a.gen_adv, b, p, HW, vec, o_adv);
  if (s_evap) store_cols(a.out_lhf, a.gen_lhf, b, p, HW, vec, o_lhf);
  if (s_prate) store_cols(a.out_prate, a.gen_prate, b, p, HW, vec, o_prate);
}

template <int K>
int launch_corrector(const sdy_corrector_args& a, bool vec, hipStream_t stream) {
  if (a.K != K) return launch_corrector<K - 1>(a, vec, stream);
  const int chunks = n_chunks(a.HW);
  double* partials = static_cast<double*>(a.ws);
  sdy_corr_scalars* scalars = reinterpret_cast<sdy_corr_scalars*>(partials + partial_doubles(a.B, a.HW));
  const dim3 grid(chunks, a.B);
  hipLaunchKernelGGL(corrector_reduce_kernel<K>, grid, dim3(kThreads), 0, stream, a, vec, partials);
  SDY_TRY(sdy_launch_status());
  hipLaunchKernelGGL(corrector_solve_kernel, dim3((a.B + 63) / 64), dim3(64), 0, stream, partials, a.B, chunks, a.flags,
                     a.budget, scalars);
  SDY_TRY(sdy_launch_status());
  hipLaunchKernelGGL(corrector_apply_kernel<K>, grid, dim3(kThreads), 0, stream, a, vec, scalars);
  return sdy_launch_status();
}
template <>
int launch_corrector<0>(const sdy_corrector_args&, bool, hipStream_t) {
  return SDY_ERR_ARG;
}

bool var_ok(const sdy_corrector_var& v, int B, int HW) {
  if (!v.base || v.channel < 0 || v.stride < 0) return false;
  if (B > 1 && v.stride < ((long)v.channel + 1) * HW) return false;
  return std::isfinite(v.mean) && std::isfinite(v.std) && v.std > 0.f;
}
bool out_ok(const sdy_corrector_out& o, int B, int HW) {
  if (!o.base || o.channel < 0 || o.stride < 0) return false;
  return !(B > 1 && o.stride < ((long)o.channel + 1) * HW);
}

// Everything that bounds an address, for the device and the host entry point alike.  On success *r is the argument block with
// every used plane moved to its channel (channel = 0), K = 1 when no rule reads the water levels, and *vec tells whether every
// used plane takes 16-byte accesses.
int check_args(const sdy_corrector_args* a, bool need_ws, sdy_corrector_args* r, bool* vec) {
  if (!a || a->B < 1 || a->HW < 1 || !a->area) return SDY_ERR_ARG;
  if (a->flags & ~(SDY_CORRECTOR_DRY_AIR | SDY_CORRECTOR_ZERO_ADV)) return SDY_ERR_ARG;
  if (a->budget < 0 || a->budget > 4) return SDY_ERR_ARG;
  const Needs need = needs_of(a->flags, a->budget);
  if (need.water && (a->K < 1 || a->K > SDY_DERIVED_MAX_LEVELS)) return SDY_ERR_ARG;
  if (a->B > 65535) return SDY_ERR_UNSUPPORTED;
  if (need_ws && !sdy_ws_ok(a->ws, a->ws_bytes, sdy_corrector_workspace_bytes(a->B, a->HW))) return SDY_ERR_ARG;
  *r = *a;
  if (!need.water) r->K = 1;
  const int B = a->B, HW = a->HW;
  bool v16 = (HW & 3) == 0 && ((uintptr_t)a->area & 15) == 0;
  bool ok = true;
  auto use_var = [&](sdy_corrector_var& v) {
    if (!var_ok(v, B, HW)) {
      ok = false;
      return;
    }
    v.base += (long)v.channel * HW;
    v.channel = 0;
    v16 = v16 && ((uintptr_t)v.base & 15) == 0 && (B == 1 || (v.stride & 3) == 0);
  };
  auto use_out = [&](sdy_corrector_out& o) {
    if (!out_ok(o, B, HW)) {
      ok = false;
      return;
    }
    o.base += (long)o.channel * HW;
    o.channel = 0;
    v16 = v16 && ((uintptr_t)o.base & 15) == 0 && (B == 1 || (o.stride & 3) == 0);
  };
  if (need.water) {
    for (int k = 0; k < a->K; ++k) {
      use_var(r->gen_q[k]);
      use_var(r->in_q[k]);
    }
    use_var(r->gen_ps);
    use_var(r->in_ps);
  }
  const bool re_adv = sdy_corr_recomputes_adv(a->budget);
  if (need.zero_adv || re_adv) {
    if (need.zero_adv) use_var(r->gen_adv);
    use_out(r->out_adv);
    // the stored form of a recomputed tendency needs the variable's mean / std even when its old value is never read
    if (!need.zero_adv && !(std::isfinite(a->gen_adv.mean) && std::isfinite(a->gen_adv.std) && a->gen_adv.std > 0.f)) ok = false;
  }
  if (need.budget) {
    use_var(r->gen_lhf);
    use_var(r->gen_prate);
    if (sdy_corr_scales_evap(a->budget)) use_out(r->out_lhf);
    if (sdy_corr_scales_prate(a->budget)) use_out(r->out_prate);
  }
  if (a->flags & SDY_CORRECTOR_DRY_AIR) use_out(r->out_ps);
  if (!ok) return SDY_ERR_ARG;
  *vec = v16;
  return SDY_OK;
}

}  // namespace

extern "C" size_t sdy_corrector_workspace_bytes(int B, int HW) {
  if (B < 1 || HW < 1) return 0;
  return partial_doubles(B, HW) * sizeof(double) + (size_t)B * sizeof(sdy_corr_scalars);
}

extern "C" int sdy_corrector_host(const sdy_corrector_args* args) {
  sdy_corrector_args a;
  bool vec = false;
  SDY_TRY(check_args(args, false, &a, &vec));
  const Needs need = needs_of(a.flags, a.budget);
  const bool dry = (a.flags & SDY_CORRECTOR_DRY_AIR) != 0, re_adv = sdy_corr_recomputes_adv(a.budget);
  const int HW = a.HW, K = a.K;
  auto get = [&](const sdy_corrector_var& v, int b, int p) {
    return sdy_corr_denorm(v.base[(long)b * v.stride + p], v.mean, v.std);
  };
  auto put = [&](const sdy_corrector_out& o, const sdy_corrector_var& like, int b, int p, float y) {
    o.base[(long)b * o.stride + p] = sdy_corr_norm(y, like.mean, like.std);
  };
  for (int b = 0; b < a.B; ++b) {
    // the device's partition: 1024-column chunks summed on their own, then added in chunk order (the order within a chunk is
    // the device's tree there and plain column order here)
    double s[SDY_CORR_NSUMS] = {};
    for (int p0 = 0; p0 < HW; p0 += kChunk) {
      double acc[SDY_CORR_NSUMS] = {};
      for (int p = p0; p < HW && p < p0 + kChunk; ++p)
        sdy_corr_accumulate(
            K, a.ak, a.bk, need.water, need.zero_adv, need.budget, a.area[p], need.water ? get(a.gen_ps, b, p) : 0.f,
            [&](int k) { return need.water ? get(a.gen_q[k], b, p) : 0.f; }, need.water ? get(a.in_ps, b, p) : 0.f,
            [&](int k) { return need.water ? get(a.in_q[k], b, p) : 0.f; }, need.zero_adv ? get(a.gen_adv, b, p) : 0.f,
            need.budget ? get(a.gen_lhf, b, p) : 0.f, need.budget ? get(a.gen_prate, b, p) : 0.f, acc);
      for (int j = 0; j < SDY_CORR_NSUMS; ++j) s[j] += acc[j];
    }
    const sdy_corr_scalars sc = sdy_corr_solve(s, dry, a.budget);
    for (int p = 0; p < HW; ++p) {
      const bool wg = dry || re_adv;
      const sdy_corr_column r = sdy_corr_apply(
          K, a.ak, a.bk, dry, need.zero_adv, a.budget, sc, wg ? get(a.gen_ps, b, p) : 0.f,
          [&](int k) { return wg ? get(a.gen_q[k], b, p) : 0.f; }, re_adv ? get(a.in_ps, b, p) : 0.f,
          [&](int k) { return re_adv ? get(a.in_q[k], b, p) : 0.f; }, need.zero_adv && !re_adv ? get(a.gen_adv, b, p) : 0.f,
          need.budget ? get(a.gen_lhf, b, p) : 0.f, need.budget ? get(a.gen_prate, b, p) : 0.f);
      if (dry) put(a.out_ps, a.gen_ps, b, p, r.ps);
      if (need.zero_adv || re_adv) put(a.out_adv, a.gen_adv, b, p, r.adv);
      if (sdy_corr_scales_evap(a.budget)) put(a.out_lhf, a.gen_lhf, b, p, r.lhf);
      if (sdy_corr_scales_prate(a.budget)) put(a.out_prate, a.gen_prate, b, p, r.prate);
    }
  }
  return SDY_OK;
}

extern "C" int sdy_corrector(const sdy_corrector_args* args, void* stream) {
  sdy_corrector_args a;
  bool vec = false;
  SDY_TRY(check_args(args, true, &a, &vec));
  return launch_corrector<SDY_DERIVED_MAX_LEVELS>(a, vec, (hipStream_t)stream);
}

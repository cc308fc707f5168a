// Derived water-budget variables of the inference loop (src/ace_inference/inference/derived_variables.py, formulas of
// src/ace_inference/core/metrics.py:296-367), gfx950.  HBM-bound: every input element is read once, every output written once.
#include "common.h"

namespace {

constexpr float kGravity = 9.80665f;
constexpr float kInvGravity = (float)(1.0 / 9.80665);   // `1 / GRAVITY * integral`: the double quotient, used as fp32
constexpr float kLatentHeat = 2.5e6f;
constexpr float kTimestepSeconds = 21600.f;

// byte offsets below 2^32 (checked by the entry point): SGPR base + 32-bit VGPR offset addressing, no 64-bit address per load
__device__ __forceinline__ f32x4 load4(const float* base, unsigned byte_off) {
  return *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + byte_off);
}
__device__ __forceinline__ void store4(float* base, unsigned byte_off, f32x4 v) {
  *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(base) + byte_off) = v;
}

// One thread = 4 neighbouring grid points of one trajectory (blockIdx.y), all times: twp of the previous time stays in a
// register, so the time difference costs no second read.  The arithmetic is the reference's fp32 chain, operation by
// operation and without contraction to FMA: p_k = ak[k] + ps*bk[k]; dp_k = p_{k+1} - p_k; sum_k dp_k*q_k in level order;
// twp = fp32(1/g) * sum; dry = ps - g*twp; resid = (twp_t - twp_{t-1}) / 21600 - ((lhf / 2.5e6 - prate) + adv).
template <int K>
__global__ __launch_bounds__(256) void derived_water_kernel(const sdy_derived_args a) {
#pragma clang fp contract(off)
  const int p = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (p >= a.HW) return;
  const int traj = blockIdx.y;
  const int i0 = traj / a.n1, i1 = traj - i0 * a.n1;
  const unsigned in0 = (unsigned)(i0 * a.s0 + i1 * a.s1 + p) * 4u, out0 = (unsigned)(traj * a.T * a.HW + p) * 4u;
  const unsigned step = (unsigned)a.HW * 4u;
  const bool resid = a.resid != nullptr;
  f32x4 prev = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < a.T; ++t) {
    const unsigned o = in0 + t * step;
    f32x4 q[K];
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = load4(a.q[k], o);
    const f32x4 ps = load4(a.ps, o);
    f32x4 lhf = {0.f, 0.f, 0.f, 0.f}, pr = lhf, adv = lhf;
    if (resid && t > 0) {
      lhf = load4(a.lhf, o);
      pr = load4(a.prate, o);
      adv = load4(a.adv, o);
    }
    f32x4 twp, dry, res;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float lo = a.ak[0] + ps[c] * a.bk[0], s = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float hi = a.ak[k + 1] + ps[c] * a.bk[k + 1];
        s += (hi - lo) * q[k][c];
        lo = hi;
      }
      twp[c] = kInvGravity * s;
      dry[c] = ps[c] - kGravity * twp[c];
      res[c] = resid && t > 0 ? (twp[c] - prev[c]) / kTimestepSeconds - ((lhf[c] / kLatentHeat - pr[c]) + adv[c]) : 0.f;
    }
    const unsigned w = out0 + t * step;
    if (a.dry) store4(a.dry, w, dry);
    if (a.twp) store4(a.twp, w, twp);
    if (resid) store4(a.resid, w, res);
    prev = twp;
  }
}

template <int K>
int launch_derived(const sdy_derived_args& a, hipStream_t stream) {
  if (a.K != K) return launch_derived<K - 1>(a, stream);
  const dim3 grid((a.HW / 4 + 255) / 256, a.n0 * a.n1);
  hipLaunchKernelGGL(derived_water_kernel<K>, grid, dim3(256), 0, stream, a);
  return sdy_launch_status();
}
template <>
int launch_derived<0>(const sdy_derived_args&, hipStream_t) {
  return SDY_ERR_ARG;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int sdy_derived_water(const sdy_derived_args* a, void* stream) {
  if (!a || a->K < 1 || a->K > SDY_DERIVED_MAX_LEVELS || a->n0 < 1 || a->n1 < 1 || a->T < 1 || a->HW < 4) return SDY_ERR_ARG;
  if (a->HW % 4 || a->s0 % 4 || a->s1 % 4 || a->s0 < 0 || a->s1 < 0) return SDY_ERR_ARG;
  if ((long)a->n0 * a->n1 > 65535) return SDY_ERR_UNSUPPORTED;
  // every element offset of an input or output below 2^30 floats (32-bit byte offsets in the kernel)
  const long in_end = (long)(a->n0 - 1) * a->s0 + (long)(a->n1 - 1) * a->s1 + (long)a->T * a->HW;
  const long out_end = (long)a->n0 * a->n1 * a->T * a->HW;
  if (in_end > (1L << 30) || out_end > (1L << 30)) return SDY_ERR_UNSUPPORTED;
  if (!a->dry && !a->twp && !a->resid) return SDY_OK;
  const float* in[SDY_DERIVED_MAX_LEVELS + 4];
  int n_in = 0;
  for (int k = 0; k < a->K; ++k) in[n_in++] = a->q[k];
  in[n_in++] = a->ps;
  if (a->resid) {
    in[n_in++] = a->lhf;
    in[n_in++] = a->prate;
    in[n_in++] = a->adv;
  }
  for (int i = 0; i < n_in; ++i)
    if (!in[i] || !aligned16(in[i])) return SDY_ERR_ARG;
  for (float* o : {a->dry, a->twp, a->resid})
    if (o && !aligned16(o)) return SDY_ERR_ARG;
  return launch_derived<SDY_DERIVED_MAX_LEVELS>(*a, (hipStream_t)stream);
}

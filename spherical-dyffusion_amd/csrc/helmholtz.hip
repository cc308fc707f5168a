// Vorticity, divergence, streamfunction and velocity potential coefficients of winds, gfx950: an element-wise pass over the two
// coefficient tensors sdy_vector_legendre_fwd leaves in the internal layout Cs[l][m][ri][field] into ONE tensor of the same
// layout that sdy_legendre_inv synthesises.  One lane owns one item of helmholtz.h: four consecutive winds of one (l, m) -- re
// and im of A_D[u], A_D[v], A_M[u], A_M[v] as eight 16-byte loads, the two scale quads, up to eight 16-byte stores -- or one
// quad of fields that no plane covers.  Items of one (l, m) are consecutive lanes, so a wave's loads and stores of one plane are
// one contiguous run.  Lanes with m > l or l = 0 load nothing and store zeros.  No LDS, no atomics; the arithmetic is
// helmholtz.h and vector_spectrum.h, shared with the host twin below.
#include "common.h"
#include "helmholtz.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

__global__ __launch_bounds__(kBlock) void helmholtz_kernel(const sdy_helmholtz_args a, unsigned items, unsigned total) {
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  const unsigned lm = idx / items, item = idx - lm * items;
  const int l = (int)(lm / (unsigned)a.mtr), m = (int)(lm - (unsigned)l * (unsigned)a.mtr);
  const int W = sdy_hh_wind_quads(a.n_winds);
  const long F = a.fields, Fo = a.out_fields;
  float* o_re = a.out + (long)lm * 2 * Fo;
  float* o_im = o_re + Fo;
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  if ((int)item >= W) {                                   // a quad no plane covers
    const int f = sdy_hh_zero_field((int)item - W, a.out_stride, a.n_out, a.n_winds);
    st4(o_re + f, zero);
    st4(o_im + f, zero);
    return;
  }
  const int i0 = 4 * (int)item;
  if (m > l || l == 0) {
#pragma unroll
    for (int q = 0; q < SDY_HH_MAX_OUT; ++q)
      if (q < a.n_out) {
        st4(o_re + (long)q * a.out_stride + i0, zero);
        st4(o_im + (long)q * a.out_stride + i0, zero);
      }
    return;
  }
  const float* d_re = a.Cs_d + (long)lm * 2 * F + i0;
  const float* m_re = a.Cs_m + (long)lm * 2 * F + i0;
  const f32x4 du_re = ld4(d_re + a.u_offset), du_im = ld4(d_re + F + a.u_offset);
  const f32x4 dv_re = ld4(d_re + a.v_offset), dv_im = ld4(d_re + F + a.v_offset);
  const f32x4 mu_re = ld4(m_re + a.u_offset), mu_im = ld4(m_re + F + a.u_offset);
  const f32x4 mv_re = ld4(m_re + a.v_offset), mv_im = ld4(m_re + F + a.v_offset);
  f32x4 su = {1.0f, 1.0f, 1.0f, 1.0f}, sv = su;
  if (a.scale) {
    su = ld4(a.scale + a.u_offset + i0);
    sv = ld4(a.scale + a.v_offset + i0);
  }
  double fac[SDY_HH_MAX_OUT];
#pragma unroll
  for (int q = 0; q < SDY_HH_MAX_OUT; ++q) fac[q] = q < a.n_out ? a.factor[(long)q * a.lmax + l] : 0.0;
  f32x4 re[SDY_HH_MAX_OUT], im[SDY_HH_MAX_OUT];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const sdy_vs_coef g = sdy_vs_combine(du_re[c], du_im[c], dv_re[c], dv_im[c], mu_re[c], mu_im[c], mv_re[c], mv_im[c],
                                         (double)su[c], (double)sv[c]);
    const bool named = i0 + c < a.n_winds;                // the last quad's fields past the last wind are zeros
#pragma unroll
    for (int q = 0; q < SDY_HH_MAX_OUT; ++q) {
      float r, i;
      sdy_hh_plane(g, a.part[q], fac[q], &r, &i);
      re[q][c] = named ? r : 0.0f;
      im[q][c] = named ? i : 0.0f;
    }
  }
#pragma unroll
  for (int q = 0; q < SDY_HH_MAX_OUT; ++q)
    if (q < a.n_out) {
      st4(o_re + (long)q * a.out_stride + i0, re[q]);
      st4(o_im + (long)q * a.out_stride + i0, im[q]);
    }
}

bool off16(const void* p) { return ((uintptr_t)p & 15) != 0; }

// everything both entry points refuse; fills the items per (l, m) and the number of items
int check_helmholtz(const sdy_helmholtz_args* a, unsigned* items, unsigned* total) {
  if (!a || a->struct_size != sizeof(sdy_helmholtz_args)) return SDY_ERR_ARG;
  if (!a->Cs_d || !a->Cs_m || !a->factor || !a->out) return SDY_ERR_ARG;
  if (a->n_out < 1 || a->n_out > SDY_HH_MAX_OUT) return SDY_ERR_ARG;
  for (int q = 0; q < a->n_out; ++q)
    if (a->part[q] != 0 && a->part[q] != 1) return SDY_ERR_ARG;
  if (a->lmax < 1 || a->mtr < 1 || a->fields < 1 || a->out_fields < 1 || a->n_winds < 1) return SDY_ERR_ARG;
  if (a->u_offset < 0 || a->v_offset < 0 || a->out_stride < 0) return SDY_ERR_ARG;
  if ((long)a->u_offset + a->n_winds > a->fields || (long)a->v_offset + a->n_winds > a->fields) return SDY_ERR_ARG;
  if ((long)(a->n_out - 1) * a->out_stride + a->n_winds > a->out_fields) return SDY_ERR_ARG;
  if (((a->fields | a->out_fields | a->u_offset | a->v_offset | a->out_stride) & 3) != 0) return SDY_ERR_ALIGN;
  if (off16(a->Cs_d) || off16(a->Cs_m) || off16(a->out) || off16(a->scale) || ((uintptr_t)a->factor & 7) != 0)
    return SDY_ERR_ALIGN;
  const int W = sdy_hh_wind_quads(a->n_winds);
  if (a->n_out > 1 && a->out_stride < 4 * W) return SDY_ERR_ARG;              // two planes would share a quad
  // the inputs end where the output begins or the other way round
  const size_t in_bytes = (size_t)a->lmax * a->mtr * 2 * a->fields * sizeof(float);
  const size_t out_bytes = (size_t)a->lmax * a->mtr * 2 * a->out_fields * sizeof(float);
  const uintptr_t o = (uintptr_t)a->out;
  for (const float* p : {a->Cs_d, a->Cs_m})
    if (o < (uintptr_t)p + in_bytes && (uintptr_t)p < o + out_bytes) return SDY_ERR_ARG;
  const unsigned long x = (unsigned long)W + (unsigned long)sdy_hh_zero_quads(a->out_fields, a->n_out, a->n_winds);
  const unsigned long n = (unsigned long)a->lmax * a->mtr * x;
  if (n >= (1ul << 31)) return SDY_ERR_UNSUPPORTED;
  *items = (unsigned)x;
  *total = (unsigned)n;
  return SDY_OK;
}

}  // namespace

extern "C" int sdy_helmholtz_factors_host(int lmax, double radius, int kind, int truncate, double* out) {
  if (!out || lmax < 1 || !(radius > 0.0) || !std::isfinite(radius) || (kind != 0 && kind != 1)) return SDY_ERR_ARG;
  for (int l = 0; l < lmax; ++l) {
    const double n = std::sqrt((double)l * ((double)l + 1.0));
    const bool zero = l == 0 || (truncate >= 0 && l > truncate);
    out[l] = zero ? 0.0 : kind == 0 ? -n / radius : radius / n;
  }
  return SDY_OK;
}

extern "C" int sdy_helmholtz_coefficients_host(const sdy_helmholtz_args* a) {
  unsigned items = 0, total = 0;
  SDY_TRY(check_helmholtz(a, &items, &total));
  const int W = sdy_hh_wind_quads(a->n_winds), Z = sdy_hh_zero_quads(a->out_fields, a->n_out, a->n_winds);
  const long F = a->fields, Fo = a->out_fields;
  for (int l = 0; l < a->lmax; ++l)
    for (int m = 0; m < a->mtr; ++m) {
      const long lm = (long)l * a->mtr + m;
      float* o_re = a->out + lm * 2 * Fo;
      float* o_im = o_re + Fo;
      for (int z = 0; z < Z; ++z) {
        const int f = sdy_hh_zero_field(z, a->out_stride, a->n_out, a->n_winds);
        for (int c = 0; c < 4; ++c) o_re[f + c] = o_im[f + c] = 0.0f;
      }
      const float* d_re = a->Cs_d + lm * 2 * F;
      const float* m_re = a->Cs_m + lm * 2 * F;
      for (int i = 0; i < 4 * W; ++i) {
        const bool live = i < a->n_winds && m <= l && l > 0;
        sdy_vs_coef g = {0.0, 0.0, 0.0, 0.0};
        if (live) {
          const long u = a->u_offset + i, v = a->v_offset + i;
          g = sdy_vs_combine(d_re[u], d_re[F + u], d_re[v], d_re[F + v], m_re[u], m_re[F + u], m_re[v], m_re[F + v],
                             a->scale ? (double)a->scale[u] : 1.0, a->scale ? (double)a->scale[v] : 1.0);
        }
        for (int q = 0; q < a->n_out; ++q) {
          float r = 0.0f, im = 0.0f;
          if (live) sdy_hh_plane(g, a->part[q], a->factor[(long)q * a->lmax + l], &r, &im);
          o_re[(long)q * a->out_stride + i] = r;
          o_im[(long)q * a->out_stride + i] = im;
        }
      }
    }
  return SDY_OK;
}

extern "C" int sdy_helmholtz_coefficients(const sdy_helmholtz_args* a, void* stream) {
  unsigned items = 0, total = 0;
  SDY_TRY(check_helmholtz(a, &items, &total));
  const unsigned blocks = (total + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(helmholtz_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, *a, items, total);
  return sdy_launch_status();
}

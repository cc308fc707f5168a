// Rotational and divergent kinetic-energy spectra of the generated, the target and the error winds, gfx950: a streaming
// reduction over the coefficient tensors sdy_vector_legendre_fwd leaves in the internal layout Cs[l][m][ri][field] -- two per
// side, the analyses by the derivative table and by the m / sin(theta) table; the u rows and the v rows of a side are two equal
// runs of one field batch, v_offset fields apart -- folded into float64 accumulators that stay on the device.  The mapping is
// degree_power_kernel's (spectrum.hip): one wave owns one accumulator element (pair, time, degree), its lanes take four
// consecutive rows each, walk the orders m = 0 .. min(l, mtr - 1) in order and meet in a butterfly of cross-lane moves.  No LDS,
// no atomics.  The arithmetic and its order are vector_spectrum.h.
// Per row and order a lane reads eight values of the generated side (re / im of four products) where the scalar spectra read
// two, and with the error accumulators eight of the row's target row: four times the bytes of sdy_degree_power per row.
#include "common.h"
#include "coef_rows.h"
#include "vector_spectrum.h"

#pragma clang fp contract(off)

namespace {

// rows r0 .. r0 + 3 (r0 < rows, a multiple of four) of a run that starts at p[0] and holds `rows` rows; rows past the end read
// as 0.  No branch: a load per quad (VEC: p + r0 is 16-byte aligned and the run's group of fields is padded to a multiple of
// four inside its buffer -- sdy_coef_rows_vec4 -- so the whole quad is addressable) or per row with the row number clamped to
// the run's last row, then a select.  (A branch per row multiplied the kernel's code past the instruction cache: that is why
// this is not spectrum.hip's ld_quad, which branches so as not to load a quad past the end.)
template <bool VEC>
__device__ __forceinline__ Quad ld_quad(const float* p, int r0, int rows) {
  Quad q;
  if (VEC) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(p + r0);
    q.v[0] = x.x; q.v[1] = x.y; q.v[2] = x.z; q.v[3] = x.w;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) q.v[c] = p[r0 + c < rows ? r0 + c : rows - 1];
  }
#pragma unroll
  for (int c = 1; c < 4; ++c) q.v[c] = r0 + c < rows ? q.v[c] : 0.0f;
  return q;
}

// the four planes (re / im of the u run, re / im of the v run) of one coefficient tensor at (l, m), rows r0 .. r0 + 3
struct Planes { Quad u_re, u_im, v_re, v_im; };

template <bool VEC>
__device__ __forceinline__ Planes ld_planes(const float* p, int m, long F, long voff, int r0, int rows) {
  Planes x;
  x.u_re = ld_quad<VEC>(p + (long)(2 * m) * F, r0, rows);
  x.u_im = ld_quad<VEC>(p + (long)(2 * m + 1) * F, r0, rows);
  x.v_re = ld_quad<VEC>(p + (long)(2 * m) * F + voff, r0, rows);
  x.v_im = ld_quad<VEC>(p + (long)(2 * m + 1) * F + voff, r0, rows);
  return x;
}

// What the kernel takes: the members of sdy_vector_spectrum_args with the v offsets between the field counts and the strides,
// filled by Launch::go.  In the public order (v offsets behind the descriptor) the compiler merges the scalar argument loads
// differently and shuffles 1400 lines of the kernel at equal registers; in this order the kernel's code is line for line what
// it was before the descriptor, so its speed is not in question (NOTEBOOK.md 7zd).
struct KernelArgs {
  size_t struct_size;
  const float *gen_d, *gen_m, *target_d, *target_m;
  const float* gen_scale;
  const float* target_scale;
  int lmax, mtr;
  int gen_fields, target_fields;
  int gen_v_offset, target_v_offset;
  int gen_var_stride, gen_time_stride;
  int target_var_stride, target_time_stride;
  int nvars, n0, n1, T;
  int t_start, n_timesteps;
  double *gen_rot, *gen_div, *target_rot, *target_div, *err_rot, *err_div;
};

// blockIdx = (degree l, window time t, pair v); 64 threads
template <bool VEC_G, bool VEC_T, bool ERR>
__global__ __launch_bounds__(kLanes) void vector_degree_power_kernel(const KernelArgs a) {
  const int l = blockIdx.x, t = blockIdx.y, v = blockIdx.z, lane = threadIdx.x;
  // sdy_coef_rows_element(a.rows, v, t, l), spelled out as in degree_power_kernel: with the helper six of the eight
  // instantiations take one more scalar register.  The fields are the u fields; every row's u and v field is inside its
  // buffer (entry point).
  const int mlast = l < a.mtr - 1 ? l : a.mtr - 1;
  const int R = a.n0 * a.n1, n1 = a.n1;
  const long Fg = a.gen_fields, Ft = a.target_fields, gvo = a.gen_v_offset, tvo = a.target_v_offset;
  const long gf0 = (long)v * a.gen_var_stride + (long)t * a.gen_time_stride;
  const long tf0 = (long)v * a.target_var_stride + (long)t * a.target_time_stride;
  const long gl = (long)l * a.mtr * 2 * Fg + gf0, tl = (long)l * a.mtr * 2 * Ft + tf0;
  const float *gd = a.gen_d + gl, *gm = a.gen_m + gl, *td = a.target_d + tl, *tm = a.target_m + tl;

  double rs[4] = {0.0, 0.0, 0.0, 0.0}, ds[4] = {0.0, 0.0, 0.0, 0.0};
  double ers[4] = {0.0, 0.0, 0.0, 0.0}, eds[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r0 = 4 * lane; r0 < R; r0 += SDY_SP_SLOTS) {
    int i1[4];
    double gsu[4], gsv[4], tsu[4], tsv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      i1[c] = (r0 + c) % n1;
      const int rc = r0 + c < R ? r0 + c : R - 1;             // a row past the end takes the last row's scale: its values are 0
      gsu[c] = a.gen_scale ? (double)a.gen_scale[gf0 + rc] : 1.0;
      gsv[c] = a.gen_scale ? (double)a.gen_scale[gf0 + gvo + rc] : 1.0;
      tsu[c] = (ERR && a.target_scale) ? (double)a.target_scale[tf0 + i1[c]] : 1.0;
      tsv[c] = (ERR && a.target_scale) ? (double)a.target_scale[tf0 + tvo + i1[c]] : 1.0;
    }
    double rot[4] = {0.0, 0.0, 0.0, 0.0}, div[4] = {0.0, 0.0, 0.0, 0.0};
    double erot[4] = {0.0, 0.0, 0.0, 0.0}, ediv[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m = 0; m <= mlast; ++m) {
      const Planes D = ld_planes<VEC_G>(gd, m, Fg, gvo, r0, R);
      const Planes M = ld_planes<VEC_G>(gm, m, Fg, gvo, r0, R);
      // the rows' target rows: i1 < n1 names a target row for every c, also past the last generated row, so these loads need no
      // branch and are all in flight together; only the addition below is conditional
      Planes TD, TM;
      if (ERR) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const long re = (long)(2 * m) * Ft + i1[c], im = (long)(2 * m + 1) * Ft + i1[c];
          TD.u_re.v[c] = td[re]; TD.u_im.v[c] = td[im]; TD.v_re.v[c] = td[re + tvo]; TD.v_im.v[c] = td[im + tvo];
          TM.u_re.v[c] = tm[re]; TM.u_im.v[c] = tm[im]; TM.v_re.v[c] = tm[re + tvo]; TM.v_im.v[c] = tm[im + tvo];
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const sdy_vs_coef g = sdy_vs_combine(D.u_re.v[c], D.u_im.v[c], D.v_re.v[c], D.v_im.v[c], M.u_re.v[c], M.u_im.v[c],
                                             M.v_re.v[c], M.v_im.v[c], gsu[c], gsv[c]);
        div[c] = sdy_vs_add(div[c], g.s_re, g.s_im, m);
        rot[c] = sdy_vs_add(rot[c], g.t_re, g.t_im, m);
        if (ERR && r0 + c < R) {
          const sdy_vs_coef h = sdy_vs_combine(TD.u_re.v[c], TD.u_im.v[c], TD.v_re.v[c], TD.v_im.v[c], TM.u_re.v[c],
                                               TM.u_im.v[c], TM.v_re.v[c], TM.v_im.v[c], tsu[c], tsv[c]);
          ediv[c] = sdy_vs_add(ediv[c], g.s_re - h.s_re, g.s_im - h.s_im, m);
          erot[c] = sdy_vs_add(erot[c], g.t_re - h.t_re, g.t_im - h.t_im, m);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      rs[c] += rot[c];
      ds[c] += div[c];
      ers[c] += erot[c];
      eds[c] += ediv[c];
    }
  }
  double trs[4] = {0.0, 0.0, 0.0, 0.0}, tds[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r0 = 4 * lane; r0 < n1; r0 += SDY_SP_SLOTS) {
    double rot[4] = {0.0, 0.0, 0.0, 0.0}, div[4] = {0.0, 0.0, 0.0, 0.0}, tsu[4], tsv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int rc = r0 + c < n1 ? r0 + c : n1 - 1;
      tsu[c] = a.target_scale ? (double)a.target_scale[tf0 + rc] : 1.0;
      tsv[c] = a.target_scale ? (double)a.target_scale[tf0 + tvo + rc] : 1.0;
    }
    for (int m = 0; m <= mlast; ++m) {
      const Planes D = ld_planes<VEC_T>(td, m, Ft, tvo, r0, n1);
      const Planes M = ld_planes<VEC_T>(tm, m, Ft, tvo, r0, n1);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const sdy_vs_coef h = sdy_vs_combine(D.u_re.v[c], D.u_im.v[c], D.v_re.v[c], D.v_im.v[c], M.u_re.v[c], M.u_im.v[c],
                                             M.v_re.v[c], M.v_im.v[c], tsu[c], tsv[c]);
        div[c] = sdy_vs_add(div[c], h.s_re, h.s_im, m);
        rot[c] = sdy_vs_add(rot[c], h.t_re, h.t_im, m);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      trs[c] += rot[c];
      tds[c] += div[c];
    }
  }
  // every lane takes part in the butterfly (lanes without rows bring 0.0)
  const double g_rot = wave_butterfly(sdy_sp_fold4(rs[0], rs[1], rs[2], rs[3]));
  const double g_div = wave_butterfly(sdy_sp_fold4(ds[0], ds[1], ds[2], ds[3]));
  const double t_rot = wave_butterfly(sdy_sp_fold4(trs[0], trs[1], trs[2], trs[3]));
  const double t_div = wave_butterfly(sdy_sp_fold4(tds[0], tds[1], tds[2], tds[3]));
  double e_rot = 0.0, e_div = 0.0;
  if (ERR) {
    e_rot = wave_butterfly(sdy_sp_fold4(ers[0], ers[1], ers[2], ers[3]));
    e_div = wave_butterfly(sdy_sp_fold4(eds[0], eds[1], eds[2], eds[3]));
  }
  if (lane == 0) {
    const long at = ((long)v * a.n_timesteps + (a.t_start + (long)t)) * a.lmax + l;   // the element's `at`
    a.gen_rot[at] += sdy_sp_mean(g_rot, R);
    a.gen_div[at] += sdy_sp_mean(g_div, R);
    a.target_rot[at] += sdy_sp_mean(t_rot, n1);
    a.target_div[at] += sdy_sp_mean(t_div, n1);
    if (ERR) {
      a.err_rot[at] += sdy_sp_mean(e_rot, R);
      a.err_div[at] += sdy_sp_mean(e_div, R);
    }
  }
}

template <bool VEC_G, bool VEC_T, bool ERR>
struct Launch {
  static void go(const sdy_vector_spectrum_args& a, dim3 grid, hipStream_t s) {
    const sdy_coef_rows& r = a.rows;
    const KernelArgs k = {a.struct_size, a.gen_d, a.gen_m, a.target_d, a.target_m, r.gen_scale, r.target_scale, r.lmax, r.mtr,
                          r.gen_fields, r.target_fields, a.gen_v_offset, a.target_v_offset, r.gen_var_stride, r.gen_time_stride,
                          r.target_var_stride, r.target_time_stride, r.nvars, r.n0, r.n1, r.T, r.t_start, r.n_timesteps,
                          a.gen_rot, a.gen_div, a.target_rot, a.target_div, a.err_rot, a.err_div};
    hipLaunchKernelGGL((vector_degree_power_kernel<VEC_G, VEC_T, ERR>), grid, dim3(kLanes), 0, s, k);
  }
};

// the entry points' own checks in front of the descriptor's, for the device and the host entry points alike
int check_vector_spectrum(const sdy_vector_spectrum_args* a) {
  if (!a || a->struct_size != sizeof(sdy_vector_spectrum_args)) return SDY_ERR_ARG;
  if (!a->gen_d || !a->gen_m || !a->target_d || !a->target_m) return SDY_ERR_ARG;
  if (!a->gen_rot || !a->gen_div || !a->target_rot || !a->target_div) return SDY_ERR_ARG;
  if ((a->err_rot == nullptr) != (a->err_div == nullptr)) return SDY_ERR_ARG;
  return sdy_coef_rows_check(&a->rows, a->gen_v_offset, a->target_v_offset);
}

// one row's eight values at order m of the two tensors p_d, p_m (already at (l, first u field)), row field r
inline sdy_vs_coef host_coef(const float* p_d, const float* p_m, int m, long F, long voff, long r, double su, double sv) {
  const long re = (long)(2 * m) * F + r, im = (long)(2 * m + 1) * F + r;
  return sdy_vs_combine(p_d[re], p_d[im], p_d[re + voff], p_d[im + voff], p_m[re], p_m[im], p_m[re + voff], p_m[im + voff], su,
                        sv);
}

}  // namespace

extern "C" int sdy_vector_degree_power_host(const sdy_vector_spectrum_args* a) {
  SDY_TRY(check_vector_spectrum(a));
  const sdy_coef_rows& r = a->rows;
  const long Fg = r.gen_fields, Ft = r.target_fields, gvo = a->gen_v_offset, tvo = a->target_v_offset;
  const int R = r.n0 * r.n1, n1 = r.n1;
  const bool err = a->err_rot != nullptr;
  double rs[SDY_SP_SLOTS], ds[SDY_SP_SLOTS], trs[SDY_SP_SLOTS], tds[SDY_SP_SLOTS], ers[SDY_SP_SLOTS], eds[SDY_SP_SLOTS];
  sdy_coef_rows_walk(r, [&](const sdy_coef_element el) {
    const long gf0 = el.gf0, tf0 = el.tf0;
    const float *gd = a->gen_d + el.gl, *gm = a->gen_m + el.gl, *td = a->target_d + el.tl, *tm = a->target_m + el.tl;
    for (int s = 0; s < SDY_SP_SLOTS; ++s) rs[s] = ds[s] = trs[s] = tds[s] = ers[s] = eds[s] = 0.0;
    for (int row = 0; row < R; ++row) {
      const int i1 = row % n1;
      const double gsu = r.gen_scale ? (double)r.gen_scale[gf0 + row] : 1.0;
      const double gsv = r.gen_scale ? (double)r.gen_scale[gf0 + gvo + row] : 1.0;
      const double tsu = r.target_scale ? (double)r.target_scale[tf0 + i1] : 1.0;
      const double tsv = r.target_scale ? (double)r.target_scale[tf0 + tvo + i1] : 1.0;
      double rot = 0.0, div = 0.0, erot = 0.0, ediv = 0.0;
      for (int m = 0; m <= el.mlast; ++m) {
        const sdy_vs_coef g = host_coef(gd, gm, m, Fg, gvo, row, gsu, gsv);
        div = sdy_vs_add(div, g.s_re, g.s_im, m);
        rot = sdy_vs_add(rot, g.t_re, g.t_im, m);
        if (err) {
          const sdy_vs_coef h = host_coef(td, tm, m, Ft, tvo, i1, tsu, tsv);
          ediv = sdy_vs_add(ediv, g.s_re - h.s_re, g.s_im - h.s_im, m);
          erot = sdy_vs_add(erot, g.t_re - h.t_re, g.t_im - h.t_im, m);
        }
      }
      rs[row % SDY_SP_SLOTS] += rot;
      ds[row % SDY_SP_SLOTS] += div;
      ers[row % SDY_SP_SLOTS] += erot;
      eds[row % SDY_SP_SLOTS] += ediv;
    }
    for (int row = 0; row < n1; ++row) {
      const double tsu = r.target_scale ? (double)r.target_scale[tf0 + row] : 1.0;
      const double tsv = r.target_scale ? (double)r.target_scale[tf0 + tvo + row] : 1.0;
      double rot = 0.0, div = 0.0;
      for (int m = 0; m <= el.mlast; ++m) {
        const sdy_vs_coef h = host_coef(td, tm, m, Ft, tvo, row, tsu, tsv);
        div = sdy_vs_add(div, h.s_re, h.s_im, m);
        rot = sdy_vs_add(rot, h.t_re, h.t_im, m);
      }
      trs[row % SDY_SP_SLOTS] += rot;
      tds[row % SDY_SP_SLOTS] += div;
    }
    sdy_coef_rows_add(a->gen_rot, el.at, rs, R);
    sdy_coef_rows_add(a->gen_div, el.at, ds, R);
    sdy_coef_rows_add(a->target_rot, el.at, trs, n1);
    sdy_coef_rows_add(a->target_div, el.at, tds, n1);
    if (err) {
      sdy_coef_rows_add(a->err_rot, el.at, ers, R);
      sdy_coef_rows_add(a->err_div, el.at, eds, R);
    }
  });
  return SDY_OK;
}

extern "C" int sdy_vector_degree_power(const sdy_vector_spectrum_args* a, void* stream) {
  SDY_TRY(check_vector_spectrum(a));
  const sdy_coef_rows& r = a->rows;
  const bool vg = sdy_coef_rows_vec4(a->gen_d, a->gen_m, r.gen_fields, a->gen_v_offset, r.gen_var_stride, r.gen_time_stride);
  const bool vt = sdy_coef_rows_vec4(a->target_d, a->target_m, r.target_fields, a->target_v_offset, r.target_var_stride,
                                     r.target_time_stride);
  sdy_coef_rows_dispatch<Launch>(r, vg, vt, a->err_rot != nullptr, *a, (hipStream_t)stream);
  return sdy_launch_status();
}

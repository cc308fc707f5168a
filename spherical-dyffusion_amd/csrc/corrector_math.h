// The post-step state corrector (src/ace_inference/core/corrector.py) as ONE definition for the device kernels (corrector.hip)
// and the host entry point sdy_corrector_host: the per-column fp32 chain, operation by operation as the reference evaluates it
// (metrics.vertical_integral, metrics.surface_pressure_due_to_dry_air, ClimateData.evaporation_rate), never contracted to FMA and
// with the levels summed in order; and the scalar solve that turns a sample's float64 sums into the three numbers the apply
// pass needs.  One quantity leaves the fp32 chain: the water-path tendency of the budget rule is formed in float64 from the
// fp32 fields and rounded once (sdy_corr_tend), so that a recomputed advective tendency closes the budget of the corrected fp32
// fields per column to one rounding of the water path; the fp32 chain's K products and sums, for gen and for the input, leave several.
#pragma once

#define SDY_CORR_HD __host__ __device__ inline

constexpr float kCorrGravity = 9.80665f;
constexpr float kCorrInvGravity = (float)(1.0 / 9.80665);   // `1 / GRAVITY * integral`: the double quotient, used as fp32
constexpr float kCorrLatentHeat = 2.5e6f;
constexpr float kCorrTimestepSeconds = 21600.f;

// the sums of one sample, all weighted by the area weight w of the column
enum {
  SDY_CORR_S_W = 0,      // w
  SDY_CORR_S_DRY_GEN,    // w * dry(gen)
  SDY_CORR_S_DRY_IN,     // w * dry(input)
  SDY_CORR_S_ADV,        // w * adv
  SDY_CORR_S_EVAP,       // w * lhf / 2.5e6
  SDY_CORR_S_PRATE,      // w * prate
  SDY_CORR_S_TEND,       // w * (twp(gen) - twp(input)) / 21600, with the surface pressure the network gave
  SDY_CORR_S_TEND_SLOPE, // w * d twp(gen) / d err  (see sdy_corr_twp_slope)
  SDY_CORR_NSUMS
};

struct sdy_corr_scalars {
  float err;        // global-mean dry air of gen minus that of the input
  float adv_mean;   // global-mean advective tendency
  float scale;      // factor on the precipitation rate or on the evaporation rate
  float pad;
};

// physical value of a stored one and back: `x * std + mean`, `(y - mean) / std`; exact for mean = 0, std = 1
SDY_CORR_HD float sdy_corr_denorm(float x, float mean, float std) {
#pragma clang fp contract(off)
  return x * std + mean;
}
SDY_CORR_HD float sdy_corr_norm(float y, float mean, float std) {
#pragma clang fp contract(off)
  return (y - mean) / std;
}

// sum_k dp_k * q_k, dp_k = (ak[k+1] + ps*bk[k+1]) - (ak[k] + ps*bk[k]), levels in order; q(k) -> specific total water of level k
template <class Q>
SDY_CORR_HD float sdy_corr_dp_q(int K, const float* ak, const float* bk, float ps, Q q) {
#pragma clang fp contract(off)
  float lo = ak[0] + ps * bk[0], s = 0.f;
  for (int k = 0; k < K; ++k) {
    const float hi = ak[k + 1] + ps * bk[k + 1];
    s += (hi - lo) * q(k);
    lo = hi;
  }
  return s;
}
SDY_CORR_HD float sdy_corr_twp(float dp_q) {
#pragma clang fp contract(off)
  return kCorrInvGravity * dp_q;
}
SDY_CORR_HD float sdy_corr_dry(float ps, float twp) {
#pragma clang fp contract(off)
  return ps - kCorrGravity * twp;
}

// A = sum_k (ak[k+1] - ak[k]) * q_k and Bq = sum_k (bk[k+1] - bk[k]) * q_k, levels in order
template <class Q>
SDY_CORR_HD void sdy_corr_ab(int K, const float* ak, const float* bk, Q q, float* A, float* Bq) {
#pragma clang fp contract(off)
  float a = 0.f, b = 0.f;
  for (int k = 0; k < K; ++k) {
    a += (ak[k + 1] - ak[k]) * q(k);
    b += (bk[k + 1] - bk[k]) * q(k);
  }
  *A = a;
  *Bq = b;
}
SDY_CORR_HD float sdy_corr_ps_new(float dry, float err, float A, float Bq) {
#pragma clang fp contract(off)
  return ((dry - err) + A) / (1.f - Bq);
}
// ps_new is affine in err per column, and so is twp(ps_new) = (A + ps_new * Bq) / g:  d twp / d err = -Bq / (g * (1 - Bq)).
// Only its weighted mean is used (sdy_corr_solve), so it is formed in float64.
SDY_CORR_HD double sdy_corr_twp_slope(float Bq) { return -(double)Bq / (9.80665 * (1.0 - (double)Bq)); }

// sum_k dp_k * q_k / g in float64, levels in order: every product of two fp32 values is exact, the sums round at 2^-53
template <class Q>
SDY_CORR_HD double sdy_corr_twp64(int K, const float* ak, const float* bk, float ps, Q q) {
#pragma clang fp contract(off)
  double lo = (double)ak[0] + (double)ps * (double)bk[0], s = 0.0;
  for (int k = 0; k < K; ++k) {
    const double hi = (double)ak[k + 1] + (double)ps * (double)bk[k + 1];
    s += (hi - lo) * (double)q(k);
    lo = hi;
  }
  return s / 9.80665;
}
// (twp(gen) - twp(input)) / 21600 of the fp32 fields, one rounding
template <class QG, class QI>
SDY_CORR_HD float sdy_corr_tend(int K, const float* ak, const float* bk, float ps_gen, QG q_gen, float ps_in, QI q_in) {
#pragma clang fp contract(off)
  return (float)((sdy_corr_twp64(K, ak, bk, ps_gen, q_gen) - sdy_corr_twp64(K, ak, bk, ps_in, q_in)) / 21600.0);
}
SDY_CORR_HD float sdy_corr_evap(float lhf) { return lhf / kCorrLatentHeat; }
// `gen.evaporation_rate = evap * scale`: the setter stores evap * scale * 2.5e6 as the latent heat flux
SDY_CORR_HD float sdy_corr_lhf_scaled(float lhf, float scale) {
#pragma clang fp contract(off)
  return (sdy_corr_evap(lhf) * scale) * kCorrLatentHeat;
}
SDY_CORR_HD float sdy_corr_adv_residual(float tend, float evap, float prate) {
#pragma clang fp contract(off)
  return tend - (evap - prate);
}

// flags / budget modes of sdy_corrector_args (include/sdy_amd.h)
SDY_CORR_HD bool sdy_corr_scales_prate(int budget) { return budget == 1 || budget == 3; }
SDY_CORR_HD bool sdy_corr_scales_evap(int budget) { return budget == 2 || budget == 4; }
SDY_CORR_HD bool sdy_corr_recomputes_adv(int budget) { return budget == 3 || budget == 4; }

// The scalar solve of one sample from its float64 sums.  The budget's global-mean tendency is the one of the surface pressure
// the apply pass will write: mean(tend) = S_TEND / W + err * S_TEND_SLOPE / (W * 21600), with the fp32 err that is applied.
// A zero mean precipitation / evaporation (or W = 0) gives inf / nan, as in the reference.
SDY_CORR_HD sdy_corr_scalars sdy_corr_solve(const double* s, bool conserve_dry_air, int budget) {
#pragma clang fp contract(off)
  sdy_corr_scalars r;
  const double W = s[SDY_CORR_S_W];
  r.err = conserve_dry_air ? (float)((s[SDY_CORR_S_DRY_GEN] - s[SDY_CORR_S_DRY_IN]) / W) : 0.f;
  r.adv_mean = (float)(s[SDY_CORR_S_ADV] / W);
  const double tend = s[SDY_CORR_S_TEND] / W + (double)r.err * (s[SDY_CORR_S_TEND_SLOPE] / W) / 21600.0;
  const double evap = s[SDY_CORR_S_EVAP] / W, prate = s[SDY_CORR_S_PRATE] / W;
  r.scale = 1.f;
  if (sdy_corr_scales_prate(budget)) r.scale = (float)((evap - tend) / prate);
  if (sdy_corr_scales_evap(budget)) r.scale = (float)((tend + prate) / evap);
  r.pad = 0.f;
  return r;
}

// One column's contribution to the sums of its sample.  `water`: the vertical integrals are needed (conserve_dry_air or a budget
// mode); values that a switched-off rule would read are passed as 0 and not touched.
template <class QG, class QI>
SDY_CORR_HD void sdy_corr_accumulate(int K, const float* ak, const float* bk, bool water, bool zero_adv, bool budget, float w,
                                     float ps_gen, QG q_gen, float ps_in, QI q_in, float adv, float lhf, float prate,
                                     double* acc) {
#pragma clang fp contract(off)
  const double wd = (double)w;
  acc[SDY_CORR_S_W] += wd;
  if (water) {
    const float twp_gen = sdy_corr_twp(sdy_corr_dp_q(K, ak, bk, ps_gen, q_gen));
    const float twp_in = sdy_corr_twp(sdy_corr_dp_q(K, ak, bk, ps_in, q_in));
    float A, Bq;
    sdy_corr_ab(K, ak, bk, q_gen, &A, &Bq);
    acc[SDY_CORR_S_DRY_GEN] += wd * (double)sdy_corr_dry(ps_gen, twp_gen);
    acc[SDY_CORR_S_DRY_IN] += wd * (double)sdy_corr_dry(ps_in, twp_in);
    if (budget) {
      acc[SDY_CORR_S_TEND] += wd * (double)sdy_corr_tend(K, ak, bk, ps_gen, q_gen, ps_in, q_in);
      acc[SDY_CORR_S_TEND_SLOPE] += wd * sdy_corr_twp_slope(Bq);
    }
  }
  if (zero_adv) acc[SDY_CORR_S_ADV] += wd * (double)adv;
  if (budget) {
    acc[SDY_CORR_S_EVAP] += wd * (double)sdy_corr_evap(lhf);
    acc[SDY_CORR_S_PRATE] += wd * (double)prate;
  }
}

// One column's corrected values, the reference's three rules in its order.  A field that no rule rewrites comes back as given.
struct sdy_corr_column {
  float ps, adv, lhf, prate;
};
template <class QG, class QI>
SDY_CORR_HD sdy_corr_column sdy_corr_apply(int K, const float* ak, const float* bk, bool conserve_dry_air, bool zero_adv,
                                           int budget, sdy_corr_scalars sc, float ps_gen, QG q_gen, float ps_in, QI q_in,
                                           float adv, float lhf, float prate) {
#pragma clang fp contract(off)
  sdy_corr_column r = {ps_gen, adv, lhf, prate};
  if (conserve_dry_air) {
    const float dry = sdy_corr_dry(ps_gen, sdy_corr_twp(sdy_corr_dp_q(K, ak, bk, ps_gen, q_gen)));
    float A, Bq;
    sdy_corr_ab(K, ak, bk, q_gen, &A, &Bq);
    r.ps = sdy_corr_ps_new(dry, sc.err, A, Bq);
  }
  if (zero_adv) r.adv = adv - sc.adv_mean;
  if (sdy_corr_scales_prate(budget)) r.prate = prate * sc.scale;
  if (sdy_corr_scales_evap(budget)) r.lhf = sdy_corr_lhf_scaled(lhf, sc.scale);
  if (sdy_corr_recomputes_adv(budget)) {
    const float tend = sdy_corr_tend(K, ak, bk, r.ps, q_gen, ps_in, q_in);
    r.adv = sdy_corr_adv_residual(tend, sdy_corr_evap(r.lhf), r.prate);
  }
  return r;
}

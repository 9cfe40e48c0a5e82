// freezing_rows.h -- the row code of the freezing path (include/sdm_freezing.h), shared by the
// stage kernels of freezing.hip and the ice passes of the mixed-phase parcel (parcel_solver.h,
// include/sdm_parcel_ice.h): both translation units evaluate a row with this text, so the fused
// parcel equals the stages to the bit by construction.
//
// Reference: PySDM/backends/impl_numba/methods/freezing_methods.py ("fm.py" below),
// impl_numba/methods/physics_methods.py:78-105 ("pm.py"), physics/trivia.py:79-92,158-163,
// physics/{heterogeneous,homogeneous}_ice_nucleation_rate/, physics/saturation_vapour_pressure/
// flatau_walko_cotton.py (pvs_ice), physics/particle_shape_and_density/mixed_phase_spheres.py.
// Python evaluates left to right; every expression keeps that order, nothing is contracted
// (-ffp-contract=off), and pow / exp are csrc/sdm_math.h.
#ifndef SDM_FREEZING_ROWS_H
#define SDM_FREEZING_ROWS_H
#include "common.h"
#include "../../include/sdm_freezing.h"

namespace {

struct Kf {
  double T0, rho_w, rho_i, eps, FWC_I[9], J_HET, ABIFM_M, ABIFM_C, ABIFM_UNIT, J_HOM, KOOP_2000[4],
      KOOP_CORR, KOOP_UNIT, KOOP_MIN, KOOP_MAX, KOOP_MURRAY[7];
};

Kf frz_consts_of(const double *c) {
  Kf k;
  k.T0 = c[SDM_FRZ_K_T0]; k.rho_w = c[SDM_FRZ_K_RHO_W]; k.rho_i = c[SDM_FRZ_K_RHO_I];
  k.eps = c[SDM_FRZ_K_EPS];
  for (int i = 0; i < 9; ++i) k.FWC_I[i] = c[SDM_FRZ_K_FWC_I0 + i];
  k.J_HET = c[SDM_FRZ_K_J_HET]; k.ABIFM_M = c[SDM_FRZ_K_ABIFM_M];
  k.ABIFM_C = c[SDM_FRZ_K_ABIFM_C]; k.ABIFM_UNIT = c[SDM_FRZ_K_ABIFM_UNIT];
  k.J_HOM = c[SDM_FRZ_K_J_HOM];
  for (int i = 0; i < 4; ++i) k.KOOP_2000[i] = c[SDM_FRZ_K_KOOP_2000_C1 + i];
  k.KOOP_CORR = c[SDM_FRZ_K_KOOP_CORR]; k.KOOP_UNIT = c[SDM_FRZ_K_KOOP_UNIT];
  k.KOOP_MIN = c[SDM_FRZ_K_KOOP_MIN_DA_W_ICE]; k.KOOP_MAX = c[SDM_FRZ_K_KOOP_MAX_DA_W_ICE];
  for (int i = 0; i < 7; ++i) k.KOOP_MURRAY[i] = c[SDM_FRZ_K_KOOP_MURRAY_C0 + i];
  return k;
}

// ---- formulae ------------------------------------------------------------------------------------
// heterogeneous_ice_nucleation_rate/{constant,abifm}.py
__device__ __forceinline__ double j_het(const Kf &k, int code, const double *a_w_ice, int64_t c) {
  if (code == SDM_FRZ_JHET_CONSTANT) return k.J_HET;
  return sdm_pow(10.0, k.ABIFM_M * (1 - a_w_ice[c]) + k.ABIFM_C) * k.ABIFM_UNIT;
}

// homogeneous_ice_nucleation_rate/{koop,koop_corr,koop_murray}.py
__device__ __forceinline__ double j_hom(const Kf &k, int code, double T, double d) {
  if (code == SDM_FRZ_JHOM_KOOPMURRAY2016) {
    const double t = T - k.T0;
    double s = k.KOOP_MURRAY[0] + k.KOOP_MURRAY[1] * t;
    s = s + k.KOOP_MURRAY[2] * sdm_pow(t, 2.0);
    s = s + k.KOOP_MURRAY[3] * sdm_pow(t, 3.0);
    s = s + k.KOOP_MURRAY[4] * sdm_pow(t, 4.0);
    s = s + k.KOOP_MURRAY[5] * sdm_pow(t, 5.0);
    s = s + k.KOOP_MURRAY[6] * sdm_pow(t, 6.0);
    return sdm_pow(10.0, s) * k.KOOP_UNIT;
  }
  double s = k.KOOP_2000[0] + k.KOOP_2000[1] * d;
  s = s + k.KOOP_2000[2] * sdm_pow(d, 2.0);
  s = s + k.KOOP_2000[3] * sdm_pow(d, 3.0);
  if (code == SDM_FRZ_JHOM_KOOP_CORRECTION) s = s + k.KOOP_CORR;
  return sdm_pow(10.0, s) * k.KOOP_UNIT;
}

// the immersion rate of cell c, NaN where no droplet of the cell can freeze (fm.py:99-103:
// unfrozen_and_saturated needs RH > 1)
__device__ __forceinline__ double het_rate_of_cell(const Kf &k, int code, const double *RH,
                                                   const double *a_w_ice, int64_t c) {
  if (!(RH[c] > 1)) return sdm_nan();
  return j_het(k, code, a_w_ice, c);
}

// the homogeneous rate of cell c, NaN where no droplet of the cell can freeze (fm.py:149-160:
// RH_ice > 1, d_a_w_ice within the formula's range, limited to its maximum)
__device__ __forceinline__ double hom_rate_of_cell(const Kf &k, int code, const double *T,
                                                   const double *RH_ice, const double *a_w_ice,
                                                   int64_t c) {
  const double rhi = RH_ice[c];
  if (!(rhi > 1)) return sdm_nan();
  if (code == SDM_FRZ_JHOM_CONSTANT) return k.J_HOM;  // constant.py: always in range
  double d = (rhi - 1.0) * a_w_ice[c];
  if (!(d >= k.KOOP_MIN)) return sdm_nan();
  if (d > k.KOOP_MAX) d = k.KOOP_MAX;
  return j_hom(k, code, T[c], d);
}

// fm.py:105-109 / :162-166 with trivia.py:158-163: true if the droplet freezes
__device__ __forceinline__ bool nucleates(double rate_per_unit, double extent, double dt,
                                          double u) {
  const double r = rate_per_unit * extent;
  const double prob = 1 - sdm_exp(-r * dt);
  return u < prob;
}

// flatau_walko_cotton.py: pvs_ice
__device__ __forceinline__ double pvs_ice(const Kf &k, double T) {
  const double t = T - k.T0;
  double s = k.FWC_I[7] + t * k.FWC_I[8];
  for (int i = 6; i >= 0; --i) s = k.FWC_I[i] + t * s;
  return s;
}

// ---- the three passes for one row: true if the mass changed sign -----------------------------------
// Thaw first (thaw && m < 0 && T > T0), else the pass's own freezing condition; the sign is applied
// once, by one select on the two conditions.
// fm.py:40-66; T, RH: the row's cell
__device__ __forceinline__ bool freeze_singular_row(double &m, double tfz, double T, double RH,
                                                    int thaw, double T0) {
  if (tfz == 0) return false;  // fm.py:52-53
  const bool thaws = thaw && m < 0 && T > T0;
  const bool freezes = !thaws && m > 0 && RH > 1 && T <= tfz;
  const bool flips = thaws || freezes;
  m = flips ? -m : m;
  return flips;
}

// fm.py:68-111; `rate`: het_rate_of_cell of the row's cell (read for m > 0 only)
__device__ __forceinline__ bool freeze_time_dependent_row(double &m, double area, double T,
                                                          double rate, double dt, double u,
                                                          int thaw, double T0) {
  if (area == 0) return false;  // fm.py:92-93
  const bool thaws = thaw && m < 0 && T > T0;
  const bool freezes = !thaws && m > 0 && nucleates(rate, area, dt, u);
  const bool flips = thaws || freezes;
  m = flips ? -m : m;
  return flips;
}

// fm.py:113-168; `rate`: hom_rate_of_cell of the row's cell (read for m > 0 only)
__device__ __forceinline__ bool freeze_homogeneous_row(double &m, double volume, double T,
                                                       double rate, double dt, double u, int thaw,
                                                       double T0) {
  const bool thaws = thaw && m < 0 && T > T0;
  const bool freezes = !thaws && m > 0 && nucleates(rate, volume, dt, u);
  const bool flips = thaws || freezes;
  m = flips ? -m : m;
  return flips;
}

// mixed_phase_spheres.py mass_to_volume of a mass > 0: what PySDM's `volume` attribute holds when
// the homogeneous pass reaches a liquid droplet (sdm_freezing_step with volume = NULL)
__device__ __forceinline__ double liquid_volume_of(const Kf &k, double m) {
  return m / k.rho_w + 0.0 / k.rho_i;
}

// fm.py:241-248; returns true if `data` changed
__device__ __forceinline__ bool record_one(double &data, double m, double T_cell) {
  if (m > 0) {
    if (data > 0) {
      data = sdm_nan();
      return true;
    }
  } else if (data != data) {
    data = T_cell;
    return true;
  }
  return false;
}

// pm.py:78-105 for one cell
__device__ __forceinline__ void a_w_ice_of(const Kf &k, double T, double p, double RH, double qv,
                                           double &a_w_ice, double &RH_ice) {
  const double pvi = pvs_ice(k, T);        // pm.py:87
  const double pv = p * qv / (qv + k.eps);  // libcloudphplusplus.py: pv
  const double pvs = pv / RH;
  a_w_ice = pvi / pvs;
  RH_ice = pv / pvi;
}

}  // namespace

#endif  // SDM_FREEZING_ROWS_H

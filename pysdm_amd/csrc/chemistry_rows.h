/*
 * chemistry_rows.h -- the per-cell and per-row arithmetic of the aqueous-chemistry path
 * (include/sdm_chemistry.h), for both compilers of this project (hipcc for gfx950, gcc for the CPU
 * checker), as sdm_math.h is: same operations in the same order, nothing contracted, so the same
 * bits on both.
 *
 * Reference: PySDM/backends/impl_numba/methods/chemistry_methods.py ("cm.py" below),
 * PySDM/dynamics/impl/chemistry_utils.py ("cu.py") and PySDM/physics/trivia.py:39-64.  Python
 * evaluates left to right; every expression keeps that order, one rounding per operation;
 * pow / exp / log10 are sdm_math.h, sqrt is IEEE.  `k` is the consts array of the header.
 */
#ifndef SDM_CHEMISTRY_ROWS_H
#define SDM_CHEMISTRY_ROWS_H
#include "../../include/sdm_chemistry.h"
#include "sdm_math.h"

/* what acidity_minfun and calc_ionic_strength read: _conc, _K (cm.py:32-33) and K_H2O */
typedef struct chem_acid {
  double N_mIII, N_V, C_IV, S_IV, S_VI;
  double NH3, SO2, HSO3, HSO4, HCO3, CO2, HNO3;
  double K_H2O;
} chem_acid;

/* cm.py:464-476 */
SDM_MATH_FN double chem_acidity_minfun(double H, const chem_acid *q) {
  const double ammonia = (q->N_mIII * H * q->NH3) / (q->K_H2O + q->NH3 * H);
  const double nitric = q->N_V * q->HNO3 / (H + q->HNO3);
  const double sulfous =
      q->S_IV * q->SO2 * (H + 2 * q->HSO3) / (H * H + H * q->SO2 + q->SO2 * q->HSO3);
  const double water = q->K_H2O / H;
  const double sulfuric = q->S_VI * (H + 2 * q->HSO4) / (H + q->HSO4);
  const double carbonic =
      q->C_IV * q->CO2 * (H + 2 * q->HCO3) / (H * H + H * q->CO2 + q->CO2 * q->HCO3);
  return H + ammonia - (nitric + sulfous + water + sulfuric + carbonic);
}

#define TOMS748_FN SDM_MATH_FN
#define TOMS748_ARGS chem_acid
#define TOMS748_EVAL(x, args) chem_acidity_minfun((x), (args))
#include "toms748.h"

/* cm.py:433-460 */
SDM_MATH_FN double chem_ionic_strength(double H, const chem_acid *q) {
  const double water = H + q->K_H2O / H;
  const double cz_S_VI =
      H * q->S_VI / (H + q->HSO4) + 4 * q->HSO4 * q->S_VI / (H + q->HSO4);
  const double cz_CO2 =
      q->CO2 * H * q->C_IV / (H * H + q->CO2 * H + q->CO2 * q->HCO3) +
      4 * q->CO2 * q->HCO3 * q->C_IV / (H * H + q->CO2 * H + q->CO2 * q->HCO3);
  const double cz_SO2 =
      q->SO2 * H * q->S_IV / (H * H + q->SO2 * H + q->SO2 * q->HSO3) +
      4 * q->SO2 * q->HSO3 * q->S_IV / (H * H + q->SO2 * H + q->SO2 * q->HSO3);
  const double cz_HNO3 = q->HNO3 * q->N_V / (H + q->HNO3);
  const double cz_NH3 = q->NH3 * H * q->N_mIII / (q->K_H2O + q->NH3 * H);
  return 0.5 * (water + cz_S_VI + cz_CO2 + cz_SO2 + cz_HNO3 + cz_NH3);
}

/* trivia.py:43-48 */
SDM_MATH_FN double chem_pH2H(double pH) { return sdm_pow(10.0, -pH) * 1e3; }
SDM_MATH_FN double chem_H2pH(double H) { return -sdm_log10(H * 1e-3); }

/* cu.py EqConst.at = trivia.vant_hoff with dH = tdep2enthalpy(dT) */
SDM_MATH_FN double chem_eq_at(const double *k, double K, double dT, double T) {
  const double dH = -dT * k[SDM_CHEM_K_R_STR];
  return K * sdm_exp(-dH / k[SDM_CHEM_K_R_STR] * (1 / T - 1 / k[SDM_CHEM_K_ROOM_TEMP]));
}

/* cu.py KinConst: A = k exp(Ea / (R_str T_0)); at = trivia.arrhenius */
SDM_MATH_FN double chem_kin_at(const double *k, double k0, double dT, double T) {
  const double Ea = -dT * k[SDM_CHEM_K_R_STR];
  const double A = k0 * sdm_exp(Ea / (k[SDM_CHEM_K_R_STR] * k[SDM_CHEM_K_ROOM_TEMP]));
  return A * sdm_exp(-Ea / (k[SDM_CHEM_K_R_STR] * T));
}

/* the 17 temperature-dependent constants of a cell */
typedef struct chem_cell {
  double eq[SDM_CHEM_N_EQ], kin[SDM_CHEM_N_KIN], henry[SDM_CHEM_N_GAS];
} chem_cell;

/* cm.py:292-305 (+ the Henry constants, cm.py:89-91) */
SDM_MATH_FN void chem_cell_data(const double *k, double T, chem_cell *c) {
  for (int e = 0; e < SDM_CHEM_N_EQ; ++e)
    c->eq[e] = chem_eq_at(k, k[SDM_CHEM_K_EQ_K + e], k[SDM_CHEM_K_EQ_DT + e], T);
  for (int e = 0; e < SDM_CHEM_N_KIN; ++e)
    c->kin[e] = chem_kin_at(k, k[SDM_CHEM_K_KIN_K + e], k[SDM_CHEM_K_KIN_DT + e], T);
  for (int g = 0; g < SDM_CHEM_N_GAS; ++g)
    c->henry[g] = chem_eq_at(k, k[SDM_CHEM_K_HENRY_K + g], k[SDM_CHEM_K_HENRY_DT + g], T);
}

/* cu.py DISSOCIATION_FACTORS, gas order; cm.py:282-290 */
SDM_MATH_FN void chem_drop_data(const double *k, const double *eq, double pH, double *df) {
  const double H = chem_pH2H(pH);
  df[SDM_CHEM_GAS_HNO3] = 1 + eq[SDM_CHEM_EQ_HNO3] / H;
  df[SDM_CHEM_GAS_H2O2] = 1;
  df[SDM_CHEM_GAS_NH3] = 1 + eq[SDM_CHEM_EQ_NH3] / k[SDM_CHEM_K_K_H2O] * H;
  df[SDM_CHEM_GAS_SO2] = 1 + eq[SDM_CHEM_EQ_SO2] * (1 / H + eq[SDM_CHEM_EQ_HSO3] / (H * H));
  df[SDM_CHEM_GAS_CO2] = 1 + eq[SDM_CHEM_EQ_CO2] * (1 / H + eq[SDM_CHEM_EQ_HCO3] / (H * H));
  df[SDM_CHEM_GAS_O3] = 1;
}

SDM_MATH_FN void chem_acid_of(const double *k, const double *eq, chem_acid *q) {
  q->NH3 = eq[SDM_CHEM_EQ_NH3]; q->SO2 = eq[SDM_CHEM_EQ_SO2]; q->HSO3 = eq[SDM_CHEM_EQ_HSO3];
  q->HSO4 = eq[SDM_CHEM_EQ_HSO4]; q->HCO3 = eq[SDM_CHEM_EQ_HCO3]; q->CO2 = eq[SDM_CHEM_EQ_CO2];
  q->HNO3 = eq[SDM_CHEM_EQ_HNO3];
  q->K_H2O = k[SDM_CHEM_K_K_H2O];
}

/* cm.py:368-429 for one row; returns 1 where the solve did not converge (all iterations used,
 * or its bracket refused) */
SDM_MATH_FN int chem_equilibrate_row(const chem_acid *q, double H_min, double H_max,
                                     double threshold, double rtol, double *pH, int *flag) {
  double a = chem_pH2H(*pH);
  double fa = chem_acidity_minfun(a, q);
  if (sdm_abs(fa) < 1e-6) return 0;
  double b = sdm_nan(), fb = sdm_nan();
  int use_default_range = 0;
  if (sdm_abs(fa) < 1) {
    b = a * 2;
    fb = chem_acidity_minfun(b, q);
    if (fa * fb > 0) {
      b = a;
      fb = fa;
      a = b / 2 / 2;
      fa = chem_acidity_minfun(a, q);
      if (fa * fb > 0) use_default_range = 1;
    }
  } else {
    use_default_range = 1;
  }
  int max_iter = 8;
  if (use_default_range) {
    a = H_min;
    b = H_max;
    fa = chem_acidity_minfun(a, q);
    fb = chem_acidity_minfun(b, q);
    max_iter = 32;
  }
  int iters;
  const double H = toms748_solve(q, a, b, fa, fb, rtol, max_iter, &iters);
  *pH = chem_H2pH(H);
  *flag = chem_ionic_strength(H, q) <= threshold;
  return iters == max_iter || iters < 0;
}

/* cm.py:131-152 for one row and one gas: the new amount of one real droplet */
SDM_MATH_FN double chem_dissolution_row(const double *k, int g, double mixing_ratio,
                                        double henry, double env_p, double env_T, double dt,
                                        double volume, double moles, double df) {
  const double sg = k[SDM_CHEM_K_MOLAR_MASS + g] * 1e-3 / k[SDM_CHEM_K_MD];
  const double Mc = sg * k[SDM_CHEM_K_MD];
  const double Rc = k[SDM_CHEM_K_R_STR] / Mc;
  const double cinf = env_p / env_T / (k[SDM_CHEM_K_RD] / mixing_ratio + Rc) / Mc;
  const double r_w = sdm_pow(volume / k[SDM_CHEM_K_PI_4_3], k[SDM_CHEM_K_ONE_THIRD]);
  const double v_avg =
      SDM_MATH_SQRT(8 * k[SDM_CHEM_K_R_STR] * env_T / (k[SDM_CHEM_K_PI] * Mc));
  const double dt_over_scale =
      dt / (4 * r_w / (3 * v_avg * k[SDM_CHEM_K_ACCOMMODATION + g]) +
            r_w * r_w / (3 * k[SDM_CHEM_K_DIFFUSION + g]));
  const double A_old = moles / volume;
  const double H_eff = henry * df;
  const double A_new = (A_old + dt_over_scale * cinf) /
                       (1 + dt_over_scale / H_eff / k[SDM_CHEM_K_R_STR] / env_T);
  return A_new * volume;
}

/* cm.py:153: delta_mr of a cell and a gas */
SDM_MATH_FN double chem_delta_mr(const double *k, int g, double taken, double dv, double rhod) {
  const double sg = k[SDM_CHEM_K_MOLAR_MASS + g] * 1e-3 / k[SDM_CHEM_K_MD];
  return taken * sg * k[SDM_CHEM_K_MD] / (dv * rhod);
}

/* cm.py:233-280 for one flagged row */
SDM_MATH_FN void chem_oxidation_row(const double *k, const double *kin, const double *eq,
                                    double dt, double volume, double pH, double df_SO2,
                                    double *m_O3, double *m_H2O2, double *m_S_IV,
                                    double *m_S_VI) {
  const double H = chem_pH2H(pH);
  const double K_SO2 = eq[SDM_CHEM_EQ_SO2], K_HSO3 = eq[SDM_CHEM_EQ_HSO3];
  const double SO2aq = *m_S_IV / volume / df_SO2;
  const double ozone =
      (kin[0] + (kin[1] * K_SO2 / H) + (kin[2] * K_SO2 * K_HSO3 / (H * H))) * (*m_O3 / volume) *
      SO2aq;
  const double peroxide =
      kin[3] * K_SO2 / (1 + k[SDM_CHEM_K_K4] * H) * (*m_H2O2 / volume) * SO2aq;
  const double dt_times_volume = dt * volume;
  const double d_O3 = -ozone, d_S_IV = -(ozone + peroxide), d_H2O2 = -peroxide,
               d_S_VI = ozone + peroxide;
  if (*m_O3 + d_O3 * dt_times_volume < 0 || *m_S_IV + d_S_IV * dt_times_volume < 0 ||
      *m_S_VI + d_S_VI * dt_times_volume < 0 || *m_H2O2 + d_H2O2 * dt_times_volume < 0)
    return;
  *m_O3 = *m_O3 + dt_times_volume * d_O3;
  *m_S_IV = *m_S_IV + dt_times_volume * d_S_IV;
  *m_S_VI = *m_S_VI + dt_times_volume * d_S_VI;
  *m_H2O2 = *m_H2O2 + dt_times_volume * d_H2O2;
}

/* gas g dissolves into the aqueous column chem_aq_of_gas(g) (cu.py GASEOUS_COMPOUNDS) */
SDM_MATH_FN int chem_aq_of_gas(int g) {
  return g == SDM_CHEM_GAS_HNO3   ? SDM_CHEM_AQ_N_V
         : g == SDM_CHEM_GAS_H2O2 ? SDM_CHEM_AQ_H2O2
         : g == SDM_CHEM_GAS_NH3  ? SDM_CHEM_AQ_N_MIII
         : g == SDM_CHEM_GAS_SO2  ? SDM_CHEM_AQ_S_IV
         : g == SDM_CHEM_GAS_CO2  ? SDM_CHEM_AQ_C_IV
                                  : SDM_CHEM_AQ_O3;
}

/* one super-droplet in registers through the sub-steps of sdm_chemistry_step */
typedef struct chem_drop {
  double m[SDM_CHEM_N_AQ], pH, volume;
  int flag;
} chem_drop;

SDM_MATH_FN int chem_solve_drop(const double *k, const chem_cell *c, double H_min, double H_max,
                                double threshold, double rtol, chem_drop *d) {
  chem_acid q;
  chem_acid_of(k, c->eq, &q);
  /* attributes/chemistry/concentration.py: conc = moles / volume */
  q.N_mIII = d->m[SDM_CHEM_AQ_N_MIII] / d->volume;
  q.N_V = d->m[SDM_CHEM_AQ_N_V] / d->volume;
  q.C_IV = d->m[SDM_CHEM_AQ_C_IV] / d->volume;
  q.S_IV = d->m[SDM_CHEM_AQ_S_IV] / d->volume;
  q.S_VI = d->m[SDM_CHEM_AQ_S_VI] / d->volume;
  return chem_equilibrate_row(&q, H_min, H_max, threshold, rtol, &d->pH, &d->flag);
}

/* one half of a sub-step of sdm_chemistry_step for one row: which == 0 is points 1-3 of the
 * header's definition (solve, drop data, dissolution), which == 1 points 4-6 (solve, drop data,
 * oxidation).  One function for both so that a kernel holds the solver once.  mr: the cell's six
 * mixing ratios at the start of the sub-step; dq: multiplicity * (new - old) of the six gases,
 * written where *took is set; counts[0] += failed solves, counts[1] += negative amounts */
SDM_MATH_FN void chem_half(const double *k, const chem_cell *c, const double *mr, double env_p,
                           double env_T, double dt, double H_min, double H_max, double threshold,
                           double rtol, double multiplicity, chem_drop *d, int which, double *dq,
                           int *took, int64_t *counts) {
  double df[SDM_CHEM_N_GAS];
  counts[0] += chem_solve_drop(k, c, H_min, H_max, threshold, rtol, d);
  chem_drop_data(k, c->eq, d->pH, df);
  if (which == 0) {
    *took = d->flag;
    if (d->flag) {
#pragma unroll
      for (int g = 0; g < SDM_CHEM_N_GAS; ++g) {
        const int aq = chem_aq_of_gas(g);
        const double old = d->m[aq];
        const double now = chem_dissolution_row(k, g, mr[g], c->henry[g], env_p, env_T, dt,
                                                d->volume, old, df[g]);
        if (!(now >= 0)) counts[1] += 1;
        dq[g] = multiplicity * (now - old);
        d->m[aq] = now;
      }
    }
  } else if (d->flag) {
    chem_oxidation_row(k, c->kin, c->eq, dt, d->volume, d->pH, df[SDM_CHEM_GAS_SO2],
                       &d->m[SDM_CHEM_AQ_O3], &d->m[SDM_CHEM_AQ_H2O2], &d->m[SDM_CHEM_AQ_S_IV],
                       &d->m[SDM_CHEM_AQ_S_VI]);
  }
}

#endif /* SDM_CHEMISTRY_ROWS_H */

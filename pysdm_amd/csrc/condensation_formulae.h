/*
 * condensation_formulae.h -- every choice of the condensation path's formulae options
 * (include/sdm_condensation_formulae.h) as a function of scalars, for both compilers of this
 * project: hipcc (condensation_formulae.hip, the general instantiation of the solver) and gcc (the
 * CPU checker, tests/condensation_formulae_checker/).
 *
 * Each function is the reference's PySDM/physics/<option>/<choice>.py with a switch on the
 * descriptor's code for that option (uniform over a kernel: the descriptor is a kernel argument).
 * Python evaluates left to right and every expression below keeps that order; the translation
 * units that include this are compiled without contraction.  `x ** y` and np.power are sdm_pow
 * (whose y == 2 and y == 0.5 cases are the exact square and the correctly rounded root), exp and
 * log are sdm_exp / sdm_log, and tanh (MurphyKoop2005) is built from sdm_exp here: no libm call.
 *
 * One deliberate difference: CompressedFilmRuehl.sigma asserts that its inner TOMS748 search did
 * not use up its 100 iterations (`assert iters != max_iters`).  Here nothing traps: cf_sigma sets
 * *fail, the condensation solver counts the droplet as failed (success[c] = 0, as for a failed
 * bracket of its own search) and sdm_critical_volume_f writes NaN.
 *
 * The includer defines CF_FN (the qualifiers of every function) before the #include and has
 * included sdm_math.h and the two condensation headers.
 */
#ifndef SDM_CONDENSATION_FORMULAE_IMPL_H
#define SDM_CONDENSATION_FORMULAE_IMPL_H

typedef struct cf_k {
  double c[SDM_COND_N_CONSTS];   /* SDM_COND_K_* */
  double f[SDM_COND_F_N_CONSTS]; /* SDM_COND_F_* */
  int32_t o[10];                 /* SDM_COND_OPT_* */
} cf_k;

/* how many choices each option has (SDM_COND_OPT_* order): a code outside [0, n) is refused */
#define CF_N_CHOICES {2, 6, 3, 2, 3, 4, 4, 4, 3}

#define CF_C(name) (k->c[SDM_COND_K_##name])
#define CF_F(name) (k->f[SDM_COND_F_##name])
#define CF_O(name) (k->o[SDM_COND_OPT_##name])

/* Python's max(x, y) / min(x, y): the first argument unless the second is strictly larger /
 * smaller; np.maximum / np.minimum: the same for numbers, NaN if either is NaN */
CF_FN double cf_py_max(double x, double y) { return y > x ? y : x; }
CF_FN double cf_py_min(double x, double y) { return y < x ? y : x; }
CF_FN double cf_np_max(double x, double y) { return (x != x || x >= y) ? x : y; }
CF_FN double cf_np_min(double x, double y) { return (x != x || x <= y) ? x : y; }

/* np.tanh from sdm_exp: (1 - e) / (1 + e) with e = exp of -2 |y| */
CF_FN double cf_tanh(double y) {
  if (y != y) return y;
  const double e = sdm_exp(-2 * sdm_abs(y));
  const double t = (1 - e) / (1 + e);
  return y < 0 ? -t : t;
}

/* ---- diffusion_coordinate: water_mass_logarithm.py, water_mass.py ---------------------------- */
CF_FN double cf_x(const cf_k *k, double mass) {
  return CF_O(DIFFUSION_COORDINATE) == SDM_COND_COORD_WATER_MASS ? mass : sdm_log(mass);
}
CF_FN double cf_mass(const cf_k *k, double x) {
  return CF_O(DIFFUSION_COORDINATE) == SDM_COND_COORD_WATER_MASS ? x : sdm_exp(x);
}
CF_FN double cf_dx_dt(const cf_k *k, double m, double dm_dt) {
  return CF_O(DIFFUSION_COORDINATE) == SDM_COND_COORD_WATER_MASS ? dm_dt : dm_dt / m;
}
CF_FN double cf_x_max(const cf_k *k) { /* const.ONE / const.ZERO */
  return CF_O(DIFFUSION_COORDINATE) == SDM_COND_COORD_WATER_MASS ? 1.0 : 0.0;
}

/* ---- saturation_vapour_pressure (pvs_water) --------------------------------------------------- */
CF_FN double cf_pvs_water(const cf_k *k, double T) {
  const double T0 = CF_C(T0);
  switch (CF_O(SATURATION_VAPOUR_PRESSURE)) {
    case SDM_COND_PVS_AUGUST_ROCHE_MAGNUS: { /* august_roche_magnus.py:13-16 */
      const double *C = &CF_F(ARM_C1);
      return C[0] * sdm_exp((C[1] * (T - T0)) / ((T - T0) + C[2]));
    }
    case SDM_COND_PVS_BOLTON_1980: { /* bolton_1980.py:13-17 */
      const double *G = &CF_F(B80W_G0);
      return G[0] * sdm_exp((G[1] * (T - T0)) / ((T - T0) + G[2]));
    }
    case SDM_COND_PVS_LOWE_1977: { /* lowe1977.py:12-28 */
      const double *A = &CF_F(L77W_A0);
      const double d = T - T0;
      return A[0] + d * (A[1] + d * (A[2] + d * (A[3] + d * (A[4] + d * (A[5] + d * (A[6]))))));
    }
    case SDM_COND_PVS_MURPHY_KOOP_2005: { /* murphy_koop_2005.py:13-27; C[i] is MK05_LIQ_C(i+1) */
      const double *C = &CF_F(MK05_LIQ_C1);
      return C[0] * sdm_exp(C[1] - C[2] / (T) - C[3] * sdm_log(T / C[4]) + C[5] * (T) +
                            cf_tanh(C[6] * (T - C[7])) *
                                (C[8] - C[9] / T - C[10] * sdm_log(T / C[11]) + C[12] * T));
    }
    case SDM_COND_PVS_WEXLER_1976: { /* wexler_1976.py:13-26 */
      const double *G = &CF_F(W76W_G0);
      return sdm_exp(G[0] / sdm_pow(T, 2.0) + G[1] / T + G[2] + G[3] * T +
                     G[4] * sdm_pow(T, 2.0) + G[5] * sdm_pow(T, 3.0) + G[6] * sdm_pow(T, 4.0) +
                     G[7] * sdm_log(T / CF_F(ONE_KELVIN))) *
             G[8];
    }
    default: { /* flatau_walko_cotton.py:12-39 */
      const double d = T - T0;
      const double *C = &CF_C(FWC_C0);
      return C[0] + d * (C[1] + d * (C[2] + d * (C[3] + d * (C[4] + d * (C[5] + d * (C[6] +
             d * (C[7] + d * C[8])))))));
    }
  }
}

/* ---- latent_heat_vapourisation: kirchhoff.py, constant.py, seinfeld_and_pandis_2010.py -------- */
CF_FN double cf_lv(const cf_k *k, double T) {
  switch (CF_O(LATENT_HEAT_VAPOURISATION)) {
    case SDM_COND_LV_CONSTANT:
      return CF_C(L_TRI);
    case SDM_COND_LV_LOWE_2019:
      return CF_C(L_TRI) * sdm_pow(CF_C(T_TRI) / T, CF_F(L_L19_A) + CF_F(L_L19_B) * T);
    default:
      return CF_C(L_TRI) + (CF_C(C_PV) - CF_C(C_PW)) * (T - CF_C(T_TRI));
  }
}

/* ---- diffusion_thermics: neglect.py, tracy_welch_porter.py, lowe_et_al_2019.py (D of
 * seinfeld_and_pandis_2010.py), grabowski_et_al_2011.py -------------------------------------- */
CF_FN double cf_thermics_D(const cf_k *k, double T, double p) {
  switch (CF_O(DIFFUSION_THERMICS)) {
    case SDM_COND_THERM_TRACY_WELCH_PORTER:
      return CF_C(D0) * sdm_pow(T / CF_C(T0), CF_F(D_EXP)) * (CF_C(P1000) / p);
    case SDM_COND_THERM_LOWE_ET_AL_2019:
      return CF_F(D_L19_A) * (CF_F(P_STP) / p) * sdm_pow(T / CF_C(T0), CF_F(D_L19_B));
    case SDM_COND_THERM_GRABOWSKI_ET_AL_2011: {
      const double *D = &CF_F(D_G11_A);
      return D[0] * (D[1] * T + D[2]);
    }
    default:
      return CF_C(D0);
  }
}
CF_FN double cf_thermics_K(const cf_k *k, double T, double p) {
  (void)p;
  switch (CF_O(DIFFUSION_THERMICS)) {
    case SDM_COND_THERM_LOWE_ET_AL_2019:
      return CF_F(K_L19_A) * (CF_F(K_L19_B) + CF_F(K_L19_C) * T);
    case SDM_COND_THERM_GRABOWSKI_ET_AL_2011: {
      const double *K = &CF_F(K_G11_A);
      return K[0] * sdm_pow(T, 3.0) + K[1] * sdm_pow(T, 2.0) + K[2] * T + K[3];
    }
    default: /* Neglect, TracyWelchPorter */
      return CF_C(K0);
  }
}

/* ---- diffusion_kinetics: fuchs_sutugin.py, neglect.py, pruppacher_and_klett_2005.py (which
 * LoweEtAl2019 and GrabowskiEtAl2011 are) ---------------------------------------------------- */
CF_FN double cf_lambdaD(const cf_k *k, double D, double T) {
  if (CF_O(DIFFUSION_KINETICS) == SDM_COND_KIN_NEGLECT) return -1;
  return D / SDM_MATH_SQRT(2 * CF_C(RV) * T);
}
CF_FN double cf_lambdaK(const cf_k *k, double T, double p) {
  if (CF_O(DIFFUSION_KINETICS) != SDM_COND_KIN_FUCHS_SUTUGIN) return -1;
  return (4.0 / 5) * CF_C(K0) * T / p / SDM_MATH_SQRT(2 * CF_C(RD) * T);
}
CF_FN double cf_kinetics_D(const cf_k *k, double D, double r, double lmbd) {
  switch (CF_O(DIFFUSION_KINETICS)) {
    case SDM_COND_KIN_NEGLECT:
      return D;
    case SDM_COND_KIN_LOWE_ET_AL_2019:
    case SDM_COND_KIN_GRABOWSKI_ET_AL_2011:
      return D / ((r / (r + CF_F(DV_PK05))) + 2 * SDM_MATH_SQRT(CF_C(PI)) * lmbd / r / CF_C(MAC));
    default:
      return D * (1 + lmbd / r) /
             (1 + (4.0 / 3 / CF_C(MAC) + 0.377) * lmbd / r +
              (4.0 / 3 / CF_C(MAC)) * lmbd / r * lmbd / r);
  }
}
CF_FN double cf_kinetics_K(const cf_k *k, double K, double r, double lmbd) {
  if (CF_O(DIFFUSION_KINETICS) != SDM_COND_KIN_FUCHS_SUTUGIN) return K;
  return K * (1 + lmbd / r) /
         (1 + (4.0 / 3 / CF_C(HAC) + 0.377) * lmbd / r +
          (4.0 / 3 / CF_C(HAC)) * lmbd / r * lmbd / r);
}

/* ---- ventilation: neglect.py, froessling_1938.py, pruppacher_rasmussen_1979.py; the argument is
 * trivia.sqrt_re_times_cbrt_sc of trivia.air_schmidt_number (trivia.py:142-147) ---------------- */
CF_FN double cf_air_schmidt_number(double dynamic_viscosity, double diffusivity, double density) {
  return dynamic_viscosity / diffusivity / density;
}
CF_FN double cf_ventilation_factor(const cf_k *k, double Re, double Sc) {
  if (CF_O(VENTILATION) == SDM_COND_VENT_NEGLECT) return 1.0; /* np.power(anything, 0) */
  const double x = sdm_pow(Re, CF_F(ONE_HALF)) * sdm_pow(Sc, CF_C(ONE_THIRD));
  if (CF_O(VENTILATION) == SDM_COND_VENT_FROESSLING_1938)
    return CF_F(FROESSLING_1938_A) + CF_F(FROESSLING_1938_B) * x;
  /* np.where(x < XTHRES, small, big): NaN takes the second branch */
  if (x < CF_F(PR79_XTHRES))
    return CF_F(PR79_CONSTSMALL) + CF_F(PR79_COEFFSMALL) * sdm_pow(x, CF_F(PR79_POWSMALL));
  return CF_F(PR79_CONSTBIG) + CF_F(PR79_COEFFBIG) * x;
}

/* ---- drop_growth: mason_1971.py, howell_1949.py, fick.py ------------------------------------- */
CF_FN double cf_Fk(const cf_k *k, double T, double K, double lv) {
  switch (CF_O(DROP_GROWTH)) {
    case SDM_COND_GROWTH_FICK:
      return 0;
    case SDM_COND_GROWTH_HOWELL_1949:
      return CF_C(RHO_W) * lv / T / K * (lv / T / CF_C(RV));
    default:
      return CF_C(RHO_W) * lv / T / K * (lv / T / CF_C(RV) - 1);
  }
}
CF_FN double cf_Fd(const cf_k *k, double T, double D, double pvs) {
  return CF_C(RHO_W) * CF_C(RV) * T / D / pvs;
}
CF_FN double cf_r_dr_dt(const cf_k *k, double RH_eq, double RH, double Fk, double Fd) {
  if (CF_O(DROP_GROWTH) == SDM_COND_GROWTH_FICK) return (RH - RH_eq) / Fd;
  return (RH - RH_eq) / (Fk + Fd);
}

/* ---- hygroscopicity: kappa_koehler_leading_terms.py, kappa_koehler.py ------------------------- */
CF_FN double cf_RH_eq(const cf_k *k, double r, double T, double kp, double rd3, double sgm) {
  if (CF_O(HYGROSCOPICITY) == SDM_COND_HYGRO_KAPPA_KOEHLER)
    return sdm_exp((2 * sgm / CF_C(RV) / T / CF_C(RHO_W)) / r) * (sdm_pow(r, 3.0) - rd3) /
           (sdm_pow(r, 3.0) - rd3 * (1 - kp));
  return 1 + (2 * sgm / CF_C(RV) / T / CF_C(RHO_W)) / r - kp * rd3 / sdm_pow(r, CF_C(THREE));
}
CF_FN double cf_r_cr(const cf_k *k, double kp, double rd3, double T, double sgm) {
  return SDM_MATH_SQRT(3 * kp * rd3 / (2 * sgm / CF_C(RV) / T / CF_C(RHO_W))); /* both choices */
}

/* ---- surface_tension --------------------------------------------------------------------------- */
/* compressed_film_ruehl.py:14-18 */
typedef struct cf_ruehl_args { double Cb_iso, C0, A0, A_iso, c; } cf_ruehl_args;
CF_FN double cf_ruehl_minfun(double f_surf, const cf_ruehl_args *a) {
  const double lhs = a->Cb_iso * (1 - f_surf) / a->C0;
  const double rhs = sdm_exp(a->c * (sdm_pow(a->A0, 2.0) - sdm_pow(a->A_iso / f_surf, 2.0)));
  return lhs - rhs;
}
#define TOMS748_FN CF_FN
#define TOMS748_ARGS cf_ruehl_args
#define TOMS748_EVAL(x, args) cf_ruehl_minfun((x), (args))
#include "toms748.h"
#define CF_RUEHL_RTOL 1e-6
#ifndef CF_RUEHL_MAX_ITERS /* (a test builds the checker with a smaller cap to reach the exit) */
#define CF_RUEHL_MAX_ITERS 100
#endif
#define CF_RUEHL_BRACKET_A 1e-16
#define CF_RUEHL_BRACKET_B 1.0

/* sigma(T, v_wet, v_dry, f_org); *fail is set (never cleared) where CompressedFilmRuehl's search
 * uses up its iterations */
CF_FN double cf_sigma(const cf_k *k, double T, double v_wet, double v_dry, double f_org,
                      int *fail) {
  switch (CF_O(SURFACE_TENSION)) {
    case SDM_COND_SGM_COMPRESSED_FILM_OVADNEVAITE: { /* compressed_film_ovadnevaite.py:24-31 */
      const double r_wet = sdm_pow((3 * v_wet) / (4 * CF_C(PI)), 1.0 / 3);
      const double v_delta =
          v_wet - ((4 * CF_C(PI)) / 3 * sdm_pow(r_wet - CF_F(DELTA_MIN), 3.0));
      const double v_beta = f_org * v_dry;
      const double c_beta = cf_np_min(v_beta / v_delta, 1.0);
      return (1 - c_beta) * CF_C(SGM_W) + c_beta * CF_F(SGM_ORG);
    }
    case SDM_COND_SGM_SZYSZKOWSKI_LANGMUIR: { /* szyszkowski_langmuir.py:28-58 */
      const double r_wet = sdm_pow((3 * v_wet) / (4 * CF_C(PI)), 1.0 / 3);
      double sgm;
      if (f_org == 0) {
        sgm = CF_C(SGM_W);
      } else {
        const double Cb_iso =
            (f_org * v_dry / CF_F(RUEHL_NU_ORG)) / (v_wet / CF_F(WATER_MOLAR_VOLUME));
        const double A_iso = (4 * CF_C(PI) * sdm_pow(r_wet, 2.0)) /
                             (f_org * v_dry * CF_F(N_A) / CF_F(RUEHL_NU_ORG));
        const double a = -CF_F(RUEHL_A0) / A_iso;
        const double b = (CF_F(RUEHL_A0) / A_iso +
                          (CF_F(RUEHL_A0) / A_iso) * (CF_F(RUEHL_C0) / Cb_iso) + 1);
        const double c = -1;
        const double f_surf = (-b + SDM_MATH_SQRT(sdm_pow(b, 2.0) - 4 * a * c)) / (2 * a);
        sgm = CF_C(SGM_W) - ((CF_F(R_STR) * T) / (CF_F(RUEHL_A0) * CF_F(N_A))) *
                                sdm_log(1 + Cb_iso * (1 - f_surf) / CF_F(RUEHL_C0));
      }
      return cf_py_min(cf_py_max(sgm, CF_F(RUEHL_SGM_MIN)), CF_C(SGM_W));
    }
    case SDM_COND_SGM_COMPRESSED_FILM_RUEHL: { /* compressed_film_ruehl.py:48-87 */
      const double r_wet = sdm_pow((3 * v_wet) / (4 * CF_C(PI)), 1.0 / 3);
      double sgm;
      if (f_org == 0) {
        sgm = CF_C(SGM_W);
      } else if (f_org == 1) {
        sgm = CF_F(RUEHL_SGM_MIN);
      } else {
        cf_ruehl_args a;
        a.Cb_iso = (f_org * v_dry / CF_F(RUEHL_NU_ORG)) / (v_wet / CF_F(WATER_MOLAR_VOLUME));
        a.A_iso = (4 * CF_C(PI) * sdm_pow(r_wet, 2.0)) /
                  (f_org * v_dry * CF_F(N_A) / CF_F(RUEHL_NU_ORG));
        a.c = (CF_F(RUEHL_M_SIGMA) * CF_F(N_A)) / (2 * CF_F(R_STR) * T);
        a.C0 = CF_F(RUEHL_C0);
        a.A0 = CF_F(RUEHL_A0);
        int iters;
        const double f_surf = toms748_solve(
            &a, CF_RUEHL_BRACKET_A, CF_RUEHL_BRACKET_B, cf_ruehl_minfun(CF_RUEHL_BRACKET_A, &a),
            cf_ruehl_minfun(CF_RUEHL_BRACKET_B, &a), CF_RUEHL_RTOL, CF_RUEHL_MAX_ITERS, &iters);
        if (iters == CF_RUEHL_MAX_ITERS) *fail = 1; /* the reference's assert */
        sgm = CF_C(SGM_W) - (CF_F(RUEHL_A0) - a.A_iso / f_surf) * CF_F(RUEHL_M_SIGMA);
      }
      return cf_np_min(cf_np_max(sgm, CF_F(RUEHL_SGM_MIN)), CF_C(SGM_W));
    }
    default: /* constant.py */
      return CF_C(SGM_W);
  }
}

/* ---- what the formulae above are combined into (the solver and the checker share these) ------- */
/* trivia.py:19-20,27-28 */
CF_FN double cf_radius(const cf_k *k, double volume) {
  return sdm_pow(volume / CF_C(PI_4_3), CF_C(ONE_THIRD));
}
CF_FN double cf_volume(const cf_k *k, double radius) {
  return CF_C(PI_4_3) * sdm_pow(radius, CF_C(THREE));
}
/* state_variable_triplet/libcloudphplusplus.py:14-40 */
CF_FN double cf_svt_T(const cf_k *k, double rhod, double thd) {
  return thd * sdm_pow(rhod * thd / CF_C(P1000) * CF_C(RD),
                       CF_C(RD_OVER_C_PD) / (1 - CF_C(RD_OVER_C_PD)));
}
CF_FN double cf_svt_p(const cf_k *k, double rhod, double T, double qv) {
  return rhod * (1 + qv) * (CF_C(RV) / (1 / qv + 1) + CF_C(RD) / (1 + qv)) * T;
}
CF_FN double cf_svt_pv(const cf_k *k, double p, double qv) { return p * qv / (qv + CF_C(EPS)); }

#endif /* SDM_CONDENSATION_FORMULAE_IMPL_H */

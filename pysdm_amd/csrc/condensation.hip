// condensation.hip -- PySDM's condensation solver (include/sdm_condensation.h) for gfx950: the
// instantiation of condensation_solver.h (where the kernel's design is described) with PySDM's
// default formulae inlined, and the elementwise ambient methods.
//
// Reference: PySDM/backends/impl_numba/methods/condensation_methods.py ("cm.py"), toms748.py and
// physics_methods.py ("pm.py"), with PySDM's default formulae inlined (physics/...).  The CPU
// checker of this file is tests/checker/condensation_checker.c.
#include "parcel_solver.h"
#include "../../include/sdm_condensation.h"

#define GRID1D(n) dim3(grid_for(n)), dim3(SDM_BLOCK), 0, ctx->stream

namespace {

struct Kc {
  double rho_w, Rv, Rd, c_pd, c_pv, c_pw, l_tri, T_tri, T0, p1000, eps, sgm_w, D0, K0, MAC, HAC,
      PI, PI_4_3, Rd_over_c_pd, ONE_THIRD, THREE, FWC[9], Z3, Z2, Z1, Z0;
};

Kc consts_of(const double *c) {
  Kc k;
  k.rho_w = c[SDM_COND_K_RHO_W]; k.Rv = c[SDM_COND_K_RV]; k.Rd = c[SDM_COND_K_RD];
  k.c_pd = c[SDM_COND_K_C_PD]; k.c_pv = c[SDM_COND_K_C_PV]; k.c_pw = c[SDM_COND_K_C_PW];
  k.l_tri = c[SDM_COND_K_L_TRI]; k.T_tri = c[SDM_COND_K_T_TRI]; k.T0 = c[SDM_COND_K_T0];
  k.p1000 = c[SDM_COND_K_P1000]; k.eps = c[SDM_COND_K_EPS]; k.sgm_w = c[SDM_COND_K_SGM_W];
  k.D0 = c[SDM_COND_K_D0]; k.K0 = c[SDM_COND_K_K0]; k.MAC = c[SDM_COND_K_MAC];
  k.HAC = c[SDM_COND_K_HAC]; k.PI = c[SDM_COND_K_PI]; k.PI_4_3 = c[SDM_COND_K_PI_4_3];
  k.Rd_over_c_pd = c[SDM_COND_K_RD_OVER_C_PD]; k.ONE_THIRD = c[SDM_COND_K_ONE_THIRD];
  k.THREE = c[SDM_COND_K_THREE];
  for (int i = 0; i < 9; ++i) k.FWC[i] = c[SDM_COND_K_FWC_C0 + i];
  k.Z3 = c[SDM_COND_K_ZOGRAFOS_T3]; k.Z2 = c[SDM_COND_K_ZOGRAFOS_T2];
  k.Z1 = c[SDM_COND_K_ZOGRAFOS_T1]; k.Z0 = c[SDM_COND_K_ZOGRAFOS_T0];
  return k;
}

// ---- default formulae (Python's left-to-right order kept in every expression) ------------------
// state_variable_triplet/libcloudphplusplus.py
DF double svt_T(const Kc &k, double rhod, double thd) {
  return thd * sdm_pow(rhod * thd / k.p1000 * k.Rd, k.Rd_over_c_pd / (1 - k.Rd_over_c_pd));
}
DF double svt_p(const Kc &k, double rhod, double T, double qv) {
  return rhod * (1 + qv) * (k.Rv / (1 / qv + 1) + k.Rd / (1 + qv)) * T;
}
DF double svt_pv(const Kc &k, double p, double qv) { return p * qv / (qv + k.eps); }
DF double lv_of(const Kc &k, double T) { return k.l_tri + (k.c_pv - k.c_pw) * (T - k.T_tri); }
DF double pvs_water(const Kc &k, double T) {  // flatau_walko_cotton.py
  const double d = T - k.T0;
  const double *C = k.FWC;
  return C[0] + d * (C[1] + d * (C[2] + d * (C[3] + d * (C[4] + d * (C[5] + d * (C[6] +
         d * (C[7] + d * C[8])))))));
}
DF double radius_of(const Kc &k, double v) { return sdm_pow(v / k.PI_4_3, k.ONE_THIRD); }
DF double RH_eq_of(const Kc &k, double r, double T, double kp, double rd3, double sgm) {
  return 1 + (2 * sgm / k.Rv / T / k.rho_w) / r - kp * rd3 / sdm_pow(r, k.THREE);
}

// pm.py:53-61: what k_temperature_pressure_rh writes for one cell and the parcel kernel for a parcel
DF void tprh_of(const Kc &k, double rhod, double thd, double qv, double &T, double &p, double &RH) {
  T = svt_T(k, rhod, thd);
  p = svt_p(k, rhod, T, qv);
  RH = svt_pv(k, p, qv) / pvs_water(k, T);
}
// pm.py:22-33; kappa_koehler_leading_terms.py:23-25 (r_cr), trivia.py:27-28 (volume): what
// k_critical_volume writes for one droplet and the parcel kernel for a row
DF double critical_volume_of(const Kc &k, double kappa, double v_dry, double t) {
  const double sgm = k.sgm_w;
  const double r_cr = SDM_MATH_SQRT(3 * kappa * (v_dry / k.PI_4_3) / (2 * sgm / k.Rv / t / k.rho_w));
  return k.PI_4_3 * sdm_pow(r_cr, k.THREE);
}

// the policy of condensation_solver.h (and parcel_solver.h) for PySDM's default formulae
struct DefaultFormulae {
  using K = Kc;
  struct Extra {};  // surface_tension Constant reads no f_org, ventilation Neglect no Re
  static constexpr int STAGE = 0;
  struct MinArgs {
    double x_old, timestep, kappa, rd3, T, RH, Fk, Fd;
  };
  struct Cellwide {  // the sub-step's cell scalars (uniform)
    double T, RH, lv, pvs, DTp, KTp, lambdaK, lambdaD, timestep, rtol_x, RH_rtol;
    int max_iters;
  };
  DF static double rho_w(const Kc &k) { return k.rho_w; }
  DF static double c_pd(const Kc &k) { return k.c_pd; }
  DF static double pi_4_3(const Kc &k) { return k.PI_4_3; }
  DF static double x_of(const Kc &, double m) { return sdm_log(m); }  // water_mass_logarithm.py
  DF static double mass_of(const Kc &, double x) { return sdm_exp(x); }
  DF static bool failed(const MinArgs &) { return false; }
  // parcel_solver.h
  DF static double Rv(const Kc &k) { return k.Rv; }
  DF static double Rd(const Kc &k) { return k.Rd; }
  DF static double c_pv(const Kc &k) { return k.c_pv; }
  DF static double lv(const Kc &k, double T) { return lv_of(k, T); }
  DF static void tprh(const Kc &k, double rhod, double thd, double qv, double &T, double &p,
                      double &RH) {
    tprh_of(k, rhod, thd, qv, T, p, RH);
  }
  DF static double critical_volume(const Kc &k, int64_t, double kappa, double v_dry, double,
                                   double T) {  // surface_tension Constant: no v_wet, no f_org
    return critical_volume_of(k, kappa, v_dry, T);
  }

  // minfun, cm.py:366-397
  DF static double minfun(const Kc &k, double x_new, const MinArgs &a) {
    if (x_new > 0.0) return a.x_old - x_new;  // x_max = ZERO (water_mass_logarithm.py)
    const double mass_new = sdm_exp(x_new);
    const double volume_new = mass_new / k.rho_w;
    const double r_new = radius_of(k, volume_new);
    const double RH_eq = RH_eq_of(k, r_new, a.T, a.kappa, a.rd3, k.sgm_w);
    const double r_dr_dt = (a.RH - RH_eq) / (a.Fk + a.Fd);
    const double dm_dt = 4 * k.PI * k.rho_w * r_new * r_dr_dt;
    return a.x_old - x_new + a.timestep * (dm_dt / mass_new);
  }

  // step_impl's cell scalars, cm.py:288-297,429-430
  DF static void cellwide(const CondArgs<DefaultFormulae> &g, int64_t, double rhod, double thd,
                          double qv, Cellwide &w) {
    const Kc &k = g.k;
    w.T = svt_T(k, rhod, thd);
    const double p = svt_p(k, rhod, w.T, qv);
    const double pv = svt_pv(k, p, qv);
    w.lv = lv_of(k, w.T);
    w.pvs = pvs_water(k, w.T);
    w.DTp = k.D0;  // diffusion_thermics/neglect.py
    w.KTp = k.K0;
    w.RH = pv / w.pvs;
    // fuchs_sutugin.py:14-18
    w.lambdaK = (4.0 / 5) * k.K0 * w.T / p / SDM_MATH_SQRT(2 * k.Rd * w.T);
    w.lambdaD = w.DTp / SDM_MATH_SQRT(2 * k.Rv * w.T);
  }

  // cm.py:434-491
  DF static void start(const Kc &k, const Cellwide &w, double m, double rd3, double kappa, Extra,
                       MinArgs &args, double &x_old, double &dx_old) {
    const double v_drop = m / k.rho_w;
    x_old = sdm_log(m);
    const double r_old = radius_of(k, v_drop);
    const double RH_eq = RH_eq_of(k, r_old, w.T, kappa, rd3, k.sgm_w);
    dx_old = 0.0;
    args = {x_old, w.timestep, kappa, rd3, w.T, w.RH, 0, 0};
    if (!within_tolerance(sdm_abs(w.RH - RH_eq), w.RH, w.RH_rtol)) {
      const double lD = w.lambdaD, lK = w.lambdaK;  // fuchs_sutugin.py:20-44
      const double Dr = w.DTp * (1 + lD / r_old) /
                        (1 + (4.0 / 3 / k.MAC + 0.377) * lD / r_old +
                         (4.0 / 3 / k.MAC) * lD / r_old * lD / r_old);
      const double Kr = w.KTp * (1 + lK / r_old) /
                        (1 + (4.0 / 3 / k.HAC + 0.377) * lK / r_old +
                         (4.0 / 3 / k.HAC) * lK / r_old * lK / r_old);
      // ventilation Neglect: factor 1; mason_1971.py (Fk), fick.py (Fd)
      args.Fk = k.rho_w * w.lv / w.T / (Kr * 1.0) * (w.lv / w.T / k.Rv - 1);
      args.Fd = k.rho_w * k.Rv * w.T / (Dr * 1.0) / w.pvs;
      const double r_dr_dt_old = (w.RH - RH_eq) / (args.Fk + args.Fd);
      const double mass_old = sdm_exp(x_old);
      const double dm_dt_old = 4 * k.PI * k.rho_w * r_old * r_dr_dt_old;
      dx_old = w.timestep * (dm_dt_old / mass_old);
    }
  }
};

__global__ __launch_bounds__(COND_CB) void k_condensation(CondArgs<DefaultFormulae> g) {
  condensation_cell<DefaultFormulae>(g);
}

// include/sdm_parcel.h with PySDM's default formulae: one workgroup per parcel, the launch's time
// steps inside (parcel_solver.h)
__global__ __launch_bounds__(COND_CB) void k_parcel(ParcelArgs<DefaultFormulae> a) {
  parcel_steps<DefaultFormulae>(a);
}

// include/sdm_parcel_diag.h: the same loop with the request table evaluated after every step, and
// the table on given columns
__global__ __launch_bounds__(COND_CB) void k_parcel_d(ParcelArgs<DefaultFormulae> a,
                                                      ParcelDiag d) {
  parcel_steps<DefaultFormulae, true>(a, &d);
}
// include/sdm_parcel_coal.h: the step over the parcel's live rows in the order of its permutation
__global__ __launch_bounds__(COND_CB) void k_parcel_p(ParcelArgs<DefaultFormulae> a,
                                                      ParcelPerm pp) {
  parcel_steps<DefaultFormulae, false, false, true>(a, nullptr, nullptr, &pp);
}
// include/sdm_parcel_ice.h: the step with the freezing and deposition passes after the solver
__global__ __launch_bounds__(COND_CB) void k_parcel_i(ParcelArgs<DefaultFormulae> a,
                                                      ParcelIce ic) {
  parcel_steps<DefaultFormulae, false, false, false, true>(a, nullptr, nullptr, nullptr, &ic);
}
__global__ __launch_bounds__(COND_CB) void k_parcel_diagnose(
    ParcelDiagnoseArgs<DefaultFormulae> a) {
  parcel_diagnose_cells<DefaultFormulae>(a);
}

// ---- ambient methods (pm.py) ---------------------------------------------------------------------
__global__ void k_temperature_pressure_rh(const double *rhod, const double *thd, const double *qv,
                                          double *T, double *p, double *RH, int64_t n, Kc k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  double t, pp, rh;
  tprh_of(k, rhod[i], thd[i], qv[i], t, pp, rh);
  T[i] = t;
  p[i] = pp;
  RH[i] = rh;
}

__global__ void k_air_density(double *out, const double *rhod, const double *qv, int64_t n) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) out[i] = air_density_of(rhod[i], qv[i]);
}

__global__ void k_air_dynamic_viscosity(double *out, const double *temperature, int64_t n, Kc k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = air_dynamic_viscosity_of(temperature[i], k.Z3, k.Z2, k.Z1, k.Z0);
}

__global__ void k_critical_volume(double *v_cr, const double *kappa, const double *v_dry,
                                  const double *T, const int64_t *cell, int64_t n, Kc k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  v_cr[i] = critical_volume_of(k, kappa[i], v_dry[i], T[cell[i]]);
}

__global__ void k_reynolds_number(double *out, const int64_t *cell_id, const double *eta,
                                  const double *rho, const double *radius, const double *u,
                                  int64_t n) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t c = cell_id[i];
  out[i] = reynolds_number_of(radius[i], u[i], rho[c], eta[c]);
}

__global__ void k_explicit_euler(double *y, int64_t n, double dt, double dy_dt) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) y[i] = y[i] + dt * dy_dt;  // trivia.py:35-36
}

}  // namespace

extern "C" int sdm_condensation(
    sdm_ctx *ctx, int64_t n_sd, int64_t n_cell, const int64_t *cell_start_arg, double *water_mass,
    const double *v_cr, const int64_t *multiplicity, const double *vdry, const int64_t *idx,
    const double *rhod, const double *thd, const double *water_vapour_mixing_ratio, double dv,
    const double *prhod, double *pthd, double *predicted_water_vapour_mixing_ratio,
    const double *kappa, const double *f_org, double rtol_x, double rtol_thd, double timestep,
    int64_t *n_substeps, int64_t *n_activating, int64_t *n_deactivating, int64_t *n_ripening,
    const int64_t *cell_order, double *RH_max, uint8_t *success, const double *reynolds_number,
    const double *air_density, const double *air_dynamic_viscosity, double dt_min, double dt_max,
    int adaptive, int fuse, int multiplier, double RH_rtol, int max_iters,
    const double consts[34]) {
  (void)f_org;  // surface_tension Constant
  (void)reynolds_number;  // ventilation Neglect
  (void)air_density;
  (void)air_dynamic_viscosity;
  CondArgs<DefaultFormulae> g;
  SDM_COND_FILL_ARGS(g);
  g.k = consts_of(consts);
  hipLaunchKernelGGL(k_condensation, dim3((unsigned)n_cell), dim3(COND_CB), 0, ctx->stream, g);
  LAUNCH_CHECK();
  return SDM_OK;
}

int sdm_parcel_launch_default(sdm_ctx *ctx, const ParcelCall &call) {
  ParcelArgs<DefaultFormulae> a;
  SDM_PARCEL_FILL_ARGS(a, call);
  a.c.k = consts_of(call.consts);
  if (call.requests) {
    const ParcelDiag d{call.requests, call.diag};
    hipLaunchKernelGGL(k_parcel_d, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0, ctx->stream,
                       a, d);
  } else {
    hipLaunchKernelGGL(k_parcel, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0, ctx->stream, a);
  }
  LAUNCH_CHECK();
  return SDM_OK;
}

int sdm_parcel_launch_default_perm(sdm_ctx *ctx, const ParcelCall &call, const int64_t *n_live,
                                   double *dv) {
  ParcelArgs<DefaultFormulae> a;
  SDM_PARCEL_FILL_ARGS(a, call);
  a.c.k = consts_of(call.consts);
  ARG_TRY(n_live && dv && !call.requests);
  const ParcelPerm pp{n_live, dv};
  hipLaunchKernelGGL(k_parcel_p, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0, ctx->stream, a,
                     pp);
  LAUNCH_CHECK();
  return SDM_OK;
}

int sdm_parcel_launch_default_ice(sdm_ctx *ctx, const ParcelCall &call,
                                  const ParcelIceCall &ice) {
  ParcelArgs<DefaultFormulae> a;
  SDM_PARCEL_FILL_ARGS(a, call);
  a.c.k = consts_of(call.consts);
  ARG_TRY(!call.requests);
  const ParcelIce ic = parcel_ice_of(ice, call.cfg.dt);
  hipLaunchKernelGGL(k_parcel_i, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0, ctx->stream, a,
                     ic);
  LAUNCH_CHECK();
  return SDM_OK;
}

int sdm_parcel_diagnose_default(sdm_ctx *ctx, const ParcelDiagnoseCall &call) {
  ParcelDiagnoseArgs<DefaultFormulae> a;
  a.k = consts_of(call.consts);
  SDM_PARCEL_FILL_DIAGNOSE_ARGS(a, call);
  hipLaunchKernelGGL(k_parcel_diagnose, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0,
                     ctx->stream, a);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_temperature_pressure_rh(sdm_ctx *ctx, const double *rhod, const double *thd,
                                           const double *water_vapour_mixing_ratio, double *T,
                                           double *p, double *RH, int64_t n,
                                           const double consts[34]) {
  ARG_TRY(ctx && n >= 0 && consts);
  if (n == 0) return SDM_OK;
  ARG_TRY(rhod && thd && water_vapour_mixing_ratio && T && p && RH);
  hipLaunchKernelGGL(k_temperature_pressure_rh, GRID1D(n), rhod, thd, water_vapour_mixing_ratio,
                     T, p, RH, n, consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_air_density(sdm_ctx *ctx, double *output, const double *rhod,
                               const double *water_vapour_mixing_ratio, int64_t n) {
  ARG_TRY(ctx && n >= 0);
  if (n == 0) return SDM_OK;
  ARG_TRY(output && rhod && water_vapour_mixing_ratio);
  hipLaunchKernelGGL(k_air_density, GRID1D(n), output, rhod, water_vapour_mixing_ratio, n);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_air_dynamic_viscosity(sdm_ctx *ctx, double *output, const double *temperature,
                                         int64_t n, const double consts[34]) {
  ARG_TRY(ctx && n >= 0 && consts);
  if (n == 0) return SDM_OK;
  ARG_TRY(output && temperature);
  hipLaunchKernelGGL(k_air_dynamic_viscosity, GRID1D(n), output, temperature, n,
                     consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_critical_volume(sdm_ctx *ctx, double *v_cr, const double *kappa,
                                   const double *f_org, const double *v_dry, const double *v_wet,
                                   const double *T, const int64_t *cell, int64_t n,
                                   const double consts[34]) {
  (void)f_org;  // surface_tension Constant: sigma ignores the volumes and f_org
  (void)v_wet;
  ARG_TRY(ctx && n >= 0 && consts);
  if (n == 0) return SDM_OK;
  ARG_TRY(v_cr && kappa && v_dry && T && cell);
  hipLaunchKernelGGL(k_critical_volume, GRID1D(n), v_cr, kappa, v_dry, T, cell, n,
                     consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_reynolds_number(sdm_ctx *ctx, double *output, const int64_t *cell_id,
                                   const double *dynamic_viscosity, const double *density,
                                   const double *radius, const double *velocity_wrt_air,
                                   int64_t n) {
  ARG_TRY(ctx && n >= 0);
  if (n == 0) return SDM_OK;
  ARG_TRY(output && cell_id && dynamic_viscosity && density && radius && velocity_wrt_air);
  hipLaunchKernelGGL(k_reynolds_number, GRID1D(n), output, cell_id, dynamic_viscosity, density,
                     radius, velocity_wrt_air, n);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_explicit_euler(sdm_ctx *ctx, double *y, int64_t n, double dt, double dy_dt) {
  ARG_TRY(ctx && n >= 0);
  if (n == 0) return SDM_OK;
  ARG_TRY(y);
  hipLaunchKernelGGL(k_explicit_euler, GRID1D(n), y, n, dt, dy_dt);
  LAUNCH_CHECK();
  return SDM_OK;
}

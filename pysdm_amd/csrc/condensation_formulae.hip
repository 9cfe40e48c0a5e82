// condensation_formulae.hip -- the condensation path with formulae other than PySDM's defaults
// (include/sdm_condensation_formulae.h) for gfx950: the general instantiation of
// condensation_solver.h (where the kernel's design is described), every option a kernel-uniform
// switch on the descriptor (condensation_formulae.h), and the two ambient methods that depend on
// the options.  ONE general kernel, not one per combination of choices.
//
// Per droplet the general formulae read more inputs than the default ones: f_org and the dry
// volume itself (surface tension; the solver caches rd3 = vdry / PI_4_3, and rd3 * PI_4_3 need not
// round back to vdry) and the Reynolds number (ventilation).  The first COND_CH positions of a
// cell keep them in LDS (3 * 8 KB next to the solver's 8240 B; a CU has 160 KB and the kernel's
// register use allows one workgroup per CU anyway), later positions read them from HBM on each
// pass.  The cell's Schmidt number is formed per sub-step from the cell's air viscosity and
// density and the sub-step's diffusivity, as step_impl does (cm.py:298-302).
//
// The CPU checker of this file is tests/condensation_formulae_checker/, which compiles the same
// condensation_formulae.h.
#include "parcel_solver.h"
#include "../../include/sdm_condensation_formulae.h"

#define CF_FN __device__ __forceinline__ static
#include "condensation_formulae.h"

#define GRID1D(n) dim3(grid_for(n)), dim3(SDM_BLOCK), 0, ctx->stream

namespace {

struct Kg {
  cf_k f;                                 // constants and option codes
  const double *f_org, *reynolds_number;  // per droplet (reynolds_number: NULL under Neglect)
  const double *vdry;                     // per droplet (CondArgs' own, for extra_of)
  const double *air_density, *air_dynamic_viscosity;  // per cell
};

// pm.py:53-61: what k_temperature_pressure_rh_f writes for one cell and the parcel kernel for a
// parcel
DF void tprh_of(const cf_k *k, double rhod, double thd, double qv, double &T, double &p,
                double &RH) {
  T = cf_svt_T(k, rhod, thd);
  p = cf_svt_p(k, rhod, T, qv);
  RH = cf_svt_pv(k, p, qv) / cf_pvs_water(k, T);
}
// pm.py:22-33: what k_critical_volume_f writes for one droplet and the parcel kernel for a row
// (f_org and v_wet are read only where the surface tension is not Constant)
DF double critical_volume_of(const cf_k *k, double kappa, const double *f_org, double v_dry,
                             double v_wet, double t) {
  int fail = 0;
  double forg = 0.0, vwet = 0.0;
  if (CF_O(SURFACE_TENSION) != SDM_COND_SGM_CONSTANT) {
    forg = *f_org;
    vwet = v_wet;
  }
  const double sigma = cf_sigma(k, t, vwet, v_dry, forg, &fail);
  const double r_cr = cf_r_cr(k, kappa, v_dry / CF_C(PI_4_3), t, sigma);
  return fail ? sdm_nan() : cf_volume(k, r_cr);
}

// the policy of condensation_solver.h (and parcel_solver.h) for any combination of choices
struct GeneralFormulae {
  using K = Kg;
  struct Extra {
    double f_org, Re, vdry;
  };
  static constexpr int STAGE = 3 * COND_CH;
  struct MinArgs {
    double x_old, timestep, kappa, f_org, rd3, T, RH, Fk, Fd;
    int fail;
  };
  struct Cellwide {  // the sub-step's cell scalars (uniform)
    double T, RH, lv, pvs, DTp, KTp, lambdaK, lambdaD, Sc, timestep, rtol_x, RH_rtol;
    int max_iters;
  };
  DF static double rho_w(const Kg &k) { return k.f.c[SDM_COND_K_RHO_W]; }
  DF static double c_pd(const Kg &k) { return k.f.c[SDM_COND_K_C_PD]; }
  DF static double pi_4_3(const Kg &k) { return k.f.c[SDM_COND_K_PI_4_3]; }
  DF static double x_of(const Kg &k, double m) { return cf_x(&k.f, m); }
  DF static double mass_of(const Kg &k, double x) { return cf_mass(&k.f, x); }
  DF static bool failed(const MinArgs &a) { return a.fail != 0; }
  // parcel_solver.h
  DF static double Rv(const Kg &k) { return k.f.c[SDM_COND_K_RV]; }
  DF static double Rd(const Kg &k) { return k.f.c[SDM_COND_K_RD]; }
  DF static double c_pv(const Kg &k) { return k.f.c[SDM_COND_K_C_PV]; }
  DF static double lv(const Kg &k, double T) { return cf_lv(&k.f, T); }
  DF static void tprh(const Kg &k, double rhod, double thd, double qv, double &T, double &p,
                      double &RH) {
    tprh_of(&k.f, rhod, thd, qv, T, p, RH);
  }
  DF static double critical_volume(const Kg &k, int64_t row, double kappa, double v_dry,
                                   double v_wet, double T) {
    return critical_volume_of(&k.f, kappa, k.f_org ? k.f_org + row : nullptr, v_dry, v_wet, T);
  }

  DF static Extra extra_of(const Kg &k, int64_t drop) {
    Extra e;
    e.f_org = k.f.o[SDM_COND_OPT_SURFACE_TENSION] != SDM_COND_SGM_CONSTANT ? k.f_org[drop] : 0.0;
    e.Re = k.f.o[SDM_COND_OPT_VENTILATION] != SDM_COND_VENT_NEGLECT ? k.reynolds_number[drop]
                                                                      : 0.0;
    e.vdry = k.vdry[drop];
    return e;
  }
  DF static void stage_put(double *stage, int q, Extra e) {
    stage[q] = e.f_org;
    stage[COND_CH + q] = e.Re;
    stage[2 * COND_CH + q] = e.vdry;
  }
  DF static Extra stage_get(const double *stage, int q) {
    Extra e;
    e.f_org = stage[q];
    e.Re = stage[COND_CH + q];
    e.vdry = stage[2 * COND_CH + q];
    return e;
  }

  // minfun, cm.py:379-406
  DF static double minfun(const Kg &kg, double x_new, MinArgs &a) {
    const cf_k *k = &kg.f;
    if (x_new > cf_x_max(k)) return a.x_old - x_new;
    const double mass_new = cf_mass(k, x_new);
    const double volume_new = mass_new / CF_C(RHO_W);
    const double r_new = cf_radius(k, volume_new);
    const double sgm = cf_sigma(k, a.T, volume_new, CF_C(PI_4_3) * a.rd3, a.f_org, &a.fail);
    const double RH_eq = cf_RH_eq(k, r_new, a.T, a.kappa, a.rd3, sgm);
    const double r_dr_dt = cf_r_dr_dt(k, RH_eq, a.RH, a.Fk, a.Fd);
    const double dm_dt = 4 * CF_C(PI) * CF_C(RHO_W) * r_new * r_dr_dt;
    return a.x_old - x_new + a.timestep * cf_dx_dt(k, mass_new, dm_dt);
  }

  // step_impl's cell scalars, cm.py:288-302,429-430
  DF static void cellwide(const CondArgs<GeneralFormulae> &g, int64_t cell, double rhod,
                          double thd, double qv, Cellwide &w) {
    cellwide_of(&g.k.f, g.k.air_dynamic_viscosity + cell, g.k.air_density + cell, rhod, thd, qv,
                w);
  }
  // ... with the cell's air behind two pointers, read only with a ventilation
  DF static void cellwide_of(const cf_k *k, const double *air_dynamic_viscosity,
                             const double *air_density, double rhod, double thd, double qv,
                             Cellwide &w) {
    w.T = cf_svt_T(k, rhod, thd);
    const double p = cf_svt_p(k, rhod, w.T, qv);
    const double pv = cf_svt_pv(k, p, qv);
    w.lv = cf_lv(k, w.T);
    w.pvs = cf_pvs_water(k, w.T);
    w.DTp = cf_thermics_D(k, w.T, p);
    w.KTp = cf_thermics_K(k, w.T, p);
    w.RH = pv / w.pvs;
    w.Sc = 0.0;
    if (CF_O(VENTILATION) != SDM_COND_VENT_NEGLECT)
      w.Sc = cf_air_schmidt_number(*air_dynamic_viscosity, w.DTp, *air_density);
    w.lambdaK = cf_lambdaK(k, w.T, p);
    w.lambdaD = cf_lambdaD(k, w.DTp, w.T);
  }

  // cm.py:434-491
  DF static void start(const Kg &kg, const Cellwide &w, double m, double rd3, double kappa,
                       Extra e, MinArgs &args, double &x_old, double &dx_old) {
    const cf_k *k = &kg.f;
    const double v_drop = m / CF_C(RHO_W);
    x_old = cf_x(k, m);
    const double r_old = cf_radius(k, v_drop);
    args = {x_old, w.timestep, kappa, e.f_org, rd3, w.T, w.RH, 0, 0, 0};
    const double sgm = cf_sigma(k, w.T, v_drop, e.vdry, e.f_org, &args.fail);
    const double RH_eq = cf_RH_eq(k, r_old, w.T, kappa, rd3, sgm);
    dx_old = 0.0;
    if (!within_tolerance(sdm_abs(w.RH - RH_eq), w.RH, w.RH_rtol)) {
      const double Dr = cf_kinetics_D(k, w.DTp, r_old, w.lambdaD);
      const double Kr = cf_kinetics_K(k, w.KTp, r_old, w.lambdaK);
      const double mass_ventilation_factor = cf_ventilation_factor(k, e.Re, w.Sc);
      const double heat_ventilation_factor = mass_ventilation_factor;
      args.Fk = cf_Fk(k, w.T, Kr * heat_ventilation_factor, w.lv);
      args.Fd = cf_Fd(k, w.T, Dr * mass_ventilation_factor, w.pvs);
      const double r_dr_dt_old = cf_r_dr_dt(k, RH_eq, w.RH, args.Fk, args.Fd);
      const double mass_old = cf_mass(k, x_old);
      const double dm_dt_old = 4 * CF_C(PI) * CF_C(RHO_W) * r_old * r_dr_dt_old;
      dx_old = w.timestep * cf_dx_dt(k, mass_old, dm_dt_old);
    }
  }
};

__global__ __launch_bounds__(COND_CB) void k_condensation_f(CondArgs<GeneralFormulae> g) {
  condensation_cell<GeneralFormulae>(g);
}

// include/sdm_parcel.h with a formulae descriptor: one workgroup per parcel, the launch's time
// steps inside (parcel_solver.h)
__global__ __launch_bounds__(COND_CB) void k_parcel_f(ParcelArgs<GeneralFormulae> a) {
  parcel_steps<GeneralFormulae>(a);
}

// include/sdm_parcel_diag.h: the same loop with the request table evaluated after every step, and
// the table on given columns
__global__ __launch_bounds__(COND_CB) void k_parcel_f_d(ParcelArgs<GeneralFormulae> a,
                                                        ParcelDiag d) {
  parcel_steps<GeneralFormulae, true>(a, &d);
}
// include/sdm_parcel_coal.h: the step over the parcel's live rows in the order of its permutation
__global__ __launch_bounds__(COND_CB) void k_parcel_f_p(ParcelArgs<GeneralFormulae> a,
                                                        ParcelPerm pp) {
  parcel_steps<GeneralFormulae, false, false, true>(a, nullptr, nullptr, &pp);
}
// include/sdm_parcel_ice.h: the step with the freezing and deposition passes after the solver
__global__ __launch_bounds__(COND_CB) void k_parcel_f_i(ParcelArgs<GeneralFormulae> a,
                                                        ParcelIce ic) {
  parcel_steps<GeneralFormulae, false, false, false, true>(a, nullptr, nullptr, nullptr, &ic);
}
// include/sdm_parcel_vent.h: the general formulae for a parcel whose air density and viscosity
// change from step to step inside the kernel - the solver's cell scalars read the parcel's pair
// from LDS (parcel_solver.h), everything else is GeneralFormulae's
struct VentFormulae : GeneralFormulae {
  DF static void cellwide(const CondArgs<VentFormulae> &g, int64_t, double rhod, double thd,
                          double qv, Cellwide &w) {
    const VentLds *vl = vent_lds();
    cellwide_of(&g.k.f, &vl->air[PA_ETA], &vl->air[PA_RHO], rhod, thd, qv, w);
  }
  DF static double air_dynamic_viscosity(const Kg &k, double T) {  // the body of the stage kernel
    return air_dynamic_viscosity_of(T, k.f.c[SDM_COND_K_ZOGRAFOS_T3], k.f.c[SDM_COND_K_ZOGRAFOS_T2],
                                    k.f.c[SDM_COND_K_ZOGRAFOS_T1], k.f.c[SDM_COND_K_ZOGRAFOS_T0]);
  }
};
__global__ __launch_bounds__(COND_CB) void k_parcel_v(ParcelArgs<VentFormulae> a, ParcelVent v) {
  parcel_steps<VentFormulae, false, true>(a, nullptr, &v);
}
__global__ __launch_bounds__(COND_CB) void k_parcel_v_d(ParcelArgs<VentFormulae> a, ParcelDiag d,
                                                        ParcelVent v) {
  parcel_steps<VentFormulae, true, true>(a, &d, &v);
}

__global__ __launch_bounds__(COND_CB) void k_parcel_diagnose_f(
    ParcelDiagnoseArgs<GeneralFormulae> a) {
  parcel_diagnose_cells<GeneralFormulae>(a);
}

// ---- ambient methods (pm.py) ---------------------------------------------------------------------
__global__ void k_temperature_pressure_rh_f(const double *rhod, const double *thd,
                                            const double *qv, double *T, double *p, double *RH,
                                            int64_t n, cf_k kk) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  double t, pp, rh;
  tprh_of(&kk, rhod[i], thd[i], qv[i], t, pp, rh);
  T[i] = t;
  p[i] = pp;
  RH[i] = rh;
}

__global__ void k_critical_volume_f(double *v_cr, const double *kappa, const double *f_org,
                                    const double *v_dry, const double *v_wet, const double *T,
                                    const int64_t *cell, int64_t n, cf_k kk) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const cf_k *k = &kk;
  const bool film = CF_O(SURFACE_TENSION) != SDM_COND_SGM_CONSTANT;
  v_cr[i] = critical_volume_of(k, kappa[i], film ? f_org + i : nullptr, v_dry[i],
                               film ? v_wet[i] : 0.0, T[cell[i]]);
}

// the descriptor and the default path's constants as the kernels' argument; refuses codes the
// header does not define
int formulae_of(const double *consts, const sdm_cond_formulae *formulae, cf_k *out) {
  static const int n_choices[SDM_COND_N_OPTS] = CF_N_CHOICES;
  for (int i = 0; i < SDM_COND_N_OPTS; ++i)
    if (formulae->option[i] < 0 || formulae->option[i] >= n_choices[i]) return 0;
  for (int i = 0; i < SDM_COND_N_CONSTS; ++i) out->c[i] = consts[i];
  for (int i = 0; i < SDM_COND_F_N_CONSTS; ++i) out->f[i] = formulae->consts[i];
  for (int i = 0; i < 10; ++i) out->o[i] = i < SDM_COND_N_OPTS ? formulae->option[i] : 0;
  return 1;
}

}  // namespace

extern "C" int sdm_condensation_f(
    sdm_ctx *ctx, int64_t n_sd, int64_t n_cell, const int64_t *cell_start_arg, double *water_mass,
    const double *v_cr, const int64_t *multiplicity, const double *vdry, const int64_t *idx,
    const double *rhod, const double *thd, const double *water_vapour_mixing_ratio, double dv,
    const double *prhod, double *pthd, double *predicted_water_vapour_mixing_ratio,
    const double *kappa, const double *f_org, double rtol_x, double rtol_thd, double timestep,
    int64_t *n_substeps, int64_t *n_activating, int64_t *n_deactivating, int64_t *n_ripening,
    const int64_t *cell_order, double *RH_max, uint8_t *success, const double *reynolds_number,
    const double *air_density, const double *air_dynamic_viscosity, double dt_min, double dt_max,
    int adaptive, int fuse, int multiplier, double RH_rtol, int max_iters,
    const double consts[34], const sdm_cond_formulae *formulae) {
  ARG_TRY(formulae);
  CondArgs<GeneralFormulae> g;
  SDM_COND_FILL_ARGS(g);
  ARG_TRY(formulae_of(consts, formulae, &g.k.f));
  const bool film = formulae->option[SDM_COND_OPT_SURFACE_TENSION] != SDM_COND_SGM_CONSTANT;
  const bool ventilated = formulae->option[SDM_COND_OPT_VENTILATION] != SDM_COND_VENT_NEGLECT;
  ARG_TRY(n_sd == 0 || !film || f_org);
  ARG_TRY(n_sd == 0 || !ventilated || reynolds_number);
  ARG_TRY(!ventilated || (air_density && air_dynamic_viscosity));
  g.k.f_org = f_org;
  g.k.reynolds_number = reynolds_number;
  g.k.vdry = vdry;
  g.k.air_density = air_density;
  g.k.air_dynamic_viscosity = air_dynamic_viscosity;
  hipLaunchKernelGGL(k_condensation_f, dim3((unsigned)n_cell), dim3(COND_CB), 0, ctx->stream, g);
  LAUNCH_CHECK();
  return SDM_OK;
}

int sdm_parcel_launch_general(sdm_ctx *ctx, const ParcelCall &call,
                              const sdm_cond_formulae *formulae) {
  ParcelArgs<GeneralFormulae> a;
  SDM_PARCEL_FILL_ARGS(a, call);
  ARG_TRY(formulae && formulae_of(call.consts, formulae, &a.c.k.f));
  // (a ventilated parcel has kernels and an entry point of its own: sdm_parcel_launch_vent)
  ARG_TRY(formulae->option[SDM_COND_OPT_VENTILATION] == SDM_COND_VENT_NEGLECT);
  ARG_TRY(formulae->option[SDM_COND_OPT_SURFACE_TENSION] == SDM_COND_SGM_CONSTANT || call.f_org);
  a.c.k.f_org = call.f_org;
  a.c.k.reynolds_number = nullptr;
  a.c.k.vdry = call.vdry;
  a.c.k.air_density = a.c.k.air_dynamic_viscosity = nullptr;
  if (call.requests) {
    const ParcelDiag d{call.requests, call.diag};
    hipLaunchKernelGGL(k_parcel_f_d, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0, ctx->stream,
                       a, d);
  } else {
    hipLaunchKernelGGL(k_parcel_f, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0, ctx->stream,
                       a);
  }
  LAUNCH_CHECK();
  return SDM_OK;
}

int sdm_parcel_launch_general_perm(sdm_ctx *ctx, const ParcelCall &call,
                                   const sdm_cond_formulae *formulae, const int64_t *n_live,
                                   double *dv) {
  ParcelArgs<GeneralFormulae> a;
  SDM_PARCEL_FILL_ARGS(a, call);
  ARG_TRY(formulae && formulae_of(call.consts, formulae, &a.c.k.f));
  ARG_TRY(formulae->option[SDM_COND_OPT_VENTILATION] == SDM_COND_VENT_NEGLECT);
  ARG_TRY(formulae->option[SDM_COND_OPT_SURFACE_TENSION] == SDM_COND_SGM_CONSTANT || call.f_org);
  ARG_TRY(n_live && dv && !call.requests);
  a.c.k.f_org = call.f_org;
  a.c.k.reynolds_number = nullptr;
  a.c.k.vdry = call.vdry;
  a.c.k.air_density = a.c.k.air_dynamic_viscosity = nullptr;
  const ParcelPerm pp{n_live, dv};
  hipLaunchKernelGGL(k_parcel_f_p, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0, ctx->stream,
                     a, pp);
  LAUNCH_CHECK();
  return SDM_OK;
}

int sdm_parcel_launch_general_ice(sdm_ctx *ctx, const ParcelCall &call,
                                  const sdm_cond_formulae *formulae, const ParcelIceCall &ice) {
  ParcelArgs<GeneralFormulae> a;
  SDM_PARCEL_FILL_ARGS(a, call);
  ARG_TRY(formulae && formulae_of(call.consts, formulae, &a.c.k.f));
  ARG_TRY(formulae->option[SDM_COND_OPT_VENTILATION] == SDM_COND_VENT_NEGLECT);
  ARG_TRY(formulae->option[SDM_COND_OPT_SURFACE_TENSION] == SDM_COND_SGM_CONSTANT || call.f_org);
  ARG_TRY(!call.requests);
  a.c.k.f_org = call.f_org;
  a.c.k.reynolds_number = nullptr;
  a.c.k.vdry = call.vdry;
  a.c.k.air_density = a.c.k.air_dynamic_viscosity = nullptr;
  const ParcelIce ic = parcel_ice_of(ice, call.cfg.dt);
  hipLaunchKernelGGL(k_parcel_f_i, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0, ctx->stream,
                     a, ic);
  LAUNCH_CHECK();
  return SDM_OK;
}

int sdm_parcel_launch_vent(sdm_ctx *ctx, const ParcelCall &call,
                           const sdm_cond_formulae *formulae, const sdm_parcel_vent *vent) {
  ParcelArgs<VentFormulae> a;
  SDM_PARCEL_FILL_ARGS(a, call);
  ARG_TRY(formulae && vent && formulae_of(call.consts, formulae, &a.c.k.f));
  ARG_TRY(formulae->option[SDM_COND_OPT_VENTILATION] != SDM_COND_VENT_NEGLECT);
  ARG_TRY(formulae->option[SDM_COND_OPT_SURFACE_TENSION] == SDM_COND_SGM_CONSTANT || call.f_org);
  a.c.k.f_org = call.f_org;
  a.c.k.reynolds_number = vent->reynolds_number;  // (written by the kernel before it is read)
  a.c.k.vdry = call.vdry;
  a.c.k.air_density = a.c.k.air_dynamic_viscosity = nullptr;  // (the parcel's pair is in LDS)
  ParcelVent v;
  v.law = vent->velocity_law;
  v.terms = vent->velocity_terms;
  v.params = vent->velocity_params;
  v.gk_a = vent->gk_a;
  v.gk_b = vent->gk_b;
  v.gk_len = vent->gk_table_len;
  v.gk_factor = vent->gk_factor;
  v.gk_top = vent->gk_top;
  v.air_density = vent->air_density;
  v.air_dynamic_viscosity = vent->air_dynamic_viscosity;
  v.reynolds_number = vent->reynolds_number;
  v.out_of_table = vent->out_of_table;
  if (call.requests) {
    const ParcelDiag d{call.requests, call.diag};
    hipLaunchKernelGGL(k_parcel_v_d, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0, ctx->stream,
                       a, d, v);
  } else {
    hipLaunchKernelGGL(k_parcel_v, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0, ctx->stream,
                       a, v);
  }
  LAUNCH_CHECK();
  return SDM_OK;
}

int sdm_parcel_diagnose_general(sdm_ctx *ctx, const ParcelDiagnoseCall &call,
                                const sdm_cond_formulae *formulae) {
  ParcelDiagnoseArgs<GeneralFormulae> a;
  ARG_TRY(formulae && formulae_of(call.consts, formulae, &a.k.f));
  ARG_TRY(formulae->option[SDM_COND_OPT_SURFACE_TENSION] == SDM_COND_SGM_CONSTANT || call.f_org);
  a.k.f_org = call.f_org;
  a.k.reynolds_number = nullptr;
  a.k.vdry = call.vdry;
  a.k.air_density = a.k.air_dynamic_viscosity = nullptr;
  SDM_PARCEL_FILL_DIAGNOSE_ARGS(a, call);
  hipLaunchKernelGGL(k_parcel_diagnose_f, dim3((unsigned)call.n_parcel), dim3(COND_CB), 0,
                     ctx->stream, a);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_temperature_pressure_rh_f(sdm_ctx *ctx, const double *rhod, const double *thd,
                                             const double *water_vapour_mixing_ratio, double *T,
                                             double *p, double *RH, int64_t n,
                                             const double consts[34],
                                             const sdm_cond_formulae *formulae) {
  ARG_TRY(ctx && n >= 0 && consts && formulae);
  cf_k k;
  ARG_TRY(formulae_of(consts, formulae, &k));
  if (n == 0) return SDM_OK;
  ARG_TRY(rhod && thd && water_vapour_mixing_ratio && T && p && RH);
  hipLaunchKernelGGL(k_temperature_pressure_rh_f, GRID1D(n), rhod, thd,
                     water_vapour_mixing_ratio, T, p, RH, n, k);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_critical_volume_f(sdm_ctx *ctx, double *v_cr, const double *kappa,
                                     const double *f_org, const double *v_dry,
                                     const double *v_wet, const double *T, const int64_t *cell,
                                     int64_t n, const double consts[34],
                                     const sdm_cond_formulae *formulae) {
  ARG_TRY(ctx && n >= 0 && consts && formulae);
  cf_k k;
  ARG_TRY(formulae_of(consts, formulae, &k));
  if (n == 0) return SDM_OK;
  ARG_TRY(v_cr && kappa && v_dry && T && cell);
  ARG_TRY(formulae->option[SDM_COND_OPT_SURFACE_TENSION] == SDM_COND_SGM_CONSTANT ||
          (f_org && v_wet));
  hipLaunchKernelGGL(k_critical_volume_f, GRID1D(n), v_cr, kappa, f_org, v_dry, v_wet, T, cell,
                     n, k);
  LAUNCH_CHECK();
  return SDM_OK;
}

/*
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_condensation_formulae.h.
 *
 * A serial, strict-IEEE restatement of the reference's condensation solver
 * (PySDM/backends/impl_numba/methods/condensation_methods.py, "cm.py" below), its TOMS748 root
 * finder (impl_numba/toms748.py) and the two ambient methods that depend on the formulae options
 * (impl_numba/methods/physics_methods.py, "pm.py"), statement for statement, every formula taken
 * from the option switches of pysdm_amd/csrc/condensation_formulae.h, which the product compiles
 * too; so are the transcendental functions (csrc/sdm_math.h): both sides get the same bits.  The
 * loop structure is the one of tests/checker/condensation_checker.c (the default formulae's
 * checker), written out again because that file implements another header.  Host pointers; the
 * context is ignored.  Built by __graft_entry__.build() next to this file (git-ignored); nothing
 * in pysdm_amd/ loads it.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/sdm_condensation_formulae.h"
#include "../../pysdm_amd/csrc/sdm_math.h"

#define CF_FN static inline
#include "../../pysdm_amd/csrc/condensation_formulae.h"

#define API __attribute__((visibility("default")))

static __thread char g_err[256] = "";
#define FAIL(code, msg)                        \
  do {                                         \
    snprintf(g_err, sizeof(g_err), "%s", msg); \
    return (code);                             \
  } while (0)

API const char *sdm_last_error(void) { return g_err; }

static int formulae_of(const double *consts, const sdm_cond_formulae *formulae, cf_k *out) {
  static const int n_choices[SDM_COND_N_OPTS] = {2, 6, 3, 2, 3, 4, 4, 4, 3};
  if (!consts || !formulae) return 0;
  for (int i = 0; i < SDM_COND_N_OPTS; ++i)
    if (formulae->option[i] < 0 || formulae->option[i] >= n_choices[i]) return 0;
  for (int i = 0; i < SDM_COND_N_CONSTS; ++i) out->c[i] = consts[i];
  for (int i = 0; i < SDM_COND_F_N_CONSTS; ++i) out->f[i] = formulae->consts[i];
  for (int i = 0; i < 10; ++i) out->o[i] = i < SDM_COND_N_OPTS ? formulae->option[i] : 0;
  return 1;
}

static int64_t floordiv(int64_t a, int64_t b) {
  int64_t q = a / b;
  return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}
/* trivia.py:38-40 */
static int within_tolerance(double error_estimate, double value, double rtol) {
  return error_estimate < rtol * sdm_abs(value);
}
/* particle_shape_and_density/liquid_spheres.py:37-44 */
static double dm_dt_of(const cf_k *k, double r, double r_dr_dt) {
  return 4 * CF_C(PI) * CF_C(RHO_W) * r * r_dr_dt;
}

/* ---- minfun (cm.py:379-406) ---------------------------------------------------------------- */
typedef struct {
  double x_old, timestep, kappa, f_org, rd3, T, RH, Fk, Fd;
  int fail; /* CompressedFilmRuehl used up its iterations (the reference's assert) */
} MinArgs;

static double minfun(const cf_k *k, double x_new, MinArgs *a) {
  if (x_new > cf_x_max(k)) return a->x_old - x_new;
  const double mass_new = cf_mass(k, x_new);
  const double volume_new = mass_new / CF_C(RHO_W);
  const double r_new = cf_radius(k, volume_new);
  const double sgm = cf_sigma(k, a->T, volume_new, CF_C(PI_4_3) * a->rd3, a->f_org, &a->fail);
  const double RH_eq = cf_RH_eq(k, r_new, a->T, a->kappa, a->rd3, sgm);
  const double r_dr_dt = cf_r_dr_dt(k, RH_eq, a->RH, a->Fk, a->Fd);
  const double dm_dt = dm_dt_of(k, r_new, r_dr_dt);
  return a->x_old - x_new + a->timestep * cf_dx_dt(k, mass_new, dm_dt);
}

/* ---- TOMS748 (toms748.py) on minfun ---------------------------------------------------------- */
#define EPS_F 2.220446049250313e-16
#define MAX_F 1.7976931348623157e308
#define MIN_F 2.2250738585072014e-308

static void bracket(const cf_k *k, MinArgs *args, double *a, double *b, double c, double *fa,
                    double *fb, double *d, double *fd) { /* :24-47 */
  const double tol = EPS_F * 2;
  if ((*b - *a) < 2 * tol * *a)
    c = *a + (*b - *a) / 2;
  else if (c <= *a + sdm_abs(*a) * tol)
    c = *a + sdm_abs(*a) * tol;
  else if (c >= *b - sdm_abs(*b) * tol)
    c = *b - sdm_abs(*a) * tol;
  const double fc = minfun(k, c, args);
  if (fc == 0) {
    *a = c; *fa = 0; *d = 0; *fd = 0;
  } else if (*fa * fc < 0) {
    *d = *b; *fd = *fb; *b = c; *fb = fc;
  } else {
    *d = *a; *fd = *fa; *a = c; *fa = fc;
  }
}
static double safe_div(double num, double denom, double r) { /* :50-55 */
  if (sdm_abs(denom) < 1)
    if (sdm_abs(denom * MAX_F) <= sdm_abs(num)) return r;
  return num / denom;
}
static double secant_interpolate(double a, double b, double fa, double fb) { /* :58-64 */
  const double tol = EPS_F * 5;
  const double c = a - (fa / (fb - fa)) * (b - a);
  if (c <= a + sdm_abs(a) * tol || c >= b - sdm_abs(b) * tol) return (a + b) / 2;
  return c;
}
static double quadratic_interpolate(double a, double b, double d, double fa, double fb,
                                    double fd, int count) { /* :67-87 */
  const double B = safe_div(fb - fa, b - a, MAX_F);
  double A = safe_div(fd - fb, d - b, MAX_F);
  A = safe_div(A - B, d - a, 0.0);
  if (A == 0) return secant_interpolate(a, b, fa, fb);
  double c = (A * fa > 0) ? a : b;
  for (int i = 1; i < count + 1; ++i)
    c -= safe_div(fa + (B + A * (c - b)) * (c - a), B + A * (2.0 * c - a - b), 1.0 + c - a);
  if ((c <= a) || (c >= b)) c = secant_interpolate(a, b, fa, fb);
  return c;
}
static double cubic_interpolate(double a, double b, double d, double e, double fa, double fb,
                                double fd, double fe) { /* :90-106 */
  const double q11 = (d - e) * fd / (fe - fd);
  const double q21 = (b - d) * fb / (fd - fb);
  const double q31 = (a - b) * fa / (fb - fa);
  const double d21 = (b - d) * fd / (fd - fb);
  const double d31 = (a - b) * fb / (fb - fa);
  const double q22 = (d21 - q11) * fb / (fe - fb);
  const double q32 = (d31 - q21) * fa / (fd - fa);
  const double d32 = (d31 - q21) * fd / (fd - fa);
  const double q33 = (d32 - q22) * fa / (fe - fa);
  double c = q31 + q32 + q33 + a;
  if ((c <= a) || (c >= b)) c = quadratic_interpolate(a, b, d, fa, fb, fd, 3);
  return c;
}
static int tol_check(double a, double b, double rtol) { /* :109-111 */
  return within_tolerance(sdm_abs(a - b), cf_py_min(sdm_abs(a), sdm_abs(b)), rtol);
}
static int prof_of(double fa, double fb, double fd, double fe) {
  const double min_diff = MIN_F * 32;
  return sdm_abs(fa - fb) < min_diff || sdm_abs(fa - fd) < min_diff ||
         sdm_abs(fa - fe) < min_diff || sdm_abs(fb - fd) < min_diff ||
         sdm_abs(fb - fe) < min_diff || sdm_abs(fd - fe) < min_diff;
}
/* :114-223; returns the root, *iters = iterations taken (-1: not a bracket) */
static double solve(const cf_k *k, MinArgs *args, double ax, double bx, double fax, double fbx,
                    double rtol, int max_iter, int *iters) {
  int count = max_iter;
  const double mu = 0.5;
  double a = ax, b = bx, fa = fax, fb = fbx;
  if (!(a < b)) { *iters = -1; return sdm_nan(); }
  if (tol_check(a, b, rtol) || fa == 0 || fb == 0) {
    if (fa == 0) b = a;
    else if (fb == 0) a = b;
    *iters = 0;
    return (a + b) / 2;
  }
  if (!(fa * fb < 0)) { *iters = -1; return sdm_nan(); }
  double fe = 1e5, e = 1e5, fd = 1e5, d = 0, c;
  if (fa != 0) {
    c = secant_interpolate(a, b, fa, fb);
    bracket(k, args, &a, &b, c, &fa, &fb, &d, &fd);
    count -= 1;
    if (count > 0 && fa != 0 && !tol_check(a, b, rtol)) {
      c = quadratic_interpolate(a, b, d, fa, fb, fd, 2);
      e = d;
      fe = fd;
      bracket(k, args, &a, &b, c, &fa, &fb, &d, &fd);
      count -= 1;
    }
  }
  while (count > 0 && fa != 0 && !tol_check(a, b, rtol)) {
    const double a0 = a, b0 = b;
    if (prof_of(fa, fb, fd, fe)) c = quadratic_interpolate(a, b, d, fa, fb, fd, 2);
    else c = cubic_interpolate(a, b, d, e, fa, fb, fd, fe);
    e = d;
    fe = fd;
    bracket(k, args, &a, &b, c, &fa, &fb, &d, &fd);
    if (count == 1 || fa == 0 || tol_check(a, b, rtol)) { count -= 1; break; }
    if (prof_of(fa, fb, fd, fe)) c = quadratic_interpolate(a, b, d, fa, fb, fd, 3);
    else c = cubic_interpolate(a, b, d, e, fa, fb, fd, fe);
    bracket(k, args, &a, &b, c, &fa, &fb, &d, &fd);
    if (count == 1 || fa == 0 || tol_check(a, b, rtol)) { count -= 1; break; }
    double u, fu;
    if (sdm_abs(fa) < sdm_abs(fb)) { u = a; fu = fa; } else { u = b; fu = fb; }
    c = u - 2 * (fu / (fb - fa)) * (b - a);
    if (sdm_abs(c - u) > (b - a) / 2) c = a + (b - a) / 2;
    e = d;
    fe = fd;
    bracket(k, args, &a, &b, c, &fa, &fb, &d, &fd);
    if (count == 1 || fa == 0 || tol_check(a, b, rtol)) { count -= 1; break; }
    if ((b - a) < mu * (b0 - a0)) continue;
    e = d;
    fe = fd;
    bracket(k, args, &a, &b, a + (b - a) / 2, &fa, &fb, &d, &fd);
    count -= 1;
  }
  *iters = max_iter - count;
  if (fa == 0) b = a;
  else if (fb == 0) a = b;
  return (a + b) / 2;
}

/* ---- the solver ----------------------------------------------------------------------------- */
typedef struct {
  const cf_k *k;
  double *water_mass;
  const double *v_cr, *vdry, *kappa, *f_org, *reynolds_number;
  const int64_t *multiplicity;
  const int64_t *cell_idx;
  int64_t n_in_cell;
  double RH_rtol;
  int max_iters;
} Cell;

typedef struct {
  double result;
  int success;
  int64_t n_activating, n_deactivating, n_ripening;
} MlNew;

/* calculate_ml_old, cm.py:359-368 */
static double calculate_ml_old(const Cell *c) {
  double result = 0;
  for (int64_t i = 0; i < c->n_in_cell; ++i) {
    const int64_t drop = c->cell_idx[i];
    if (c->water_mass[drop] > 0) result += (double)c->multiplicity[drop] * c->water_mass[drop];
  }
  return result;
}

/* calculate_ml_new, cm.py:408-570 */
static MlNew calculate_ml_new(const Cell *c, double timestep, int fake, double T, double p,
                              double RH, double Sc, double lv, double pvs, double DTp,
                              double KTp, double rtol_x) {
  const cf_k *k = c->k;
  MlNew out = {0, 1, 0, 0, 0};
  int64_t n_activated_and_growing = 0;
  const double lambdaK = cf_lambdaK(k, T, p);
  const double lambdaD = cf_lambdaD(k, DTp, T);
  const int film = CF_O(SURFACE_TENSION) != SDM_COND_SGM_CONSTANT;
  const int ventilated = CF_O(VENTILATION) != SDM_COND_VENT_NEGLECT;
  for (int64_t i = 0; i < c->n_in_cell; ++i) {
    const int64_t drop = c->cell_idx[i];
    const double m = c->water_mass[drop];
    if (m <= 0) continue;
    const double f_org = film ? c->f_org[drop] : 0.0;
    const double v_drop = m / CF_C(RHO_W);
    const double x_old = cf_x(k, m);
    const double r_old = cf_radius(k, v_drop);
    const double x_insane = cf_x(k, CF_C(RHO_W) * (c->vdry[drop] / 100));
    const double rd3 = c->vdry[drop] / CF_C(PI_4_3);
    MinArgs args = {x_old, timestep, c->kappa[drop], f_org, rd3, T, RH, 0, 0, 0};
    const double sgm = cf_sigma(k, T, v_drop, c->vdry[drop], f_org, &args.fail);
    const double RH_eq = cf_RH_eq(k, r_old, T, c->kappa[drop], rd3, sgm);
    double dx_old;
    if (!within_tolerance(sdm_abs(RH - RH_eq), RH, c->RH_rtol)) {
      const double Dr = cf_kinetics_D(k, DTp, r_old, lambdaD);
      const double Kr = cf_kinetics_K(k, KTp, r_old, lambdaK);
      const double mass_ventilation_factor =
          cf_ventilation_factor(k, ventilated ? c->reynolds_number[drop] : 0.0, Sc);
      const double heat_ventilation_factor = mass_ventilation_factor;
      args.Fk = cf_Fk(k, T, Kr * heat_ventilation_factor, lv);
      args.Fd = cf_Fd(k, T, Dr * mass_ventilation_factor, pvs);
      const double r_dr_dt_old = cf_r_dr_dt(k, RH_eq, RH, args.Fk, args.Fd);
      const double mass_old = cf_mass(k, x_old);
      const double dm_dt_old = dm_dt_of(k, r_old, r_dr_dt_old);
      dx_old = timestep * cf_dx_dt(k, mass_old, dm_dt_old);
    } else {
      dx_old = 0.0;
    }
    double x_new;
    if (dx_old == 0) {
      x_new = x_old;
    } else {
      double a = x_old;
      double b = cf_py_max(x_insane, a + dx_old);
      double fa = minfun(k, a, &args);
      double fb = minfun(k, b, &args);
      int counter = 0;
      while (!(fa * fb < 0)) {
        counter += 1;
        if (counter > c->max_iters) {
          out.success = 0;
          break;
        }
        b = cf_py_max(x_insane, a + dx_old * sdm_pow2i(counter)); /* math.ldexp */
        fb = minfun(k, b, &args);
      }
      if (!out.success) break;
      if (a != b) {
        if (a > b) {
          double t = a; a = b; b = t;
          t = fa; fa = fb; fb = t;
        }
        int iters_taken;
        x_new = solve(k, &args, a, b, fa, fb, rtol_x, c->max_iters, &iters_taken);
        if (iters_taken == -1 || iters_taken == c->max_iters) {
          out.success = 0;
          break;
        }
      } else {
        x_new = x_old;
      }
    }
    if (args.fail) { /* the reference's assert in CompressedFilmRuehl.sigma: a failed droplet */
      out.success = 0;
      break;
    }
    const double mass_new = cf_mass(k, x_new);
    const double mass_cr = CF_C(RHO_W) * c->v_cr[drop];
    out.result += (double)c->multiplicity[drop] * mass_new;
    if (!fake) {
      const int64_t n = c->multiplicity[drop];
      if (mass_new > mass_cr && mass_new > m) n_activated_and_growing += n;
      if (mass_new > mass_cr && mass_cr > m) out.n_activating += n;
      if (mass_new < mass_cr && mass_cr < m) out.n_deactivating += n;
      c->water_mass[drop] = mass_new;
    }
  }
  out.n_ripening = out.n_deactivating > 0 ? n_activated_and_growing : 0;
  return out;
}

typedef struct {
  double qv, thd, RH_max;
  int64_t n_activating, n_deactivating, n_ripening;
  int success;
} StepOut;

typedef struct {
  double thd, qv, rhod, dthd_dt, dqv_dt, drhod_dt, m_d, rtol_x, air_density,
      air_dynamic_viscosity;
} StepArgs;

/* step_impl, cm.py:249-357 */
static StepOut step_impl(const Cell *c, const StepArgs *s, double timestep, int64_t n_substeps,
                         int fake) {
  const cf_k *k = c->k;
  double thd = s->thd, qv = s->qv, rhod = s->rhod;
  timestep /= (double)n_substeps;
  double ml_old = calculate_ml_old(c);
  StepOut o = {0, 0, 0, 0, 0, 0, 1};
  for (int64_t it = 0; it < n_substeps; ++it) {
    thd += timestep * s->dthd_dt / 2;
    qv += timestep * s->dqv_dt / 2;
    rhod += timestep * s->drhod_dt / 2;
    const double T = cf_svt_T(k, rhod, thd);
    const double p = cf_svt_p(k, rhod, T, qv);
    const double pv = cf_svt_pv(k, p, qv);
    const double lv = cf_lv(k, T);
    const double pvs = cf_pvs_water(k, T);
    const double DTp = cf_thermics_D(k, T, p), KTp = cf_thermics_K(k, T, p);
    const double RH = pv / pvs;
    const double Sc = CF_O(VENTILATION) != SDM_COND_VENT_NEGLECT
                          ? cf_air_schmidt_number(s->air_dynamic_viscosity, DTp, s->air_density)
                          : 0.0;
    const MlNew mn =
        calculate_ml_new(c, timestep, fake, T, p, RH, Sc, lv, pvs, DTp, KTp, s->rtol_x);
    const double dml_dt = (mn.result - ml_old) / timestep;
    const double dqv_corr = -dml_dt / s->m_d;
    /* state_variable_triplet/libcloudphplusplus.py: dthd_dt */
    const double dthd_dt_corr = -lv * dqv_corr / CF_C(C_PD) / T * thd * rhod;
    thd += timestep * (s->dthd_dt / 2 + dthd_dt_corr);
    qv += timestep * (s->dqv_dt / 2 + dqv_corr);
    rhod += timestep * s->drhod_dt / 2;
    ml_old = mn.result;
    o.n_activating += mn.n_activating;
    o.n_deactivating += mn.n_deactivating;
    o.n_ripening += mn.n_ripening;
    o.RH_max = cf_py_max(o.RH_max, RH);
    o.success = o.success && mn.success;
  }
  o.qv = qv;
  o.thd = thd;
  return o;
}

/* step_fake, cm.py:231-238 */
static double step_fake(const Cell *c, const StepArgs *s, double dt, int64_t n_substeps,
                        int *success) {
  dt /= (double)n_substeps;
  const StepOut o = step_impl(c, s, dt, 1, 1);
  *success = o.success;
  return o.thd;
}

typedef struct {
  int64_t n_min, n_max;
  double timestep, rtol_thd;
  int adaptive, fuse, multiplier;
} Adapt;

/* adapt_substeps, cm.py:190-227; returns n_substeps, *success */
static int64_t adapt_substeps(const Cell *c, const StepArgs *s, const Adapt *ad,
                              int64_t n_substeps, double thd, int *success) {
  const int64_t mult = ad->multiplier;
  int64_t fd = floordiv(n_substeps, mult);
  n_substeps = fd > ad->n_min ? fd : ad->n_min;
  *success = 0;
  double thd_new_long = 0;
  for (int burnout = 0; burnout < ad->fuse + 1; ++burnout) {
    if (burnout == ad->fuse) { *success = 0; return 0; }
    thd_new_long = step_fake(c, s, ad->timestep, n_substeps, success);
    if (*success) break;
    n_substeps *= mult;
  }
  for (int burnout = 0; burnout < ad->fuse + 1; ++burnout) {
    if (burnout == ad->fuse) { *success = 0; return 0; }
    const double thd_new_short = step_fake(c, s, ad->timestep, n_substeps * mult, success);
    if (!*success) return 0;
    const double dthd_long = thd_new_long - thd;
    const double dthd_short = thd_new_short - thd;
    const double error_estimate = sdm_abs(dthd_long - (double)mult * dthd_short);
    thd_new_long = thd_new_short;
    if (within_tolerance(error_estimate, thd, ad->rtol_thd)) break;
    n_substeps *= mult;
    if (n_substeps > ad->n_max) break;
  }
  return ad->n_max < n_substeps ? ad->n_max : n_substeps;
}

API int sdm_condensation_f(sdm_ctx *ctx, int64_t n_sd, int64_t n_cell,
                           const int64_t *cell_start_arg, double *water_mass, const double *v_cr,
                           const int64_t *multiplicity, const double *vdry, const int64_t *idx,
                           const double *rhod, const double *thd,
                           const double *water_vapour_mixing_ratio, double dv,
                           const double *prhod, double *pthd,
                           double *predicted_water_vapour_mixing_ratio, const double *kappa,
                           const double *f_org, double rtol_x, double rtol_thd, double timestep,
                           int64_t *n_substeps, int64_t *n_activating, int64_t *n_deactivating,
                           int64_t *n_ripening, const int64_t *cell_order, double *RH_max,
                           uint8_t *success, const double *reynolds_number,
                           const double *air_density, const double *air_dynamic_viscosity,
                           double dt_min, double dt_max, int adaptive, int fuse, int multiplier,
                           double RH_rtol, int max_iters, const double consts[34],
                           const sdm_cond_formulae *formulae) {
  (void)ctx;
  if (n_sd < 0 || n_cell < 0 || multiplier < 1 || fuse < 0 || max_iters < 0)
    FAIL(SDM_E_ARG, "sdm_condensation_f: bad size or solver parameter");
  cf_k kk;
  if (!formulae_of(consts, formulae, &kk))
    FAIL(SDM_E_ARG, "sdm_condensation_f: missing or unknown formulae");
  const cf_k *k = &kk;
  const int ventilated = CF_O(VENTILATION) != SDM_COND_VENT_NEGLECT;
  if (n_sd > 0 && ((CF_O(SURFACE_TENSION) != SDM_COND_SGM_CONSTANT && !f_org) ||
                   (ventilated && !reynolds_number)))
    FAIL(SDM_E_ARG, "sdm_condensation_f: the formulae need f_org / reynolds_number");
  if (ventilated && (!air_density || !air_dynamic_viscosity))
    FAIL(SDM_E_ARG, "sdm_condensation_f: ventilation needs air_density / air_dynamic_viscosity");
  /* make_adapt_substeps, cm.py:181-188 */
  if (dt_max > timestep) dt_max = timestep;
  if (dt_min == 0) FAIL(SDM_E_ARG, "sdm_condensation_f: dt_range[0] == 0 is not implemented");
  Adapt ad = {(int64_t)ceil(timestep / dt_max), (int64_t)floor(timestep / dt_min), timestep,
              rtol_thd, adaptive, fuse, multiplier};
  for (int64_t i = 0; i < n_cell; ++i) { /* _condensation, cm.py:102-176 */
    const int64_t cell_id = cell_order[i];
    const int64_t cell_start = cell_start_arg[cell_id];
    const int64_t cell_end = cell_start_arg[cell_id + 1];
    const int64_t n_sd_in_cell = cell_end - cell_start;
    if (n_sd_in_cell == 0) continue;
    const Cell c = {k, water_mass, v_cr, vdry, kappa, f_org, reynolds_number, multiplicity,
                    idx + cell_start, n_sd_in_cell, RH_rtol, max_iters};
    const StepArgs s = {thd[cell_id], water_vapour_mixing_ratio[cell_id], rhod[cell_id],
                        (pthd[cell_id] - thd[cell_id]) / timestep,
                        (predicted_water_vapour_mixing_ratio[cell_id] -
                         water_vapour_mixing_ratio[cell_id]) / timestep,
                        (prhod[cell_id] - rhod[cell_id]) / timestep,
                        (prhod[cell_id] + rhod[cell_id]) / 2 * dv, rtol_x,
                        ventilated ? air_density[cell_id] : 0.0,
                        ventilated ? air_dynamic_viscosity[cell_id] : 0.0};
    /* solve, cm.py:636-698 */
    int ok = 1;
    int64_t n = n_substeps[cell_id];
    if (adaptive) n = adapt_substeps(&c, &s, &ad, n, s.thd, &ok);
    StepOut o;
    if (ok) {
      o = step_impl(&c, &s, timestep, n, 0);
      ok = o.success;
    } else {
      o = (StepOut){s.qv, s.thd, -1, -1, -1, -1, 0};
    }
    success[cell_id] = (uint8_t)(ok != 0);
    predicted_water_vapour_mixing_ratio[cell_id] = o.qv;
    pthd[cell_id] = o.thd;
    n_substeps[cell_id] = n;
    n_activating[cell_id] = o.n_activating;
    n_deactivating[cell_id] = o.n_deactivating;
    n_ripening[cell_id] = o.n_ripening;
    RH_max[cell_id] = o.RH_max;
  }
  return SDM_OK;
}

/* ---- ambient methods (pm.py) ------------------------------------------------------------------ */
API int sdm_temperature_pressure_rh_f(sdm_ctx *ctx, const double *rhod, const double *thd,
                                      const double *qv, double *T, double *p, double *RH,
                                      int64_t n, const double consts[34],
                                      const sdm_cond_formulae *formulae) {
  (void)ctx;
  cf_k kk;
  if (!formulae_of(consts, formulae, &kk))
    FAIL(SDM_E_ARG, "sdm_temperature_pressure_rh_f: missing or unknown formulae");
  const cf_k *k = &kk;
  for (int64_t i = 0; i < n; ++i) { /* :53-61 */
    T[i] = cf_svt_T(k, rhod[i], thd[i]);
    p[i] = cf_svt_p(k, rhod[i], T[i], qv[i]);
    RH[i] = cf_svt_pv(k, p[i], qv[i]) / cf_pvs_water(k, T[i]);
  }
  return SDM_OK;
}

API int sdm_critical_volume_f(sdm_ctx *ctx, double *v_cr, const double *kappa,
                              const double *f_org, const double *v_dry, const double *v_wet,
                              const double *T, const int64_t *cell, int64_t n,
                              const double consts[34], const sdm_cond_formulae *formulae) {
  (void)ctx;
  cf_k kk;
  if (!formulae_of(consts, formulae, &kk))
    FAIL(SDM_E_ARG, "sdm_critical_volume_f: missing or unknown formulae");
  const cf_k *k = &kk;
  const int film = CF_O(SURFACE_TENSION) != SDM_COND_SGM_CONSTANT;
  if (n > 0 && film && (!f_org || !v_wet))
    FAIL(SDM_E_ARG, "sdm_critical_volume_f: the surface tension needs f_org and v_wet");
  for (int64_t i = 0; i < n; ++i) { /* :22-33 */
    int fail = 0;
    const double sigma = cf_sigma(k, T[cell[i]], film ? v_wet[i] : 0.0, v_dry[i],
                                  film ? f_org[i] : 0.0, &fail);
    const double r_cr = cf_r_cr(k, kappa[i], v_dry[i] / CF_C(PI_4_3), T[cell[i]], sigma);
    v_cr[i] = fail ? sdm_nan() : cf_volume(k, r_cr);
  }
  return SDM_OK;
}

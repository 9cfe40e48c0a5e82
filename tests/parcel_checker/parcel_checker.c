/*
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_parcel.h.
 *
 * sdm_parcel_run for host pointers as the loop the header writes out: per parcel and time step
 * the advance of the parcel's variables in plain doubles (environments/parcel.py:101-134 with
 * hydrostatics ConstantGVapourMixingRatioAndThetaStd.drho_dz inlined, left to right), then the
 * STAGE symbols of the two condensation checkers, which this library links against
 * (tests/checker/, tests/condensation_formulae_checker/): sdm_critical_volume(_f),
 * sdm_condensation(_f) with n_cell = 1 on the parcel's slice of the columns, and
 * sdm_temperature_pressure_rh(_f).  The solver is not restated here.  The latent heat is
 * csrc/condensation_formulae.h's cf_lv, the header the product compiles too.  The context is
 * ignored.  Built by __graft_entry__.build() next to this file (git-ignored), after the two
 * checkers it links against; nothing in pysdm_amd/ loads it.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* (the translation unit is compiled with hidden visibility: the stage symbols live in other
 * shared objects, and sdm_parcel_run is this one's export) */
#pragma GCC visibility push(default)
#include "../../include/sdm_parcel.h"
#pragma GCC visibility pop
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

API int sdm_parcel_run(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, int64_t n_steps,
                       int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start,
                       double *water_mass, const int64_t *multiplicity, const double *vdry,
                       const double *kappa, const double *f_org, double *v_cr,
                       const sdm_parcel_state *st, const double *w_mid,
                       const sdm_parcel_profile *profile, const double consts[34],
                       const sdm_cond_formulae *formulae) {
  if (!cfg || !consts || !st || n_steps < 0 || n_parcel < 0 || n_sd < 0)
    FAIL(SDM_E_ARG, "sdm_parcel_run: bad size or missing argument");
  if (cfg->dt_min == 0) FAIL(SDM_E_ARG, "sdm_parcel_run: dt_min == 0 is not implemented");
  if (formulae && formulae->option[SDM_COND_OPT_VENTILATION] != SDM_COND_VENT_NEGLECT)
    FAIL(SDM_E_ARG, "sdm_parcel_run: ventilation stays on the stage route");
  if (n_parcel == 0 || n_steps == 0) return SDM_OK;
  if (parcel_start[0] < 0 || parcel_start[n_parcel] > n_sd)
    FAIL(SDM_E_ARG, "sdm_parcel_run: parcel_start outside the columns");
  int64_t n_most = 0;
  for (int64_t c = 0; c < n_parcel; ++c) {
    const int64_t n = parcel_start[c + 1] - parcel_start[c];
    if (n <= 0) FAIL(SDM_E_ARG, "sdm_parcel_run: a parcel has no rows");
    if (n > n_most) n_most = n;
  }
  cf_k kk;
  memset(&kk, 0, sizeof(kk));
  for (int i = 0; i < SDM_COND_N_CONSTS; ++i) kk.c[i] = consts[i];
  if (formulae) {
    for (int i = 0; i < SDM_COND_F_N_CONSTS; ++i) kk.f[i] = formulae->consts[i];
    for (int i = 0; i < SDM_COND_N_OPTS; ++i) kk.o[i] = formulae->option[i];
  }
  const cf_k *k = &kk;
  const sdm_parcel_profile none = {0};
  const sdm_parcel_profile *pr = profile ? profile : &none;
  const double dt = cfg->dt;

  double *v_wet = malloc((size_t)n_most * sizeof(double));
  double *backup = malloc((size_t)n_most * sizeof(double));
  int64_t *identity = malloc((size_t)n_most * sizeof(int64_t));
  int64_t *zeros = calloc((size_t)n_most, sizeof(int64_t));
  if (!v_wet || !backup || !identity || !zeros) {
    free(v_wet); free(backup); free(identity); free(zeros);
    FAIL(SDM_E_NOMEM, "sdm_parcel_run: out of memory");
  }
  for (int64_t q = 0; q < n_most; ++q) identity[q] = q;
  int rc = SDM_OK;

  for (int64_t c = 0; c < n_parcel && rc == SDM_OK; ++c) {
    if (st->failed_step[c] >= 0) continue; /* skipped for good */
    const int64_t row0 = parcel_start[c], n = parcel_start[c + 1] - row0;
    const int64_t cell_start[2] = {0, n}, cell_order[1] = {0};
    const double *forg = f_org ? f_org + row0 : NULL;
    for (int64_t j = 0; j < n_steps && rc == SDM_OK; ++j) {
      const double T = st->T[c], p = st->p[c], rhod = st->rhod[c], qv = st->qv[c];
      const double thd = st->thd[c];
      const double w = w_mid[j * n_parcel + c];
      const double delta = st->qv_prev[c] - qv;
      const double qv_mid = qv - delta / 2;
      const double lv = cf_lv(k, T);
      const double Rq = CF_C(RV) / (1 / qv_mid + 1) + CF_C(RD) / (1 + qv_mid);
      const double cp = CF_C(C_PV) / (1 / qv_mid + 1) + CF_C(C_PD) / (1 + qv_mid);
      const double rho = p / Rq / T;
      const double dql_dz = delta / w / dt;
      const double drho_dz =
          (cfg->g_std / T * rho * (Rq / cp - 1) - p * lv / cp / (T * T) * dql_dz) / Rq;
      const double z = st->z[c] + dt * w;
      const double prhod = rhod + dt * (w * drho_dz);
      const double dv = st->mass_of_dry_air[c] / ((prhod + rhod) / 2);

      for (int64_t q = 0; q < n; ++q) {
        backup[q] = water_mass[row0 + q];
        v_wet[q] = water_mass[row0 + q] / CF_C(RHO_W);
      }
      rc = formulae ? sdm_critical_volume_f(ctx, v_cr + row0, kappa + row0, forg, vdry + row0,
                                            v_wet, &T, zeros, n, consts, formulae)
                    : sdm_critical_volume(ctx, v_cr + row0, kappa + row0, forg, vdry + row0,
                                          v_wet, &T, zeros, n, consts);
      if (rc != SDM_OK) break;

      double pthd = thd, pqv = qv, RH_max = 0;
      int64_t n_sub = st->n_substeps[c], n_act = 0, n_deact = 0, n_rip = 0;
      uint8_t success = 0;
      rc = formulae
               ? sdm_condensation_f(ctx, n, 1, cell_start, water_mass + row0, v_cr + row0,
                                    multiplicity + row0, vdry + row0, identity, &rhod, &thd, &qv,
                                    dv, &prhod, &pthd, &pqv, kappa + row0, forg, cfg->rtol_x,
                                    cfg->rtol_thd, dt, &n_sub, &n_act, &n_deact, &n_rip,
                                    cell_order, &RH_max, &success, NULL, NULL, NULL, cfg->dt_min,
                                    cfg->dt_max, cfg->adaptive, cfg->fuse, cfg->multiplier,
                                    cfg->RH_rtol, cfg->max_iters, consts, formulae)
               : sdm_condensation(ctx, n, 1, cell_start, water_mass + row0, v_cr + row0,
                                  multiplicity + row0, vdry + row0, identity, &rhod, &thd, &qv,
                                  dv, &prhod, &pthd, &pqv, kappa + row0, forg, cfg->rtol_x,
                                  cfg->rtol_thd, dt, &n_sub, &n_act, &n_deact, &n_rip, cell_order,
                                  &RH_max, &success, NULL, NULL, NULL, cfg->dt_min, cfg->dt_max,
                                  cfg->adaptive, cfg->fuse, cfg->multiplier, cfg->RH_rtol,
                                  cfg->max_iters, consts);
      if (rc != SDM_OK) break;
      if (!success) { /* the parcel stops with its state as before the step */
        for (int64_t q = 0; q < n; ++q) water_mass[row0 + q] = backup[q];
        st->failed_step[c] = st->steps_done[c];
        break;
      }
      st->qv_prev[c] = qv;
      st->z[c] = z;
      st->rhod[c] = prhod;
      st->thd[c] = pthd;
      st->qv[c] = pqv;
      rc = formulae ? sdm_temperature_pressure_rh_f(ctx, st->rhod + c, st->thd + c, st->qv + c,
                                                    st->T + c, st->p + c, st->RH + c, 1, consts,
                                                    formulae)
                    : sdm_temperature_pressure_rh(ctx, st->rhod + c, st->thd + c, st->qv + c,
                                                  st->T + c, st->p + c, st->RH + c, 1, consts);
      if (rc != SDM_OK) break;
      if (cfg->adaptive) { /* dynamics/condensation.py:122-131 */
        n_sub = n_sub > cfg->n_clamp_lo ? n_sub : cfg->n_clamp_lo;
        n_sub = n_sub < cfg->n_clamp_hi ? n_sub : cfg->n_clamp_hi;
      }
      st->n_substeps[c] = n_sub;
      st->n_activating[c] = n_act;
      st->n_deactivating[c] = n_deact;
      st->n_ripening[c] = n_rip;
      st->RH_max[c] = RH_max;
      st->steps_done[c] += 1;
      const int64_t at = j * n_parcel + c;
      if (pr->z) pr->z[at] = z;
      if (pr->rhod) pr->rhod[at] = prhod;
      if (pr->thd) pr->thd[at] = pthd;
      if (pr->qv) pr->qv[at] = pqv;
      if (pr->T) pr->T[at] = st->T[c];
      if (pr->p) pr->p[at] = st->p[c];
      if (pr->RH) pr->RH[at] = st->RH[c];
      if (pr->RH_max) pr->RH_max[at] = RH_max;
      if (pr->n_substeps) pr->n_substeps[at] = n_sub;
      if (pr->n_activating) pr->n_activating[at] = n_act;
      if (pr->n_deactivating) pr->n_deactivating[at] = n_deact;
      if (pr->n_ripening) pr->n_ripening[at] = n_rip;
    }
  }
  free(v_wet); free(backup); free(identity); free(zeros);
  if (rc != SDM_OK) FAIL(rc, "sdm_parcel_run: a stage symbol of the condensation checkers failed");
  return SDM_OK;
}

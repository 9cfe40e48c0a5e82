/*
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_parcel_ice.h.
 *
 * sdm_parcel_run_ice for host pointers as the loop the header writes out: per parcel and time step
 * the advance of the parcel's variables in plain doubles (as tests/parcel_checker/ writes it), then
 * nothing but STAGE symbols of the libraries this one links against:
 *   tests/checker/ and tests/condensation_formulae_checker/: sdm_temperature_pressure_rh(_f),
 *     sdm_critical_volume(_f) (copied back for the liquid rows only), sdm_condensation(_f) with
 *     n_cell = 1 on the parcel's slice;
 *   tests/freezing_checker/: sdm_a_w_ice, sdm_freezing_step with n_cell = 1, volume = NULL and the
 *     parcel's own stream;
 *   tests/deposition_checker/: sdm_deposition with n_cell = 1 and cell_volume = the step's dv.
 * No solver, no row arithmetic and no generator is restated.  The ice profile's mass is the SUM of
 * include/sdm_parcel_diag.h, written out here add for add.  The latent heat is
 * csrc/condensation_formulae.h's cf_lv, the header the product compiles too.  The context is
 * ignored.  Built by __graft_entry__.build() next to this file (git-ignored), after the libraries
 * it links against; nothing in pysdm_amd/ loads it.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#pragma GCC visibility push(default)
#include "../../include/sdm_parcel_ice.h"
#pragma GCC visibility pop
#include "../../pysdm_amd/csrc/sdm_math.h"

#define CF_FN static inline
#include "../../pysdm_amd/csrc/condensation_formulae.h"

#define API __attribute__((visibility("default")))
#define LANES 256 /* the partials of the SUM of include/sdm_parcel_diag.h */

static __thread char g_err[256] = "";
#define FAIL(code, msg)                        \
  do {                                         \
    snprintf(g_err, sizeof(g_err), "%s", msg); \
    return (code);                             \
  } while (0)

API const char *sdm_last_error(void) { return g_err; }

API int parcel_ice_checker_cfg_size(void) { return (int)sizeof(sdm_parcel_ice_cfg); }

/* the SUM of include/sdm_parcel_diag.h of multiplicity * (-m) over the rows with m < 0 */
static double ice_mass_of(const double *m, const int64_t *mult, int64_t n) {
  double partial[LANES];
  for (int j = 0; j < LANES; ++j) partial[j] = 0.0;
  for (int64_t q = 0; q < n; ++q)
    if (m[q] < 0) partial[q % LANES] += (double)mult[q] * (-m[q]);
  for (int stride = LANES / 2; stride >= 1; stride /= 2)
    for (int j = 0; j < stride; ++j) partial[j] = partial[j] + partial[j + stride];
  return partial[0];
}

API int sdm_parcel_run_ice(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, const sdm_parcel_ice_cfg *ic,
                           int64_t n_steps, int64_t n_parcel, int64_t n_sd,
                           const int64_t *parcel_start, double *water_mass,
                           const int64_t *multiplicity, const double *vdry, const double *kappa,
                           const double *f_org, double *v_cr, const sdm_parcel_state *st,
                           const double *w_mid, const sdm_parcel_profile *profile,
                           const double consts[34], const sdm_cond_formulae *formulae,
                           const sdm_parcel_ice_state *is, const sdm_parcel_ice_profile *ice_profile,
                           const double frz_consts[33], const double dep_consts[39]) {
  if (!ic || !is || !frz_consts) FAIL(SDM_E_ARG, "sdm_parcel_run_ice: missing argument");
  const int freezing = ic->freezing != 0, deposition = ic->deposition != 0;
  if (!freezing && !deposition)
    FAIL(SDM_E_ARG, "sdm_parcel_run_ice: both passes off (that is sdm_parcel_run)");
  if (ic->order != SDM_PARCEL_ICE_FREEZING_FIRST && ic->order != SDM_PARCEL_ICE_DEPOSITION_FIRST)
    FAIL(SDM_E_ARG, "sdm_parcel_run_ice: unknown order");
  if (!is->a_w_ice || !is->RH_ice || !is->n_exceeded)
    FAIL(SDM_E_ARG, "sdm_parcel_run_ice: the carried pair or n_exceeded is missing");
  const int imm_singular = freezing && ic->immersion_freezing && ic->singular;
  const int imm_td = freezing && ic->immersion_freezing && !ic->singular;
  const int hom = freezing && ic->homogeneous_freezing;
  if (imm_singular && !is->freezing_temperature)
    FAIL(SDM_E_ARG, "sdm_parcel_run_ice: singular freezing without freezing_temperature");
  if (imm_td && !is->immersed_surface_area)
    FAIL(SDM_E_ARG, "sdm_parcel_run_ice: time-dependent freezing without immersed_surface_area");
  if ((imm_td || hom) && (!is->rng_offset || !is->rng_state_inc))
    FAIL(SDM_E_ARG, "sdm_parcel_run_ice: a stochastic pass without a stream");
  if (deposition && !dep_consts) FAIL(SDM_E_ARG, "sdm_parcel_run_ice: dep_consts missing");
  if (!cfg || !consts || !st || n_steps < 0 || n_parcel < 0 || n_sd < 0)
    FAIL(SDM_E_ARG, "sdm_parcel_run_ice: bad size or missing argument");
  if (cfg->dt_min == 0) FAIL(SDM_E_ARG, "sdm_parcel_run_ice: dt_min == 0 is not implemented");
  if (formulae && formulae->option[SDM_COND_OPT_VENTILATION] != SDM_COND_VENT_NEGLECT)
    FAIL(SDM_E_ARG, "sdm_parcel_run_ice: ventilated ice is not served");
  if (n_parcel == 0 || n_steps == 0) return SDM_OK;
  if (parcel_start[0] < 0 || parcel_start[n_parcel] > n_sd)
    FAIL(SDM_E_ARG, "sdm_parcel_run_ice: parcel_start outside the columns");
  int64_t n_most = 0;
  for (int64_t c = 0; c < n_parcel; ++c) {
    const int64_t n = parcel_start[c + 1] - parcel_start[c];
    if (n <= 0) FAIL(SDM_E_ARG, "sdm_parcel_run_ice: a parcel has no rows");
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
  const sdm_parcel_ice_profile ice_none = {0};
  const sdm_parcel_ice_profile *ipr = ice_profile ? ice_profile : &ice_none;
  const double dt = cfg->dt;

  double *v_wet = malloc((size_t)n_most * sizeof(double));
  double *v_cr_all = malloc((size_t)n_most * sizeof(double));
  double *backup = malloc((size_t)n_most * sizeof(double));
  int64_t *identity = malloc((size_t)n_most * sizeof(int64_t));
  int64_t *zeros = calloc((size_t)n_most, sizeof(int64_t));
  if (!v_wet || !v_cr_all || !backup || !identity || !zeros) {
    free(v_wet); free(v_cr_all); free(backup); free(identity); free(zeros);
    FAIL(SDM_E_NOMEM, "sdm_parcel_run_ice: out of memory");
  }
  for (int64_t q = 0; q < n_most; ++q) identity[q] = q;
  int rc = SDM_OK;

  for (int64_t c = 0; c < n_parcel && rc == SDM_OK; ++c) {
    if (st->failed_step[c] >= 0) continue; /* skipped for good */
    const int64_t row0 = parcel_start[c], n = parcel_start[c + 1] - row0;
    const int64_t cell_start[2] = {0, n}, cell_order[1] = {0};
    const double *forg = f_org ? f_org + row0 : NULL;
    sdm_freezing_cfg fcfg;
    memset(&fcfg, 0, sizeof(fcfg));
    fcfg.singular = ic->singular;
    fcfg.immersion_freezing = ic->immersion_freezing;
    fcfg.homogeneous_freezing = ic->homogeneous_freezing;
    fcfg.thaw = ic->thaw;
    fcfg.j_het = ic->j_het;
    fcfg.j_hom = ic->j_hom;
    fcfg.rates = SDM_FRZ_RATES_AUTO;
    fcfg.timestep = dt;
    if (imm_td || hom)
      for (int i = 0; i < 4; ++i) fcfg.rng_state_inc[i] = is->rng_state_inc[4 * c + i];
    for (int64_t j = 0; j < n_steps && rc == SDM_OK; ++j) {
      /* 1: the advance */
      const double T = st->T[c], p = st->p[c], RH = st->RH[c], rhod = st->rhod[c];
      const double qv = st->qv[c], thd = st->thd[c];
      const double a_w_ice = is->a_w_ice[c], RH_ice = is->RH_ice[c];
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

      /* 2: Moist.sync - the pair the next step reads */
      double sync_T, sync_p, sync_RH, a_w_ice_new, RH_ice_new;
      rc = formulae ? sdm_temperature_pressure_rh_f(ctx, &prhod, &thd, &qv, &sync_T, &sync_p,
                                                    &sync_RH, 1, consts, formulae)
                    : sdm_temperature_pressure_rh(ctx, &prhod, &thd, &qv, &sync_T, &sync_p,
                                                  &sync_RH, 1, consts);
      if (rc != SDM_OK) break;
      rc = sdm_a_w_ice(ctx, &sync_T, &sync_p, &sync_RH, &qv, &a_w_ice_new, &RH_ice_new, 1,
                       frz_consts);
      if (rc != SDM_OK) break;

      /* 3: the critical volume of the liquid rows */
      for (int64_t q = 0; q < n; ++q) {
        backup[q] = water_mass[row0 + q];
        v_wet[q] = water_mass[row0 + q] / CF_C(RHO_W);
      }
      rc = formulae ? sdm_critical_volume_f(ctx, v_cr_all, kappa + row0, forg, vdry + row0, v_wet,
                                            &T, zeros, n, consts, formulae)
                    : sdm_critical_volume(ctx, v_cr_all, kappa + row0, forg, vdry + row0, v_wet,
                                          &T, zeros, n, consts);
      if (rc != SDM_OK) break;
      for (int64_t q = 0; q < n; ++q)
        if (backup[q] > 0) v_cr[row0 + q] = v_cr_all[q];

      /* 4: condensation */
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
      double nT, np, nRH;
      rc = formulae ? sdm_temperature_pressure_rh_f(ctx, &prhod, &pthd, &pqv, &nT, &np, &nRH, 1,
                                                    consts, formulae)
                    : sdm_temperature_pressure_rh(ctx, &prhod, &pthd, &pqv, &nT, &np, &nRH, 1,
                                                  consts);
      if (rc != SDM_OK) break;

      /* 5: the ice passes on the CURRENT T, p, RH, a_w_ice, RH_ice, qv, rhod, thd */
      int64_t exceeded = 0;
      for (int pass = 0; pass < 2 && rc == SDM_OK; ++pass) {
        const int freeze_now = (pass == 0) == (ic->order == SDM_PARCEL_ICE_FREEZING_FIRST);
        if (freeze_now && freezing) {
          rc = sdm_freezing_step(
              ctx, &fcfg, (imm_td || hom) ? is->rng_offset[c] : 0, n, 1, water_mass + row0,
              is->freezing_temperature ? is->freezing_temperature + row0 : NULL,
              is->immersed_surface_area ? is->immersed_surface_area + row0 : NULL, NULL, zeros,
              is->temperature_of_last_freezing ? is->temperature_of_last_freezing + row0 : NULL,
              &T, &RH, &a_w_ice, &RH_ice, frz_consts);
          if (imm_td || hom) is->rng_offset[c] += (uint64_t)n * (uint64_t)(imm_td + hom);
        } else if (!freeze_now && deposition) {
          sdm_deposition_cfg dcfg;
          dcfg.coordinate = ic->coordinate;
          dcfg.capacity = ic->capacity;
          dcfg.kinetics = ic->kinetics;
          dcfg.sum = ic->sum;
          dcfg.time_step = dt;
          dcfg.cell_volume = dv;
          rc = sdm_deposition(ctx, &dcfg, n, 1, multiplicity + row0, water_mass + row0, zeros, &T,
                              &p, &RH, &a_w_ice, &qv, &rhod, &thd, &pqv, &pthd, &exceeded,
                              dep_consts);
        }
      }
      if (rc != SDM_OK) break;
      is->n_exceeded[c] += exceeded;

      /* 6: the state */
      st->qv_prev[c] = qv;
      st->z[c] = z;
      st->rhod[c] = prhod;
      st->thd[c] = pthd;
      st->qv[c] = pqv;
      st->T[c] = nT;
      st->p[c] = np;
      st->RH[c] = nRH;
      is->a_w_ice[c] = a_w_ice_new;
      is->RH_ice[c] = RH_ice_new;
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
      if (pr->T) pr->T[at] = nT;
      if (pr->p) pr->p[at] = np;
      if (pr->RH) pr->RH[at] = nRH;
      if (pr->RH_max) pr->RH_max[at] = RH_max;
      if (pr->n_substeps) pr->n_substeps[at] = n_sub;
      if (pr->n_activating) pr->n_activating[at] = n_act;
      if (pr->n_deactivating) pr->n_deactivating[at] = n_deact;
      if (pr->n_ripening) pr->n_ripening[at] = n_rip;
      /* 7: the ice profile row */
      if (ipr->a_w_ice) ipr->a_w_ice[at] = a_w_ice_new;
      if (ipr->RH_ice) ipr->RH_ice[at] = RH_ice_new;
      if (ipr->n_ice) {
        int64_t n_ice = 0;
        for (int64_t q = 0; q < n; ++q)
          if (water_mass[row0 + q] < 0) n_ice += multiplicity[row0 + q];
        ipr->n_ice[at] = n_ice;
      }
      if (ipr->ice_mass) ipr->ice_mass[at] = ice_mass_of(water_mass + row0, multiplicity + row0, n);
      if (ipr->n_exceeded) ipr->n_exceeded[at] = exceeded;
      if (ipr->dv) ipr->dv[at] = dv;
    }
  }
  free(v_wet); free(v_cr_all); free(backup); free(identity); free(zeros);
  if (rc != SDM_OK) FAIL(rc, "sdm_parcel_run_ice: a stage symbol of the checkers failed");
  return SDM_OK;
}

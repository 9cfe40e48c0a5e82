/*
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_parcel_chem.h.
 *
 * sdm_parcel_run_chem for host pointers is a loop over the steps that restates no solver: ONE step
 * of sdm_parcel_run of tests/parcel_checker/, then per parcel that carried the step out
 * sdm_chemistry_step of tests/chemistry_checker/ on the parcel's slice (n_cell = 1, an identity
 * idx, cell_volume = the step's dv from the parcel's rhod before and after the step), the two
 * element-wise updates of the header's point 4, the chemistry profile row (aq_total in the
 * summation shape of include/sdm_parcel_diag.h) and, with a request table, sdm_parcel_diagnose of
 * tests/parcel_diag_checker/ on the columns after the updates.  The shared object links against
 * the three.  The context is ignored.  Built by __graft_entry__.build() next to this file
 * (git-ignored); nothing in pysdm_amd/ loads it.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#pragma GCC visibility push(default)
#include "../../include/sdm_parcel_chem.h"
#pragma GCC visibility pop

#define API __attribute__((visibility("default")))
#define LANES 256

static __thread char g_err[256] = "";
#define FAIL(code, msg)                        \
  do {                                         \
    snprintf(g_err, sizeof(g_err), "%s", msg); \
    return (code);                             \
  } while (0)

API const char *sdm_last_error(void) { return g_err; }

/* steps 1-3 of the SUM of include/sdm_parcel_diag.h over n terms n_q * x_q */
static double diag_sum(const int64_t *multiplicity, const double *x, int64_t n) {
  double partial[LANES];
  for (int t = 0; t < LANES; ++t) {
    partial[t] = 0.0;
    for (int64_t q = t; q < n; q += LANES) partial[t] += (double)multiplicity[q] * x[q];
  }
  for (int stride = LANES / 2; stride >= 1; stride /= 2)
    for (int t = 0; t < stride; ++t) partial[t] += partial[t + stride];
  return partial[0];
}

API int sdm_parcel_run_chem(
    sdm_ctx *ctx, const sdm_parcel_cfg *cfg, const sdm_chemistry_cfg *chem_cfg, int64_t n_steps,
    int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start, double *water_mass,
    const int64_t *multiplicity, double *vdry, double *kappa, const double *f_org, double *v_cr,
    const sdm_parcel_state *st, const double *w_mid, const sdm_parcel_profile *profile,
    const double consts[34], const sdm_cond_formulae *formulae, const sdm_parcel_requests *rq,
    const sdm_parcel_diag *diag, const double *kappa_times_dry_volume, double *const moles[7],
    double *pH, uint8_t *do_chemistry_flag, double *const env_mixing_ratio[6],
    const double chem_consts[62], double dry_factor, int64_t *n_failed, int64_t *n_negative,
    int64_t *n_exceeded, const sdm_parcel_chem_profile *chem_profile) {
  if (!cfg || !chem_cfg || !chem_consts || !consts || !st)
    FAIL(SDM_E_ARG, "sdm_parcel_run_chem: missing argument");
  if (chem_cfg->n_substep < 1) FAIL(SDM_E_ARG, "sdm_parcel_run_chem: n_substep < 1");
  if (chem_cfg->system_type != SDM_CHEM_SYSTEM_OPEN &&
      chem_cfg->system_type != SDM_CHEM_SYSTEM_CLOSED)
    FAIL(SDM_E_ARG, "sdm_parcel_run_chem: unknown system_type");
  if (chem_cfg->sum != SDM_CHEM_SUM_ORDERED && chem_cfg->sum != SDM_CHEM_SUM_BLOCKED)
    FAIL(SDM_E_ARG, "sdm_parcel_run_chem: unknown sum mode");
  if (formulae && formulae->option[SDM_COND_OPT_SURFACE_TENSION] != SDM_COND_SGM_CONSTANT)
    FAIL(SDM_E_ARG, "sdm_parcel_run_chem: a surface tension other than Constant");
  const int with_diag =
      diag && (diag->moment_0 || diag->moments || diag->spectrum || diag->dv);
  if (with_diag && !rq) FAIL(SDM_E_ARG, "sdm_parcel_run_chem: outputs without requests");
  if (n_steps <= 0 || n_parcel <= 0) {
    /* (the parents' argument checks) */
    const int rc = sdm_parcel_run_diag(ctx, cfg, n_steps, n_parcel, n_sd, parcel_start, water_mass,
                                       multiplicity, vdry, kappa, f_org, v_cr, st, w_mid, profile,
                                       consts, formulae, rq, diag);
    if (rc != SDM_OK) FAIL(rc, "sdm_parcel_run_chem: sdm_parcel_run_diag refused the arguments");
    return SDM_OK;
  }
  if (!kappa_times_dry_volume || !moles || !pH || !do_chemistry_flag || !env_mixing_ratio ||
      !vdry || !kappa || !st->rhod || !st->steps_done || !st->T || !st->p ||
      !st->mass_of_dry_air || !w_mid || !parcel_start || !water_mass || !multiplicity)
    FAIL(SDM_E_ARG, "sdm_parcel_run_chem: missing column");
  for (int a = 0; a < SDM_CHEM_N_AQ; ++a)
    if (!moles[a]) FAIL(SDM_E_ARG, "sdm_parcel_run_chem: missing moles column");
  for (int g = 0; g < SDM_CHEM_N_GAS; ++g)
    if (!env_mixing_ratio[g]) FAIL(SDM_E_ARG, "sdm_parcel_run_chem: missing mixing ratio");

  double *rhod_before = malloc((size_t)n_parcel * sizeof(double));
  int64_t *done_before = malloc((size_t)n_parcel * sizeof(int64_t));
  double *volume = malloc((size_t)(n_sd > 0 ? n_sd : 1) * sizeof(double));
  int64_t *identity = malloc((size_t)(n_sd > 0 ? n_sd : 1) * sizeof(int64_t));
  int64_t *zeros = calloc((size_t)(n_sd > 0 ? n_sd : 1), sizeof(int64_t));
  if (!rhod_before || !done_before || !volume || !identity || !zeros) {
    free(rhod_before); free(done_before); free(volume); free(identity); free(zeros);
    FAIL(SDM_E_NOMEM, "sdm_parcel_run_chem: out of memory");
  }
  for (int64_t q = 0; q < n_sd; ++q) identity[q] = q;
  const double rho_w = consts[SDM_COND_K_RHO_W];
  const int64_t nm = rq ? rq->n_moments : 0, nb = rq ? rq->n_bins : 0;
  int rc = SDM_OK;
  for (int64_t j = 0; j < n_steps && rc == SDM_OK; ++j) {
    sdm_parcel_profile row;
    memset(&row, 0, sizeof(row));
    if (profile) {
      const int64_t at = j * n_parcel;
#define ROW(member) row.member = profile->member ? profile->member + at : NULL
      ROW(z); ROW(rhod); ROW(thd); ROW(qv); ROW(T); ROW(p); ROW(RH); ROW(RH_max);
      ROW(n_substeps); ROW(n_activating); ROW(n_deactivating); ROW(n_ripening);
#undef ROW
    }
    for (int64_t c = 0; c < n_parcel; ++c) {
      rhod_before[c] = st->rhod[c];
      done_before[c] = st->steps_done[c];
    }
    rc = sdm_parcel_run(ctx, cfg, 1, n_parcel, n_sd, parcel_start, water_mass, multiplicity, vdry,
                        kappa, f_org, v_cr, st, w_mid + j * n_parcel, profile ? &row : NULL,
                        consts, formulae);
    if (rc != SDM_OK) {
      snprintf(g_err, sizeof(g_err), "sdm_parcel_run_chem: sdm_parcel_run failed (%d)", rc);
      break;
    }
    for (int64_t c = 0; c < n_parcel && rc == SDM_OK; ++c) {
      if (st->steps_done[c] == done_before[c]) continue; /* failed: everything of it stays */
      const int64_t at = j * n_parcel + c;
      const int64_t row0 = parcel_start[c], n = parcel_start[c + 1] - row0;
      const double dv = st->mass_of_dry_air[c] / ((st->rhod[c] + rhod_before[c]) / 2);
      for (int64_t q = 0; q < n; ++q) volume[q] = water_mass[row0 + q] / rho_w;
      sdm_chemistry_cfg one = *chem_cfg;
      one.constants = SDM_CHEM_CONSTS_AUTO;
      one.timestep = cfg->dt;
      one.cell_volume = dv;
      const int64_t cell_start[2] = {0, n};
      double *m[SDM_CHEM_N_AQ], *mr[SDM_CHEM_N_GAS];
      for (int a = 0; a < SDM_CHEM_N_AQ; ++a) m[a] = moles[a] + row0;
      for (int g = 0; g < SDM_CHEM_N_GAS; ++g) mr[g] = env_mixing_ratio[g] + c;
      int64_t counts[3] = {0, 0, 0};
      rc = sdm_chemistry_step(ctx, &one, n, 1, identity, cell_start, zeros, multiplicity + row0,
                              volume, m, pH + row0, do_chemistry_flag + row0, st->T + c,
                              st->p + c, st->rhod + c, mr, counts, chem_consts);
      if (rc != SDM_OK) {
        snprintf(g_err, sizeof(g_err), "sdm_parcel_run_chem: sdm_chemistry_step failed (%d)", rc);
        break;
      }
      if (n_failed) n_failed[c] += counts[0];
      if (n_negative) n_negative[c] += counts[1];
      if (n_exceeded) n_exceeded[c] += counts[2];
      int64_t flagged = 0;
      for (int64_t q = row0; q < row0 + n; ++q) {
        vdry[q] = moles[SDM_CHEM_AQ_S_VI][q] * dry_factor;
        kappa[q] = kappa_times_dry_volume[q] / vdry[q];
        flagged += do_chemistry_flag[q] != 0;
      }
      if (chem_profile) {
        for (int g = 0; g < SDM_CHEM_N_GAS; ++g)
          if (chem_profile->mixing_ratio[g]) chem_profile->mixing_ratio[g][at] = mr[g][0];
        for (int a = 0; a < SDM_CHEM_N_AQ; ++a)
          if (chem_profile->aq_total[a])
            chem_profile->aq_total[a][at] = diag_sum(multiplicity + row0, m[a], n);
        if (chem_profile->n_flagged) chem_profile->n_flagged[at] = flagged;
        if (chem_profile->dv) chem_profile->dv[at] = dv;
      }
      if (with_diag) {
        if (diag->dv) diag->dv[at] = dv;
        sdm_parcel_diag out;
        out.moment_0 = diag->moment_0 ? diag->moment_0 + at * nm : NULL;
        out.moments = diag->moments ? diag->moments + at * nm : NULL;
        out.spectrum = diag->spectrum ? diag->spectrum + at * nb : NULL;
        out.dv = NULL;
        const int64_t start[2] = {row0, row0 + n};
        rc = sdm_parcel_diagnose(ctx, 1, n_sd, start, water_mass, multiplicity, vdry, kappa, f_org,
                                 st->T + c, consts, formulae, rq, &out);
        if (rc != SDM_OK)
          snprintf(g_err, sizeof(g_err), "sdm_parcel_run_chem: sdm_parcel_diagnose failed (%d)",
                   rc);
      }
    }
  }
  free(rhod_before); free(done_before); free(volume); free(identity); free(zeros);
  return rc;
}

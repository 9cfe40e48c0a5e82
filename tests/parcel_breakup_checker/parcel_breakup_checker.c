/*
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_parcel_breakup.h.
 *
 * sdm_parcel_run_collision for host pointers is the loop of tests/parcel_coal_checker/ over the
 * steps and the parcels with coal_cfg->enable_breakup as given: it restates no solver and no
 * collision code.  Per parcel that has not failed:
 *   1. its live rows are gathered into scratch columns in the order of its permutation, ONE step
 *      of sdm_parcel_run of tests/parcel_checker/ runs on them as a parcel of its own, and the
 *      water masses and critical volumes are scattered back;
 *   2. sdm_collision_step of the CPU oracle (oracle/) runs with n_cell = 1 on the parcel's rows -
 *      with breakup: the parcel's breakup counters and the position of its proc / frag stream;
 *   3. the division of point 3, the events (the overflow count included) and the records' rows.
 * The shared object links against the two.  Built by __graft_entry__.build() next to this file
 * (git-ignored); nothing in pysdm_amd/ loads it.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#pragma GCC visibility push(default)
#include "../../include/sdm_parcel_breakup.h"
#pragma GCC visibility pop

#define API __attribute__((visibility("default")))

static __thread char g_err[256] = "";
#define FAIL(code, msg)                        \
  do {                                         \
    snprintf(g_err, sizeof(g_err), "%s", msg); \
    return (code);                             \
  } while (0)

API const char *sdm_last_error(void) { return g_err; }

API int sdm_parcel_run_collision(
    sdm_ctx *ctx, const sdm_parcel_cfg *cfg, const sdm_step_cfg *coal_cfg, int64_t n_steps,
    int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start, double *water_mass,
    int64_t *multiplicity, double *vdry, double *kappa, const double *f_org, double *v_cr,
    const sdm_parcel_state *st, const double *w_mid, const sdm_parcel_profile *profile,
    const double consts[34], const sdm_cond_formulae *formulae, const sdm_parcel_coal_state *coal,
    const sdm_parcel_coal_profile *coal_profile, int fresh_idx,
    const sdm_parcel_breakup_state *breakup, const sdm_parcel_breakup_profile *breakup_profile) {
  if (!cfg || !coal_cfg || !coal || !consts || !st)
    FAIL(SDM_E_ARG, "sdm_parcel_run_collision: missing argument");
  const int with_breakup = coal_cfg->enable_breakup != 0;
  if (coal_cfg->optimized_random) FAIL(SDM_E_ARG, "sdm_parcel_run_collision: optimized_random");
  if (!coal_cfg->croupier_local)
    FAIL(SDM_E_ARG, "sdm_parcel_run_collision: croupier_local == 0 (the global croupier)");
  if (coal_cfg->velocity_source != SDM_VELOCITY_TERMINAL)
    FAIL(SDM_E_ARG, "sdm_parcel_run_collision: velocity_source other than SDM_VELOCITY_TERMINAL");
  if (formulae && formulae->option[SDM_COND_OPT_VENTILATION] != SDM_COND_VENT_NEGLECT)
    FAIL(SDM_E_ARG, "sdm_parcel_run_collision: a ventilation other than Neglect");
  if (coal_cfg->kernel < SDM_KERNEL_GOLOVIN || coal_cfg->kernel > SDM_KERNEL_LINEAR)
    FAIL(SDM_E_ARG, "sdm_parcel_run_collision: unknown kernel");
  if (with_breakup) {
    if (coal_cfg->ec < SDM_EC_CONST || coal_cfg->ec > SDM_EC_LOWLIST1982)
      FAIL(SDM_E_ARG, "sdm_parcel_run_collision: unknown ec");
    if (coal_cfg->frag < SDM_FRAG_ALWAYS_N || coal_cfg->frag > SDM_FRAG_LOWLIST1982)
      FAIL(SDM_E_ARG, "sdm_parcel_run_collision: unknown frag");
    if (coal_cfg->max_multiplicity < 1)
      FAIL(SDM_E_ARG, "sdm_parcel_run_collision: max_multiplicity < 1");
    const int needs_velocity =
        coal_cfg->ec == SDM_EC_STRAUB2010 || coal_cfg->ec == SDM_EC_LOWLIST1982 ||
        coal_cfg->frag == SDM_FRAG_STRAUB2010 || coal_cfg->frag == SDM_FRAG_LOWLIST1982;
    if (needs_velocity && coal_cfg->velocity_law == SDM_VELOCITY_LAW_GUNN_KINZER &&
        !(coal->gk_a && coal->gk_b && coal_cfg->gk_table_len > 0))
      FAIL(SDM_E_ARG, "sdm_parcel_run_collision: the breakup set-up needs a fall velocity "
                      "(gk_a, gk_b, gk_table_len)");
  }
  if (!coal_cfg->adaptive && coal_cfg->substeps < 1)
    FAIL(SDM_E_ARG, "sdm_parcel_run_collision: substeps < 1");
  if (coal_cfg->dt_min <= 0 || (coal_cfg->adaptive && coal_cfg->dt_min != coal_cfg->dt_min))
    FAIL(SDM_E_ARG, "sdm_parcel_run_collision: dt_min");
  if (n_steps <= 0 || n_parcel <= 0) {
    /* (the parent's argument checks) */
    const int rc = sdm_parcel_run(ctx, cfg, n_steps, n_parcel, n_sd, parcel_start, water_mass,
                                  multiplicity, vdry, kappa, f_org, v_cr, st, w_mid, profile,
                                  consts, formulae);
    if (rc != SDM_OK) FAIL(rc, "sdm_parcel_run_collision: sdm_parcel_run refused the arguments");
    return SDM_OK;
  }
  if (!parcel_start || !water_mass || !multiplicity || !vdry || !kappa || !v_cr || !w_mid ||
      !st->rhod || !st->steps_done || !st->failed_step || !st->mass_of_dry_air || !coal->idx ||
      !coal->n_live || !coal->kappa_times_dry_volume || !coal->collision_rate ||
      !coal->collision_rate_deficit || !coal->coalescence_rate || !coal->stats_n_substep ||
      !coal->stats_dt_min || !coal->events || !coal->rng_offset || !coal->rng_state_inc)
    FAIL(SDM_E_ARG, "sdm_parcel_run_collision: missing column");
  if (with_breakup && (!breakup || !breakup->breakup_rate || !breakup->breakup_rate_deficit ||
                       !breakup->rng_offset_breakup))
    FAIL(SDM_E_ARG, "sdm_parcel_run_collision: missing breakup column");
  if (cfg->dt_min == 0) FAIL(SDM_E_ARG, "sdm_parcel_run_collision: dt_min == 0 is not implemented");
  if (parcel_start[0] < 0 || parcel_start[n_parcel] > n_sd)
    FAIL(SDM_E_ARG, "sdm_parcel_run_collision: parcel_start outside the columns");
  int64_t most = 0;
  for (int64_t c = 0; c < n_parcel; ++c) {
    const int64_t row0 = parcel_start[c], rows = parcel_start[c + 1] - row0;
    if (rows <= 0) FAIL(SDM_E_ARG, "sdm_parcel_run_collision: a parcel has no rows");
    if (rows > SDM_PARCEL_COAL_MAX_ROWS)
      FAIL(SDM_E_ARG,
           "sdm_parcel_run_collision: a parcel of more than SDM_PARCEL_COAL_MAX_ROWS rows");
    if (rows > most) most = rows;
    if (!fresh_idx) continue;
    if (coal->n_live[c] < 1 || coal->n_live[c] > rows)
      FAIL(SDM_E_ARG, "sdm_parcel_run_collision: n_live outside 1 .. rows");
    for (int64_t p = 0; p < coal->n_live[c]; ++p)
      if (coal->idx[row0 + p] < row0 || coal->idx[row0 + p] >= row0 + rows)
        FAIL(SDM_E_ARG, "sdm_parcel_run_collision: an idx entry outside the rows of its parcel");
  }

  const size_t m = (size_t)most;
  double *g_mass = malloc(m * sizeof(double)), *g_vdry = malloc(m * sizeof(double));
  double *g_kappa = malloc(m * sizeof(double)), *g_forg = malloc(m * sizeof(double));
  double *g_vcr = malloc(m * sizeof(double)), *block = malloc(3 * m * sizeof(double));
  int64_t *g_mult = malloc(m * sizeof(int64_t)), *perm = malloc(m * sizeof(int64_t));
  int64_t *spare = malloc(m * sizeof(int64_t)), *zeros = calloc(m, sizeof(int64_t));
  int rc = SDM_OK;
  if (!g_mass || !g_vdry || !g_kappa || !g_forg || !g_vcr || !block || !g_mult || !perm ||
      !spare || !zeros) {
    snprintf(g_err, sizeof(g_err), "sdm_parcel_run_collision: out of memory");
    rc = SDM_E_NOMEM;
  }
  double *ktdv = coal->kappa_times_dry_volume;
  for (int64_t j = 0; j < n_steps && rc == SDM_OK; ++j) {
    for (int64_t c = 0; c < n_parcel && rc == SDM_OK; ++c) {
      if (st->failed_step[c] >= 0) continue; /* stopped for good */
      const int64_t at = j * n_parcel + c;
      const int64_t row0 = parcel_start[c], rows = parcel_start[c + 1] - row0;
      const int64_t n = coal->n_live[c];
      if (n < 1 || n > rows) continue;
      const int64_t *idx = coal->idx + row0;
      /* ---- 1. the parcel step over the live rows in position order ---- */
      for (int64_t p = 0; p < n; ++p) {
        const int64_t row = idx[p];
        g_mass[p] = water_mass[row];
        g_mult[p] = multiplicity[row];
        g_vdry[p] = vdry[row];
        g_kappa[p] = kappa[row];
        g_forg[p] = f_org ? f_org[row] : 0.0;
        g_vcr[p] = v_cr[row];
      }
      sdm_parcel_state one;
#define AT(member) one.member = st->member ? st->member + c : NULL
      AT(z); AT(rhod); AT(thd); AT(qv); AT(T); AT(p); AT(RH); AT(qv_prev); AT(mass_of_dry_air);
      AT(n_substeps); AT(n_activating); AT(n_deactivating); AT(n_ripening); AT(RH_max);
      AT(steps_done); AT(failed_step);
#undef AT
      sdm_parcel_profile row;
      memset(&row, 0, sizeof(row));
      if (profile) {
#define ROW(member) row.member = profile->member ? profile->member + at : NULL
        ROW(z); ROW(rhod); ROW(thd); ROW(qv); ROW(T); ROW(p); ROW(RH); ROW(RH_max);
        ROW(n_substeps); ROW(n_activating); ROW(n_deactivating); ROW(n_ripening);
#undef ROW
      }
      const double rhod_before = st->rhod[c];
      const int64_t done_before = st->steps_done[c];
      const int64_t start[2] = {0, n};
      rc = sdm_parcel_run(ctx, cfg, 1, 1, n, start, g_mass, g_mult, g_vdry, g_kappa,
                          f_org ? g_forg : NULL, g_vcr, &one, w_mid + at, profile ? &row : NULL,
                          consts, formulae);
      if (rc != SDM_OK) {
        snprintf(g_err, sizeof(g_err), "sdm_parcel_run_collision: sdm_parcel_run failed (%d)", rc);
        break;
      }
      for (int64_t p = 0; p < n; ++p) {
        water_mass[idx[p]] = g_mass[p];
        v_cr[idx[p]] = g_vcr[p];
      }
      if (st->steps_done[c] == done_before) continue; /* failed: everything else of it stays */
      const double dv = st->mass_of_dry_air[c] / ((st->rhod[c] + rhod_before) / 2);
      /* ---- 2. the collision step of the parcel as one cell ---- */
      int64_t new_live = n, n_sub = 0, n_overflow = 0;
      const int64_t coalesced_before = coal->coalescence_rate[c];
      const int64_t deficit_before = coal->collision_rate_deficit[c];
      const int64_t broken_before = with_breakup ? breakup->breakup_rate[c] : 0;
      const int64_t broken_deficit_before = with_breakup ? breakup->breakup_rate_deficit[c] : 0;
      if (rows >= 2) {
        for (int64_t p = 0; p < rows; ++p) perm[p] = p < n ? idx[p] - row0 : rows;
        memcpy(block, water_mass + row0, (size_t)rows * sizeof(double));
        memcpy(block + rows, vdry + row0, (size_t)rows * sizeof(double));
        memcpy(block + 2 * rows, ktdv + row0, (size_t)rows * sizeof(double));
        sdm_step_cfg k = *coal_cfg;
        k.n_sd = rows;
        k.n_cell = 1;
        k.n_attr = 3;
        k.mass_attr = 0;
        k.dt = cfg->dt;
        k.dv = dv;
        for (int w = 0; w < 4; ++w) k.rng_state_inc[w] = coal->rng_state_inc[4 * c + w];
        int64_t cell_idx[1] = {0}, cell_start[2] = {0, n}, ctl[8] = {n, n, 1, 1, 0, 0, 0, 0};
        double dt_left[1] = {0.0};
        sdm_step_state s;
        memset(&s, 0, sizeof(s));
        s.idx = perm;
        s.tmp_idx = spare;
        s.multiplicity = multiplicity + row0;
        s.attributes = block;
        s.cell_id = zeros;
        s.cell_idx = cell_idx;
        s.cell_start = cell_start;
        s.dt_left = dt_left;
        s.stats_dt_min = coal->stats_dt_min + c;
        s.stats_n_substep = coal->stats_n_substep + c;
        s.collision_rate = coal->collision_rate + c;
        s.collision_rate_deficit = coal->collision_rate_deficit + c;
        s.coalescence_rate = coal->coalescence_rate + c;
        if (with_breakup) {
          s.breakup_rate = breakup->breakup_rate + c;
          s.breakup_rate_deficit = breakup->breakup_rate_deficit + c;
          s.rng_offset_breakup = breakup->rng_offset_breakup[c];
        }
        s.gk_a = coal->gk_a;
        s.gk_b = coal->gk_b;
        s.velocity_params = coal->velocity_params;
        s.ctl = ctl;
        s.known_valid = -1;
        s.rng_offset = coal->rng_offset[c];
        sdm_step_result result;
        memset(&result, 0, sizeof(result));
        rc = sdm_collision_step(ctx, &k, &s, &result, SDM_STEP_READ_BACK | SDM_STEP_FRESH_CTL);
        if (rc != SDM_OK) {
          snprintf(g_err, sizeof(g_err),
                   "sdm_parcel_run_collision: sdm_collision_step failed (%d)", rc);
          break;
        }
        const int64_t *now = result.idx_swapped ? spare : perm;
        new_live = result.valid_n_sd;
        n_sub = result.n_substeps;
        for (int64_t p = 0; p < new_live; ++p) coal->idx[row0 + p] = row0 + now[p];
        memcpy(water_mass + row0, block, (size_t)rows * sizeof(double));
        memcpy(vdry + row0, block + rows, (size_t)rows * sizeof(double));
        memcpy(ktdv + row0, block + 2 * rows, (size_t)rows * sizeof(double));
        coal->rng_offset[c] = result.rng_offset;
        if (with_breakup) breakup->rng_offset_breakup[c] = result.rng_offset_breakup;
        coal->n_live[c] = new_live;
        if (ctl[7] & 0x100) coal->events[c] |= SDM_PARCEL_COAL_EVENT_DT_MIN;
        n_overflow = ctl[4];
        if (n_overflow > 0) coal->events[c] += n_overflow << SDM_PARCEL_COAL_OVERFLOW_SHIFT;
      }
      /* ---- 3. kappa of the live rows ---- */
      for (int64_t p = 0; p < new_live; ++p) {
        const int64_t r = coal->idx[row0 + p];
        kappa[r] = ktdv[r] / vdry[r];
      }
      if (coal_profile) {
        if (coal_profile->n_live) coal_profile->n_live[at] = new_live;
        if (coal_profile->n_substeps) coal_profile->n_substeps[at] = n_sub;
        if (coal_profile->coalescence_rate)
          coal_profile->coalescence_rate[at] = coal->coalescence_rate[c] - coalesced_before;
        if (coal_profile->collision_rate_deficit)
          coal_profile->collision_rate_deficit[at] =
              coal->collision_rate_deficit[c] - deficit_before;
        if (coal_profile->dv) coal_profile->dv[at] = dv;
      }
      if (with_breakup && breakup_profile) {
        if (breakup_profile->breakup_rate)
          breakup_profile->breakup_rate[at] = breakup->breakup_rate[c] - broken_before;
        if (breakup_profile->breakup_rate_deficit)
          breakup_profile->breakup_rate_deficit[at] =
              breakup->breakup_rate_deficit[c] - broken_deficit_before;
        if (breakup_profile->n_overflow) breakup_profile->n_overflow[at] = n_overflow;
      }
    }
  }
  free(g_mass); free(g_vdry); free(g_kappa); free(g_forg); free(g_vcr); free(block);
  free(g_mult); free(perm); free(spare); free(zeros);
  return rc;
}

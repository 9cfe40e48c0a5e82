/*
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_chemistry.h.
 *
 * The header in serial C: the reference's loops
 * (PySDM/backends/impl_numba/methods/chemistry_methods.py, "cm.py" below) around the per-cell and
 * per-row arithmetic of pysdm_amd/csrc/chemistry_rows.h and the TOMS748 transcription of
 * pysdm_amd/csrc/toms748.h, which the product compiles too (as it does sdm_math.h), so both sides
 * get the same bits; what checks that arithmetic against the reference is the recorded goldens.
 * Written here on their own: the loops over rows and cells, SDM_CHEM_SUM_ORDERED as the
 * reference's serial accumulation, SDM_CHEM_SUM_BLOCKED as the header's definition, literally, and
 * sdm_chemistry_step as the header's stage sequence over temporary columns (conc, dissociation
 * factors, constants), literally.  Host pointers; the context is ignored.  Built by
 * __graft_entry__.build() next to this file (git-ignored); nothing in pysdm_amd/ loads it.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/sdm_chemistry.h"
#include "../../pysdm_amd/csrc/chemistry_rows.h"

#define API __attribute__((visibility("default")))

static __thread char g_err[256] = "";
#define FAIL(code, msg)                        \
  do {                                         \
    snprintf(g_err, sizeof(g_err), "%s", msg); \
    return (code);                             \
  } while (0)

API const char *sdm_last_error(void) { return g_err; }
API int64_t chemistry_checker_cfg_size(void) { return (int64_t)sizeof(sdm_chemistry_cfg); }
API int64_t chemistry_checker_n_consts(void) { return SDM_CHEM_N_CONSTS; }

static int all_set(const void *const *p, int n) {
  if (!p) return 0;
  for (int i = 0; i < n; ++i)
    if (!p[i]) return 0;
  return 1;
}
#define ALL(p, n) all_set((const void *const *)(p), (n))

static int cfg_ok(const sdm_chemistry_cfg *cfg) {
  return cfg &&
         (cfg->system_type == SDM_CHEM_SYSTEM_OPEN || cfg->system_type == SDM_CHEM_SYSTEM_CLOSED) &&
         (cfg->sum == SDM_CHEM_SUM_ORDERED || cfg->sum == SDM_CHEM_SUM_BLOCKED) &&
         cfg->constants >= SDM_CHEM_CONSTS_AUTO && cfg->constants <= SDM_CHEM_CONSTS_PER_CELL;
}

/* cm.py:292-305 */
API int sdm_chem_recalculate_cell_data(sdm_ctx *ctx, int64_t n_cell, const double *T,
                                       double *const equilibrium[7], double *const kinetic[4],
                                       double *const henry[6], const double consts[62]) {
  (void)ctx;
  if (!consts || n_cell < 0) FAIL(SDM_E_ARG, "bad argument");
  if (n_cell == 0) return SDM_OK;
  if (!T || !ALL(equilibrium, 7) || !ALL(kinetic, 4) || !ALL(henry, 6))
    FAIL(SDM_E_ARG, "bad argument: a column is missing");
  for (int64_t c = 0; c < n_cell; ++c) {
    chem_cell cell;
    chem_cell_data(consts, T[c], &cell);
    for (int e = 0; e < 7; ++e) equilibrium[e][c] = cell.eq[e];
    for (int e = 0; e < 4; ++e) kinetic[e][c] = cell.kin[e];
    for (int g = 0; g < 6; ++g) henry[g][c] = cell.henry[g];
  }
  return SDM_OK;
}

/* cm.py:282-290 */
API int sdm_chem_recalculate_drop_data(sdm_ctx *ctx, int64_t n_sd, const double *pH,
                                       const int64_t *cell_id, const double *const equilibrium[7],
                                       double *const dissociation_factors[6],
                                       const double consts[62]) {
  (void)ctx;
  if (!consts || n_sd < 0) FAIL(SDM_E_ARG, "bad argument");
  if (n_sd == 0) return SDM_OK;
  if (!pH || !cell_id || !ALL(equilibrium, 7) || !ALL(dissociation_factors, 6))
    FAIL(SDM_E_ARG, "bad argument: a column is missing");
  for (int64_t i = 0; i < n_sd; ++i) {
    double eq[7], df[6];
    for (int e = 0; e < 7; ++e) eq[e] = equilibrium[e][cell_id[i]];
    chem_drop_data(consts, eq, pH[i], df);
    for (int g = 0; g < 6; ++g) dissociation_factors[g][i] = df[g];
  }
  return SDM_OK;
}

/* cm.py:353-429 */
API int sdm_equilibrate_H(sdm_ctx *ctx, const sdm_chemistry_cfg *cfg, int64_t n_sd,
                          const int64_t *cell_id, const double *const conc[5],
                          const double *const equilibrium[7], double *pH,
                          uint8_t *do_chemistry_flag, int64_t *n_failed, const double consts[62]) {
  (void)ctx;
  if (!cfg || !consts || n_sd < 0) FAIL(SDM_E_ARG, "bad argument");
  if (n_failed) *n_failed = 0;
  if (n_sd == 0) return SDM_OK;
  if (!cell_id || !pH || !do_chemistry_flag || !ALL(conc, 5) || !ALL(equilibrium, 7))
    FAIL(SDM_E_ARG, "bad argument: a column is missing");
  int64_t failed = 0;
  for (int64_t i = 0; i < n_sd; ++i) {
    double eq[7];
    for (int e = 0; e < 7; ++e) eq[e] = equilibrium[e][cell_id[i]];
    chem_acid q;
    chem_acid_of(consts, eq, &q);
    q.N_mIII = conc[SDM_CHEM_CONC_N_MIII][i];
    q.N_V = conc[SDM_CHEM_CONC_N_V][i];
    q.C_IV = conc[SDM_CHEM_CONC_C_IV][i];
    q.S_IV = conc[SDM_CHEM_CONC_S_IV][i];
    q.S_VI = conc[SDM_CHEM_CONC_S_VI][i];
    double now = pH[i];
    int flag = 2; /* 2: the row was left alone (cm.py:390-391) */
    failed += chem_equilibrate_row(&q, cfg->H_min, cfg->H_max, cfg->ionic_strength_threshold,
                                   cfg->rtol, &now, &flag);
    if (flag != 2) {
      pH[i] = now;
      do_chemistry_flag[i] = (uint8_t)flag;
    }
  }
  if (n_failed) *n_failed = failed;
  return SDM_OK;
}

/* the header's SDM_CHEM_SUM_BLOCKED, literally: acc = 0, blocks in order */
static double blocked_sum(const double *values, int64_t n) {
  double acc = 0.0;
  double a[SDM_CHEM_SUM_BLOCK];
  for (int64_t first = 0; first < n; first += SDM_CHEM_SUM_BLOCK) {
    const int len = (int)(n - first < SDM_CHEM_SUM_BLOCK ? n - first : SDM_CHEM_SUM_BLOCK);
    for (int j = 0; j < len; ++j) a[j] = values[first + j];
    for (int h = 128; h >= 1; h /= 2)
      for (int j = 0; j < h; ++j)
        if (j + h < len) a[j] += a[j + h];
    acc += a[0];
  }
  return acc;
}

/* cm.py:67-156 for every cell: `took[i]` marks the rows of the loop (the flag at the time of the
 * row update), dq[g * n_sd + i] their multiplicity * (new - old) */
static int apply_sums(const sdm_chemistry_cfg *cfg, int64_t n_sd, int64_t n_cell,
                      const int64_t *idx, const int64_t *cell_start, const uint8_t *took,
                      const double *dq, double *const mr[6], const double *rhod,
                      int64_t *n_exceeded, const double *consts) {
  double *list = (double *)malloc(sizeof(double) * (size_t)(n_sd > 0 ? n_sd : 1));
  if (!list) FAIL(SDM_E_ARG, "out of memory");
  for (int64_t c = 0; c < n_cell; ++c) {
    for (int g = 0; g < 6; ++g) {
      int64_t n = 0;
      double taken = 0.0; /* cm.py:131 */
      for (int64_t q = cell_start[c]; q < cell_start[c + 1]; ++q) {
        const int64_t i = idx[q];
        if (i < 0 || i >= n_sd || !took[i]) continue;
        list[n++] = dq[(int64_t)g * n_sd + i];
        taken += dq[(int64_t)g * n_sd + i]; /* cm.py:149-151 */
      }
      if (n == 0) continue; /* cm.py:81-82: no flagged row */
      if (cfg->sum == SDM_CHEM_SUM_BLOCKED) taken = blocked_sum(list, n);
      const double delta = chem_delta_mr(consts, g, taken, cfg->cell_volume, rhod[c]);
      if (!(delta <= mr[g][c]) && n_exceeded) *n_exceeded += 1; /* cm.py:154 */
      mr[g][c] -= delta;
    }
  }
  free(list);
  return SDM_OK;
}

API int sdm_dissolution(sdm_ctx *ctx, const sdm_chemistry_cfg *cfg, int64_t n_sd, int64_t n_cell,
                        const int64_t *idx, const int64_t *cell_start,
                        const uint8_t *do_chemistry_flag, double *const moles[6],
                        double *const env_mixing_ratio[6], const double *T, const double *p,
                        const double *rhod, const double *const henry[6],
                        const double *const dissociation_factors[6], const double *volume,
                        const int64_t *multiplicity, int64_t *n_negative, int64_t *n_exceeded,
                        const double consts[62]) {
  (void)ctx;
  if (!cfg_ok(cfg) || !consts || n_sd < 0 || n_cell < 1) FAIL(SDM_E_ARG, "bad argument");
  if (n_negative) *n_negative = 0;
  if (n_exceeded) *n_exceeded = 0;
  if (n_sd == 0) return SDM_OK;
  if (!idx || !cell_start || !do_chemistry_flag || !T || !p || !rhod || !volume ||
      !multiplicity || !ALL(moles, 6) || !ALL(env_mixing_ratio, 6) || !ALL(henry, 6) ||
      !ALL(dissociation_factors, 6))
    FAIL(SDM_E_ARG, "bad argument: a column is missing");
  const int closed = cfg->system_type == SDM_CHEM_SYSTEM_CLOSED;
  double *dq = NULL;
  if (closed) {
    dq = (double *)malloc(sizeof(double) * 6 * (size_t)n_sd);
    if (!dq) FAIL(SDM_E_ARG, "out of memory");
  }
  for (int64_t c = 0; c < n_cell; ++c)
    for (int64_t q = cell_start[c]; q < cell_start[c + 1]; ++q) {
      const int64_t i = idx[q];
      if (i < 0 || i >= n_sd || !do_chemistry_flag[i]) continue;
      for (int g = 0; g < 6; ++g) {
        const double old = moles[g][i];
        const double now = chem_dissolution_row(consts, g, env_mixing_ratio[g][c], henry[g][c],
                                                p[c], T[c], cfg->timestep, volume[i], old,
                                                dissociation_factors[g][i]);
        if (!(now >= 0) && n_negative) *n_negative += 1; /* cm.py:147 */
        if (dq) dq[(int64_t)g * n_sd + i] = (double)multiplicity[i] * (now - old);
        moles[g][i] = now;
      }
    }
  int rc = SDM_OK;
  if (closed)
    rc = apply_sums(cfg, n_sd, n_cell, idx, cell_start, do_chemistry_flag, dq, env_mixing_ratio,
                    rhod, n_exceeded, consts);
  free(dq);
  return rc;
}

/* cm.py:203-280 */
API int sdm_oxidation(sdm_ctx *ctx, int64_t n_sd, const int64_t *cell_id,
                      const uint8_t *do_chemistry_flag, const double *const kinetic[4],
                      const double *const equilibrium[7], double timestep, const double *volume,
                      const double *pH, const double *dissociation_factor_SO2, double *moles_O3,
                      double *moles_H2O2, double *moles_S_IV, double *moles_S_VI,
                      const double consts[62]) {
  (void)ctx;
  if (!consts || n_sd < 0) FAIL(SDM_E_ARG, "bad argument");
  if (n_sd == 0) return SDM_OK;
  if (!cell_id || !do_chemistry_flag || !volume || !pH || !dissociation_factor_SO2 ||
      !moles_O3 || !moles_H2O2 || !moles_S_IV || !moles_S_VI || !ALL(kinetic, 4) ||
      !ALL(equilibrium, 7))
    FAIL(SDM_E_ARG, "bad argument: a column is missing");
  for (int64_t i = 0; i < n_sd; ++i) {
    if (!do_chemistry_flag[i]) continue;
    const int64_t c = cell_id[i];
    double eq[7], kin[4];
    for (int e = 0; e < 7; ++e) eq[e] = equilibrium[e][c];
    for (int e = 0; e < 4; ++e) kin[e] = kinetic[e][c];
    chem_oxidation_row(consts, kin, eq, timestep, volume[i], pH[i], dissociation_factor_SO2[i],
                       &moles_O3[i], &moles_H2O2[i], &moles_S_IV[i], &moles_S_VI[i]);
  }
  return SDM_OK;
}

/* the header's definition of the step, literally: the stage symbols over temporary columns */
API int sdm_chemistry_step(sdm_ctx *ctx, const sdm_chemistry_cfg *cfg, int64_t n_sd,
                           int64_t n_cell, const int64_t *idx, const int64_t *cell_start,
                           const int64_t *cell_id, const int64_t *multiplicity,
                           const double *volume, double *const moles[7], double *pH,
                           uint8_t *do_chemistry_flag, const double *T, const double *p,
                           const double *rhod, double *const env_mixing_ratio[6], int64_t *counts,
                           const double consts[62]) {
  if (!cfg_ok(cfg) || !consts || n_sd < 0 || n_cell < 1 || cfg->n_substep < 1)
    FAIL(SDM_E_ARG, "bad argument");
  /* (where the constants come from changes no bit: one route here) */
  if (cfg->constants == SDM_CHEM_CONSTS_PER_CELL && n_cell > SDM_CHEM_LDS_CELLS)
    FAIL(SDM_E_ARG, "bad argument: SDM_CHEM_CONSTS_PER_CELL with more than SDM_CHEM_LDS_CELLS cells");
  if (counts) counts[0] = counts[1] = counts[2] = 0;
  if (n_sd == 0) return SDM_OK;
  if (!idx || !cell_start || !cell_id || !multiplicity || !volume || !pH || !do_chemistry_flag ||
      !T || !p || !rhod || !ALL(moles, 7) || !ALL(env_mixing_ratio, 6))
    FAIL(SDM_E_ARG, "bad argument: a column is missing");
  const size_t per_cell = 7 + 4 + 6, per_row = 5 + 6;
  double *cells = (double *)malloc(sizeof(double) * per_cell * (size_t)n_cell);
  double *rows = (double *)malloc(sizeof(double) * per_row * (size_t)n_sd);
  if (!cells || !rows) {
    free(cells);
    free(rows);
    FAIL(SDM_E_ARG, "out of memory");
  }
  double *eq[7], *kin[4], *henry[6], *conc[5], *df[6];
  for (int e = 0; e < 7; ++e) eq[e] = cells + (size_t)e * n_cell;
  for (int e = 0; e < 4; ++e) kin[e] = cells + (size_t)(7 + e) * n_cell;
  for (int g = 0; g < 6; ++g) henry[g] = cells + (size_t)(11 + g) * n_cell;
  for (int s = 0; s < 5; ++s) conc[s] = rows + (size_t)s * n_sd;
  for (int g = 0; g < 6; ++g) df[g] = rows + (size_t)(5 + g) * n_sd;
  /* acidity.py / concentration.py: the five species the pH depends on */
  const int conc_of[5] = {SDM_CHEM_AQ_N_MIII, SDM_CHEM_AQ_N_V, SDM_CHEM_AQ_C_IV, SDM_CHEM_AQ_S_IV,
                          SDM_CHEM_AQ_S_VI};
  double *gas_moles[6];
  for (int g = 0; g < 6; ++g) gas_moles[g] = moles[chem_aq_of_gas(g)];
  sdm_chemistry_cfg sub = *cfg;
  sub.timestep = cfg->timestep / cfg->n_substep;
  int rc = sdm_chem_recalculate_cell_data(ctx, n_cell, T, eq, kin, henry, consts);
  for (int s = 0; s < cfg->n_substep && rc == SDM_OK; ++s) {
    for (int half = 0; half < 2 && rc == SDM_OK; ++half) {
      int64_t failed = 0, negative = 0, exceeded = 0;
      for (int sp = 0; sp < 5; ++sp)
        for (int64_t i = 0; i < n_sd; ++i) conc[sp][i] = moles[conc_of[sp]][i] / volume[i];
      rc = sdm_equilibrate_H(ctx, cfg, n_sd, cell_id, (const double *const *)conc,
                             (const double *const *)eq, pH, do_chemistry_flag, &failed, consts);
      if (rc == SDM_OK)
        rc = sdm_chem_recalculate_drop_data(ctx, n_sd, pH, cell_id, (const double *const *)eq, df,
                                            consts);
      if (rc == SDM_OK && half == 0)
        rc = sdm_dissolution(ctx, &sub, n_sd, n_cell, idx, cell_start, do_chemistry_flag,
                             gas_moles, env_mixing_ratio, T, p, rhod,
                             (const double *const *)henry, (const double *const *)df, volume,
                             multiplicity, &negative, &exceeded, consts);
      if (rc == SDM_OK && half == 1)
        rc = sdm_oxidation(ctx, n_sd, cell_id, do_chemistry_flag, (const double *const *)kin,
                           (const double *const *)eq, sub.timestep, volume, pH,
                           df[SDM_CHEM_GAS_SO2], moles[SDM_CHEM_AQ_O3], moles[SDM_CHEM_AQ_H2O2],
                           moles[SDM_CHEM_AQ_S_IV], moles[SDM_CHEM_AQ_S_VI], consts);
      if (counts) {
        counts[0] += failed;
        counts[1] += negative;
        counts[2] += exceeded;
      }
    }
  }
  free(cells);
  free(rows);
  return rc;
}

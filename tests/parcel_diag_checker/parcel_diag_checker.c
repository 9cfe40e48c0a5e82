/*
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_parcel_diag.h.
 *
 * sdm_parcel_diagnose for host pointers is the evaluation the header writes out, in plain C and
 * in the header's summation shape (256 partials, rows t, t + 256, ... in ascending order, then
 * the strides 128 .. 1).  sdm_parcel_run_diag does not restate the time step: it calls
 * sdm_parcel_run of tests/parcel_checker/ ONE step at a time (nine run(1) equal run(9) bit for
 * bit, tests/test_parcel_checker.py), takes dv from the parcel's rhod before and after the step
 * and evaluates the table at the temperature after it.  The critical volume of the ratio filter
 * is the stage symbol sdm_critical_volume(_f) of the condensation checkers, which this library
 * links against as the parcel checker does.  The context is ignored.  Built by
 * __graft_entry__.build() next to this file (git-ignored); nothing in pysdm_amd/ loads it.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#pragma GCC visibility push(default)
#include "../../include/sdm_parcel_diag.h"
#pragma GCC visibility pop
#include "../../pysdm_amd/csrc/sdm_math.h"

#define API __attribute__((visibility("default")))
#define LANES 256

static __thread char g_err[256] = "";
#define FAIL(code, msg)                        \
  do {                                         \
    snprintf(g_err, sizeof(g_err), "%s", msg); \
    return (code);                             \
  } while (0)

API const char *sdm_last_error(void) { return g_err; }

static int check_requests(const sdm_parcel_requests *rq) {
  if (rq->n_moments < 0 || rq->n_moments > SDM_PARCEL_MAX_MOMENTS)
    FAIL(SDM_E_ARG, "parcel diagnostics: too many moment requests");
  if (rq->n_bins < 0 || rq->n_bins > SDM_PARCEL_MAX_BINS)
    FAIL(SDM_E_ARG, "parcel diagnostics: too many bins");
  for (int i = 0; i < rq->n_moments; ++i) {
    const sdm_parcel_moment_request *m = &rq->moment[i];
    if (m->attr < 0 || m->attr >= SDM_PARCEL_N_ATTRS || m->filter_attr < 0 ||
        m->filter_attr >= SDM_PARCEL_N_FILTERS)
      FAIL(SDM_E_ARG, "parcel diagnostics: unknown attribute");
    if (!(m->min_x <= m->max_x)) FAIL(SDM_E_ARG, "parcel diagnostics: min_x > max_x");
    if (m->rank != m->rank) FAIL(SDM_E_ARG, "parcel diagnostics: rank is NaN");
  }
  if (rq->n_bins > 0) {
    if (rq->bin_attr < 0 || rq->bin_attr >= SDM_PARCEL_N_FILTERS)
      FAIL(SDM_E_ARG, "parcel diagnostics: unknown bin attribute");
    for (int b = 0; b < rq->n_bins; ++b)
      if (!(rq->edges[b] < rq->edges[b + 1]))
        FAIL(SDM_E_ARG, "parcel diagnostics: edges do not strictly increase");
  }
  return SDM_OK;
}

static int check_starts(const int64_t *parcel_start, int64_t n_parcel, int64_t n_sd) {
  if (parcel_start[0] < 0 || parcel_start[n_parcel] > n_sd)
    FAIL(SDM_E_ARG, "parcel diagnostics: parcel_start outside the columns");
  for (int64_t c = 0; c < n_parcel; ++c)
    if (parcel_start[c + 1] <= parcel_start[c])
      FAIL(SDM_E_ARG, "parcel diagnostics: a parcel has no rows");
  return SDM_OK;
}

/* attributes' Radius: sign(v) |v * (1 / PI_4_3)| ** (1 / 3) */
static double radius_of_volume(double v, double inv_pi_4_3) {
  const double x = v * inv_pi_4_3;
  const double sg = (double)((x > 0) - (x < 0));
  return (x != x) ? x : sg * sdm_pow(fabs(x), 1.0 / 3.0);
}

static double power(double x, double rank) {
  return rank == 0 ? 1.0 : (rank == 1 ? x : sdm_pow(x, rank));
}

/* steps 2 and 3 of the header's SUM */
static double fold(double *partial) {
  for (int stride = LANES / 2; stride >= 1; stride /= 2)
    for (int t = 0; t < stride; ++t) partial[t] += partial[t + stride];
  return partial[0];
}

/* the table for rows row0 .. row0 + n at temperature T; out_* point at the parcel's row */
static int evaluate(sdm_ctx *ctx, const sdm_parcel_requests *rq, int64_t row0, int64_t n,
                    double T, const double *water_mass, const int64_t *multiplicity,
                    const double *vdry, const double *kappa, const double *f_org,
                    const double consts[34], const sdm_cond_formulae *formulae, double *out_m0,
                    double *out_m, double *out_spectrum) {
  const double rho_w = consts[SDM_COND_K_RHO_W], inv_pi_4_3 = 1 / consts[SDM_COND_K_PI_4_3];
  double *values = malloc((size_t)n * 7 * sizeof(double));
  int64_t *zeros = calloc((size_t)n, sizeof(int64_t));
  if (!values || !zeros) {
    free(values); free(zeros);
    FAIL(SDM_E_NOMEM, "parcel diagnostics: out of memory");
  }
  double *mass = values, *volume = values + n, *radius = values + 2 * n;
  double *dry_volume = values + 3 * n, *dry_radius = values + 4 * n, *ratio = values + 5 * n;
  double *v_cr = values + 6 * n;
  for (int64_t q = 0; q < n; ++q) {
    mass[q] = water_mass[row0 + q];
    volume[q] = mass[q] / rho_w;
    radius[q] = radius_of_volume(volume[q], inv_pi_4_3);
    dry_volume[q] = vdry[row0 + q];
    dry_radius[q] = radius_of_volume(dry_volume[q], inv_pi_4_3);
  }
  const double *forg = f_org ? f_org + row0 : NULL;
  const int rc = formulae ? sdm_critical_volume_f(ctx, v_cr, kappa + row0, forg, vdry + row0,
                                                  volume, &T, zeros, n, consts, formulae)
                          : sdm_critical_volume(ctx, v_cr, kappa + row0, forg, vdry + row0,
                                                volume, &T, zeros, n, consts);
  if (rc != SDM_OK) {
    free(values); free(zeros);
    FAIL(rc, "parcel diagnostics: sdm_critical_volume of the condensation checkers failed");
  }
  for (int64_t q = 0; q < n; ++q) ratio[q] = volume[q] / v_cr[q];
  const double *attrs[SDM_PARCEL_N_ATTRS] = {mass, volume, radius, dry_volume, dry_radius};
  const double *filters[SDM_PARCEL_N_FILTERS] = {mass, volume, dry_volume, ratio};

  for (int i = 0; i < rq->n_moments; ++i) {
    const sdm_parcel_moment_request *m = &rq->moment[i];
    const double *x = attrs[m->attr], *f = filters[m->filter_attr];
    double part_0[LANES], part_m[LANES];
    for (int t = 0; t < LANES; ++t) {
      part_0[t] = part_m[t] = 0.0;
      for (int64_t q = t; q < n; q += LANES)
        if (m->min_x <= f[q] && f[q] < m->max_x) {
          const double nn = (double)multiplicity[row0 + q];
          part_0[t] += nn;
          part_m[t] += nn * power(x[q], m->rank);
        }
    }
    const double m0 = fold(part_0), mk = fold(part_m);
    if (out_m0) out_m0[i] = m0;
    if (out_m) out_m[i] = m->skip_division_by_m0 ? mk : (m0 != 0 ? mk / m0 : 0.0);
  }
  if (rq->n_bins > 0 && out_spectrum) {
    const double *f = filters[rq->bin_attr];
    uint64_t bins[SDM_PARCEL_MAX_BINS] = {0};
    for (int64_t q = 0; q < n; ++q)
      for (int b = 0; b < rq->n_bins; ++b)
        if (rq->edges[b] <= f[q] && f[q] < rq->edges[b + 1]) {
          bins[b] += (uint64_t)multiplicity[row0 + q];
          break;
        }
    for (int b = 0; b < rq->n_bins; ++b) out_spectrum[b] = (double)bins[b];
  }
  free(values); free(zeros);
  return SDM_OK;
}

API int sdm_parcel_diagnose(sdm_ctx *ctx, int64_t n_parcel, int64_t n_sd,
                            const int64_t *parcel_start, const double *water_mass,
                            const int64_t *multiplicity, const double *vdry, const double *kappa,
                            const double *f_org, const double *T, const double consts[34],
                            const sdm_cond_formulae *formulae, const sdm_parcel_requests *rq,
                            const sdm_parcel_diag *diag) {
  if (!consts || !rq || !diag || n_parcel < 0 || n_sd < 0)
    FAIL(SDM_E_ARG, "sdm_parcel_diagnose: bad size or missing argument");
  int rc = check_requests(rq);
  if (rc != SDM_OK) return rc;
  if (n_parcel == 0) return SDM_OK;
  if (!parcel_start || !water_mass || !multiplicity || !vdry || !kappa || !T)
    FAIL(SDM_E_ARG, "sdm_parcel_diagnose: missing column");
  rc = check_starts(parcel_start, n_parcel, n_sd);
  if (rc != SDM_OK) return rc;
  const int64_t nm = rq->n_moments, nb = rq->n_bins;
  for (int64_t c = 0; c < n_parcel; ++c) {
    rc = evaluate(ctx, rq, parcel_start[c], parcel_start[c + 1] - parcel_start[c], T[c],
                  water_mass, multiplicity, vdry, kappa, f_org, consts, formulae,
                  diag->moment_0 ? diag->moment_0 + c * nm : NULL,
                  diag->moments ? diag->moments + c * nm : NULL,
                  diag->spectrum ? diag->spectrum + c * nb : NULL);
    if (rc != SDM_OK) return rc;
  }
  return SDM_OK;
}

API int sdm_parcel_run_diag(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, int64_t n_steps,
                            int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start,
                            double *water_mass, const int64_t *multiplicity, const double *vdry,
                            const double *kappa, const double *f_org, double *v_cr,
                            const sdm_parcel_state *st, const double *w_mid,
                            const sdm_parcel_profile *profile, const double consts[34],
                            const sdm_cond_formulae *formulae, const sdm_parcel_requests *rq,
                            const sdm_parcel_diag *diag) {
  const int with_diag =
      diag && (diag->moment_0 || diag->moments || diag->spectrum || diag->dv);
  if (rq) {
    const int rc = check_requests(rq);
    if (rc != SDM_OK) return rc;
  }
  if (with_diag && !rq) FAIL(SDM_E_ARG, "sdm_parcel_run_diag: outputs without requests");
  if (!with_diag || n_steps <= 0 || n_parcel <= 0) {
    const int rc = sdm_parcel_run(ctx, cfg, n_steps, n_parcel, n_sd, parcel_start, water_mass,
                                  multiplicity, vdry, kappa, f_org, v_cr, st, w_mid, profile,
                                  consts, formulae);
    if (rc != SDM_OK) FAIL(rc, "sdm_parcel_run_diag: sdm_parcel_run of the parcel checker failed");
    return SDM_OK;
  }
  if (!st || !st->rhod || !st->steps_done || !st->T || !st->mass_of_dry_air || !w_mid)
    FAIL(SDM_E_ARG, "sdm_parcel_run_diag: missing state");
  double *rhod_before = malloc((size_t)n_parcel * sizeof(double));
  int64_t *done_before = malloc((size_t)n_parcel * sizeof(int64_t));
  if (!rhod_before || !done_before) {
    free(rhod_before); free(done_before);
    FAIL(SDM_E_NOMEM, "sdm_parcel_run_diag: out of memory");
  }
  const int64_t nm = rq->n_moments, nb = rq->n_bins;
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
    rc = sdm_parcel_run(ctx, cfg, 1, n_parcel, n_sd, parcel_start, water_mass, multiplicity,
                        vdry, kappa, f_org, v_cr, st, w_mid + j * n_parcel,
                        profile ? &row : NULL, consts, formulae);
    if (rc != SDM_OK) {
      snprintf(g_err, sizeof(g_err), "sdm_parcel_run_diag: sdm_parcel_run failed (%d)", rc);
      break;
    }
    for (int64_t c = 0; c < n_parcel && rc == SDM_OK; ++c) {
      if (st->steps_done[c] == done_before[c]) continue; /* failed: its rows stay untouched */
      const int64_t at = j * n_parcel + c;
      if (diag->dv) diag->dv[at] = st->mass_of_dry_air[c] / ((st->rhod[c] + rhod_before[c]) / 2);
      rc = evaluate(ctx, rq, parcel_start[c], parcel_start[c + 1] - parcel_start[c], st->T[c],
                    water_mass, multiplicity, vdry, kappa, f_org, consts, formulae,
                    diag->moment_0 ? diag->moment_0 + at * nm : NULL,
                    diag->moments ? diag->moments + at * nm : NULL,
                    diag->spectrum ? diag->spectrum + at * nb : NULL);
    }
  }
  free(rhod_before); free(done_before);
  return rc;
}

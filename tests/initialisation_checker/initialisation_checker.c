/*
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_initialisation.h.
 *
 * A serial, strict-IEEE restatement of the reference's PySDM/initialisation/
 * equilibrate_wet_radii.py:43-122 ("ewr.py" below), statement for statement.  The formulae are the
 * option switches of pysdm_amd/csrc/condensation_formulae.h, the search is pysdm_amd/csrc/toms748.h
 * and the transcendental functions are csrc/sdm_math.h, all of which the product compiles too: both
 * sides get the same bits.  Host pointers; the context is ignored.  Built by
 * __graft_entry__.build() next to this file (git-ignored); nothing in pysdm_amd/ loads it.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/sdm_initialisation.h"
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

/* ewr.py:48-50 */
typedef struct {
  const cf_k *k;
  double T, RH, kp, rd3, f_org;
  int *fail; /* CompressedFilmRuehl used up its iterations (the reference's assert) */
} MinArgs;

static double minfun(double r, const MinArgs *a) {
  const cf_k *k = a->k;
  const double sgm = cf_sigma(k, a->T, cf_volume(k, r), CF_C(PI_4_3) * a->rd3, a->f_org, a->fail);
  return a->RH - cf_RH_eq(k, r, a->T, a->kp, a->rd3, sgm);
}
#undef TOMS748_ARGS
#undef TOMS748_EVAL
#define TOMS748_ARGS MinArgs
#define TOMS748_EVAL(x, args) minfun((x), (args))
#define TOMS748_NAME(name) name##_minfun
#include "../../pysdm_amd/csrc/toms748.h"

API int sdm_equilibrate_wet_radii(sdm_ctx *ctx, int64_t n, const double *r_dry,
                                  const double *kappa_times_dry_volume, const double *f_org,
                                  const int64_t *cell_id, const double *T, const double *RH,
                                  int64_t n_cell, double rtol, int max_iters,
                                  const double consts[34], const sdm_cond_formulae *formulae,
                                  double *r_wet, int64_t *iters, int64_t *status) {
  static const int n_choices[SDM_COND_N_OPTS] = CF_N_CHOICES;
  (void)ctx;
  if (n < 0 || n_cell < 1 || max_iters < 1 || !consts) FAIL(SDM_E_ARG, "bad argument");
  cf_k kk;
  const cf_k *k = &kk;
  memset(&kk, 0, sizeof(kk));
  for (int i = 0; i < SDM_COND_N_CONSTS; ++i) kk.c[i] = consts[i];
  if (formulae) {
    for (int i = 0; i < SDM_COND_N_OPTS; ++i) {
      if (formulae->option[i] < 0 || formulae->option[i] >= n_choices[i])
        FAIL(SDM_E_ARG, "bad argument: an option code the descriptor does not define");
      kk.o[i] = formulae->option[i];
    }
    for (int i = 0; i < SDM_COND_F_N_CONSTS; ++i) kk.f[i] = formulae->consts[i];
  }
  const int film = CF_O(SURFACE_TENSION) != SDM_COND_SGM_CONSTANT;
  if (n == 0) return SDM_OK;
  if (!r_dry || !kappa_times_dry_volume || !T || !RH || !r_wet || !iters || !status)
    FAIL(SDM_E_ARG, "bad argument: null pointer");
  if (film && !f_org) FAIL(SDM_E_ARG, "bad argument: f_org is NULL with a film");
  int64_t n_failed = 0, n_max = 0, n_sigma = 0, first = n;
  for (int64_t i = 0; i < n; ++i) { /* ewr.py:64 */
    const int64_t cid = cell_id ? cell_id[i] : 0;
    int it = 0, fail = 0;
    double rw;
    if (cid < 0 || cid >= n_cell) {
      rw = sdm_nan();
      it = -1;
    } else {
      const double kappa = kappa_times_dry_volume[i] / cf_volume(k, r_dry[i]); /* :43 */
      const double rd3 = sdm_pow(r_dry[i], 3.0);
      const double a = r_dry[i];                                  /* :68 */
      const double b = cf_r_cr(k, kappa, rd3, T[cid], CF_C(SGM_W)); /* :69 */
      if (!(a < b)) {                                             /* :71-74 */
        rw = r_dry[i];
      } else {
        MinArgs args = {k, T[cid], cf_np_max(0.0, cf_np_min(1.0, RH[cid])), kappa, rd3,
                        (film && f_org) ? f_org[i] : 0.0, &fail}; /* :77-83 */
        const double fa = minfun(a, &args);
        if (fa < 0) {                                             /* :86-89 */
          rw = r_dry[i];
        } else {
          const double fb = minfun(b, &args);
          rw = toms748_solve_minfun(&args, a, b, fa, fb, rtol, max_iters, &it); /* :92-102 */
        }
      }
    }
    r_wet[i] = rw;
    iters[i] = it;
    n_failed += it == -1;
    n_max += it == max_iters;
    n_sigma += fail;
    if ((it == -1 || it == max_iters) && i < first) first = i;
  }
  status[SDM_INIT_STATUS_FAILED] = n_failed;
  status[SDM_INIT_STATUS_MAX_ITERS] = n_max;
  status[SDM_INIT_STATUS_FIRST] = first;
  status[SDM_INIT_STATUS_SIGMA_FAILED] = n_sigma;
  return SDM_OK;
}

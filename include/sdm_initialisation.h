/*
 * sdm_initialisation.h -- C ABI of the initialisation path of libsdm_hip.so: the step before the
 * first time step that has a hot loop, PySDM/initialisation/equilibrate_wet_radii.py (the wet
 * radius at which a dry aerosol particle is in Koehler equilibrium with the air of its cell), one
 * TOMS748 root search per super-droplet.
 *
 * Same conventions as sdm_hip.h (whose context, error codes and sdm_last_error() it uses): a
 * context first, DEVICE pointers owned by the caller, 0 = ok, negative = SDM_E_*; work is enqueued
 * on the context's stream.  The formulae are those of include/sdm_condensation_formulae.h: `consts`
 * (SDM_COND_K_*) and an options descriptor, of which only surface_tension and hygroscopicity are
 * read.  A separate header so that implementations of the other headers need not implement it.
 *
 * The contract, row i of n (equilibrate_wet_radii.py:43-122, every operation rounded once, pow /
 * exp / log being those of sdm_math.h):
 *     kappa = kappa_times_dry_volume[i] / (PI_4_3 * pow(r_dry[i], 3))
 *     c     = cell_id ? cell_id[i] : 0          (outside [0, n_cell): r_wet = NaN, iters = -1)
 *     rd3   = pow(r_dry[i], 3)
 *     a     = r_dry[i];  b = r_cr(kappa, rd3, T[c], sgm_w)     (the constant sgm_w, not the film's)
 *     not a < b                          ->  r_wet = r_dry, iters = 0
 *     RH    = max(0, min(1, RH[c]))
 *     minfun(r) = RH - RH_eq(r, T[c], kappa, rd3, sigma(T[c], volume(r), PI_4_3 * rd3, f_org[i]))
 *     minfun(a) < 0                      ->  r_wet = r_dry, iters = 0
 *     otherwise  (r_wet, iters) = toms748_solve(minfun, a, b, rtol, max_iters) with
 *                trivia.within_tolerance; (NaN, -1) where the bracket holds no sign change
 */
#ifndef SDM_INITIALISATION_H
#define SDM_INITIALISATION_H
#include "sdm_condensation_formulae.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows of one pass of the kernel's capped grid (more rows: a grid-stride loop) */
#define SDM_INIT_ROWS_PER_PASS 262144

/* words of `status` */
#define SDM_INIT_STATUS_FAILED 0      /* rows with iters == -1 (cell_id out of range included) */
#define SDM_INIT_STATUS_MAX_ITERS 1   /* rows with iters == max_iters */
#define SDM_INIT_STATUS_FIRST 2       /* the smallest index among those rows; n if there is none */
#define SDM_INIT_STATUS_SIGMA_FAILED 3 /* rows on which CompressedFilmRuehl's inner search used up
                                          its iterations (the reference's assert) */
#define SDM_INIT_STATUS_WORDS 4

/* One `equilibrate_wet_radii`.  Enqueues only.  r_dry, kappa_times_dry_volume, r_wet: n doubles;
 * iters: n int64; f_org: n doubles, NULL = zeros (refused unless the surface tension is Constant);
 * cell_id: n int64, NULL = cell 0; T, RH: n_cell doubles; `formulae`: a HOST struct read before the
 * call returns, NULL = PySDM's defaults; `status`: int64[SDM_INIT_STATUS_WORDS] on the device,
 * written by the call, read by the caller when it next synchronises.  Nothing traps: a failed row
 * is counted in `status`.  n == 0 returns before any launch (status is not written).
 * SDM_E_ARG: a null pointer, n < 0, n_cell < 1, max_iters < 1, an option code the descriptor does
 * not define, f_org == NULL with a film.                                                        */
int sdm_equilibrate_wet_radii(sdm_ctx *ctx, int64_t n, const double *r_dry,
                              const double *kappa_times_dry_volume, const double *f_org,
                              const int64_t *cell_id, const double *T, const double *RH,
                              int64_t n_cell, double rtol, int max_iters, const double consts[34],
                              const sdm_cond_formulae *formulae, double *r_wet, int64_t *iters,
                              int64_t *status);

#ifdef __cplusplus
}
#endif
#endif

/*
 * sdm_parcel_diag.h -- C ABI of the parcel's diagnostics in libsdm_hip.so: statistical moments and
 * one size spectrum of every parcel's droplet population, evaluated inside the time-step loop of
 * include/sdm_parcel.h (sdm_parcel_run_diag) or on given columns (sdm_parcel_diagnose).  They are
 * what PySDM's products read: `moments` and the `moment_0` of `spectrum_moments`
 * (backends/impl_numba/methods/moments_methods.py:14-99, :101-182) for a one-cell domain with
 * weighting_rank = 0.
 *
 * Same conventions as sdm_parcel.h, which it extends.  A header of its own, as every path has, so
 * that an implementation of sdm_parcel.h need not implement it (the bindings demand every symbol
 * a header declares).
 *
 * One evaluation of a request table for one parcel of n rows (row q: multiplicity n_q, water mass
 * m_q, dry volume, kappa, f_org) at temperature T, in plain IEEE doubles without contraction, the
 * transcendentals those of the library (csrc/sdm_math.h):
 *
 *   volume      = m / rho_w
 *   radius      = sign(volume) * sdm_pow(|volume * (1 / PI_4_3)|, 1 / 3)    (attributes' Radius)
 *   dry radius  = the same of the dry volume
 *   ratio       = volume / sdm_critical_volume(_f)(kappa, f_org, dry volume, volume, T)
 *   power(x, r) = 1 if r == 0, x if r == 1, sdm_pow(x, r) otherwise
 *
 *   moment request i (attr, rank, filter_attr, min_x, max_x, skip_division_by_m0):
 *     selected_q  = min_x <= filter_attr_q < max_x                       (half-open)
 *     moment_0[i] = SUM over selected rows of (double)n_q                (exact below 2^53)
 *     moments[i]  = SUM over selected rows of (double)n_q * power(attr_q, rank)
 *     unless skip_division_by_m0: moments[i] = moment_0[i] != 0 ? moments[i] / moment_0[i] : 0
 *   the spectrum request (bin_attr, n_bins, edges):
 *     spectrum[k] = (double) of the 64-bit integer sum of n_q over the rows with
 *                   edges[k] <= bin_attr_q < edges[k + 1]                (exact, order-free)
 *
 * SUM has a fixed shape, which every implementation follows add for add (the reference's own
 * order is undefined: atomics under prange).  With partial[0 .. 255] = +0.0:
 *   1. for t = 0 .. 255: partial[t] += term of row q, for q = t, t + 256, t + 512, ... ascending
 *      (rows that are not selected add nothing);
 *   2. for stride = 128, 64, 32, 16, 8, 4, 2, 1: partial[t] += partial[t + stride] for t < stride;
 *   3. SUM = partial[0].
 *
 * The temperature of the ratio's critical volume.  sdm_parcel_run_diag evaluates the table after
 * a step with the parcel's temperature AFTER that step, which is what the reference's
 * `CriticalVolume.recalculate` reads from environment["T"] when a product asks at output time
 * (the recorded products of tests/golden/parcel_products.npz pin this).  It is not the `v_cr`
 * column of the call: that one holds the value the step itself used, at the temperature before.
 */
#ifndef SDM_PARCEL_DIAG_H
#define SDM_PARCEL_DIAG_H
#include "sdm_parcel.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDM_PARCEL_MAX_MOMENTS 16
#define SDM_PARCEL_MAX_BINS 256

/* `attr` of a moment request */
#define SDM_PARCEL_ATTR_WATER_MASS 0
#define SDM_PARCEL_ATTR_VOLUME 1
#define SDM_PARCEL_ATTR_RADIUS 2
#define SDM_PARCEL_ATTR_DRY_VOLUME 3
#define SDM_PARCEL_ATTR_DRY_RADIUS 4
#define SDM_PARCEL_N_ATTRS 5
/* `filter_attr` of a moment request and `bin_attr` of the spectrum.  Water mass is PySDM's
 * "signed water mass" too: the two are the same thing under liquid spheres. */
#define SDM_PARCEL_FILTER_WATER_MASS 0
#define SDM_PARCEL_FILTER_VOLUME 1
#define SDM_PARCEL_FILTER_DRY_VOLUME 2
#define SDM_PARCEL_FILTER_VOLUME_RATIO 3 /* "wet to critical volume ratio" */
#define SDM_PARCEL_N_FILTERS 4

typedef struct sdm_parcel_moment_request {
  int32_t attr, filter_attr;
  double rank, min_x, max_x;
  int32_t skip_division_by_m0, reserved;
} sdm_parcel_moment_request;

/* a HOST struct, read before the call returns */
typedef struct sdm_parcel_requests {
  int32_t n_moments; /* 0 .. SDM_PARCEL_MAX_MOMENTS */
  int32_t n_bins;    /* 0 (no spectrum) .. SDM_PARCEL_MAX_BINS */
  int32_t bin_attr;  /* SDM_PARCEL_FILTER_* */
  int32_t reserved;
  sdm_parcel_moment_request moment[SDM_PARCEL_MAX_MOMENTS];
  double edges[SDM_PARCEL_MAX_BINS + 1]; /* n_bins + 1 of them, strictly increasing */
} sdm_parcel_requests;

/* the outputs: DEVICE arrays, step-major, row (k * n_parcel + c) of step k of the call and parcel
 * c; within a row moment_0 / moments hold n_moments entries and spectrum n_bins.  dv holds one
 * entry per row: the step's dv = mass_of_dry_air / ((prhod + rhod) / 2), which is `mesh.dv` at
 * output time and what the concentration products divide by.  Any member may be NULL.  Rows of
 * steps a parcel did not carry out (after a failure) are left untouched, as in the profile. */
typedef struct sdm_parcel_diag {
  double *moment_0, *moments, *spectrum, *dv;
} sdm_parcel_diag;

/* sdm_parcel_run with the request table evaluated after every step (kernels of their own; with
 * `requests` NULL or empty and `diag` NULL or empty it is sdm_parcel_run itself, on its kernels).
 *
 * SDM_E_ARG, beyond sdm_parcel_run's: more than SDM_PARCEL_MAX_MOMENTS moment requests or
 * SDM_PARCEL_MAX_BINS bins, an unknown attr / filter_attr / bin_attr, edges that do not strictly
 * increase (a NaN among them included), min_x > max_x (or a NaN bound), a rank that is NaN. */
int sdm_parcel_run_diag(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, int64_t n_steps,
                        int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start,
                        double *water_mass, const int64_t *multiplicity, const double *vdry,
                        const double *kappa, const double *f_org, double *v_cr,
                        const sdm_parcel_state *state, const double *w_mid,
                        const sdm_parcel_profile *profile, const double consts[34],
                        const sdm_cond_formulae *formulae, const sdm_parcel_requests *requests,
                        const sdm_parcel_diag *diag);

/* the stage symbol: the request table on given columns, one row of moment_0 / moments / spectrum
 * per parcel (`diag->dv` is not written).  `T` holds one temperature per parcel.  It gives the
 * products of an initial state, and is the yardstick of the fused rows: sdm_parcel_run_diag's row
 * of a step equals what this writes for the columns and the temperature after that step, bit for
 * bit.  `formulae` as in sdm_parcel_run (the ventilation is not read). */
int sdm_parcel_diagnose(sdm_ctx *ctx, int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start,
                        const double *water_mass, const int64_t *multiplicity, const double *vdry,
                        const double *kappa, const double *f_org, const double *T,
                        const double consts[34], const sdm_cond_formulae *formulae,
                        const sdm_parcel_requests *requests, const sdm_parcel_diag *diag);

#ifdef __cplusplus
}
#endif
#endif

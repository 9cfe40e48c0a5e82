/*
 * sdm_parcel.h -- C ABI of the adiabatic-parcel path of libsdm_hip.so: whole ascents of an
 * ensemble of independent parcels (PySDM's `Parcel` environment with the dynamics
 * `AmbientThermodynamics` and `Condensation`; environments/parcel.py:101-153,
 * environments/impl/moist.py:73-100, dynamics/condensation.py:95-131) in one call.
 *
 * Same conventions as sdm_condensation.h (whose constants, and sdm_condensation_formulae.h whose
 * descriptor, it uses): a context first, DEVICE pointers owned by the caller (int64 / double), 0 =
 * ok, negative = SDM_E_*; the function only enqueues work on the context's stream (it reads
 * `parcel_start` back once to check it, before anything is launched).  A header of its own so
 * that implementations of the other headers need not implement it.
 *
 * One time step of one parcel, in plain IEEE doubles, left to right, without contraction
 * (hydrostatics ConstantGVapourMixingRatioAndThetaStd; `w` is the step's entry of `w_mid`):
 *
 *   delta   = qv_prev - qv
 *   qv_mid  = qv - delta / 2
 *   lv      = <latent heat of vapourisation of the formulae>(T)
 *   Rq      = Rv / (1 / qv_mid + 1) + Rd / (1 + qv_mid)
 *   cp      = c_pv / (1 / qv_mid + 1) + c_pd / (1 + qv_mid)
 *   rho     = p / Rq / T
 *   dql_dz  = delta / w / dt
 *   drho_dz = (g_std / T * rho * (Rq / cp - 1) - p * lv / cp / (T * T) * dql_dz) / Rq
 *   z      += dt * w
 *   prhod   = rhod + dt * (w * drho_dz)
 *   dv      = mass_of_dry_air / ((prhod + rhod) / 2)
 *   v_cr[row] = sdm_critical_volume(_f) at T, of the row's water_mass / rho_w, vdry, kappa, f_org
 *   (pthd, pqv, water masses, counters, RH_max, success) = the solver of sdm_condensation(_f) for
 *           thd, qv, rhod, prhod, pthd = thd, pqv = qv, dv, n_substeps read as the previous count
 *   if not success: failed_step = steps_done, and the parcel stops with its state (water masses
 *           included; v_cr excepted) as before the step
 *   qv_prev = qv;  rhod, thd, qv = prhod, pthd, pqv;  T, p, RH = sdm_temperature_pressure_rh(_f)
 *   if adaptive: n_substeps = min(max(n_substeps, n_clamp_lo), n_clamp_hi)
 *   steps_done += 1; the profile row is written
 */
#ifndef SDM_PARCEL_H
#define SDM_PARCEL_H
#include "sdm_condensation_formulae.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a HOST struct, read before the call returns */
typedef struct sdm_parcel_cfg {
  double dt;    /* the time step */
  double g_std; /* constants' g_std */
  /* the solver's parameters, as sdm_condensation takes them */
  double rtol_x, rtol_thd, dt_min, dt_max, RH_rtol;
  int32_t adaptive, fuse, multiplier, max_iters;
  /* dynamics/condensation.py:122-131: int(dt / dt_cond_range[1]), int(dt / dt_cond_range[0]) */
  int64_t n_clamp_lo, n_clamp_hi;
  /* time steps per kernel launch; 0: the library's default */
  int32_t steps_per_launch;
  int32_t reserved;
} sdm_parcel_cfg;

/* the parcels' state: DEVICE arrays of n_parcel (the struct itself is a host struct) */
typedef struct sdm_parcel_state {
  double *z, *rhod, *thd, *qv, *T, *p, *RH; /* the current values */
  double *qv_prev;         /* qv before the last step (== qv before the first step) */
  double *mass_of_dry_air; /* read only */
  int64_t *n_substeps, *n_activating, *n_deactivating, *n_ripening;
  double *RH_max;
  int64_t *steps_done;  /* time steps carried out so far */
  int64_t *failed_step; /* -1, or the value of steps_done at the step whose solver failed */
} sdm_parcel_state;

/* optional record: DEVICE arrays of n_steps x n_parcel, step-major; row k holds the state after
 * step k of the call.  Any member may be NULL.  Entries of steps a parcel did not carry out
 * (after a failure) are left untouched. */
typedef struct sdm_parcel_profile {
  double *z, *rhod, *thd, *qv, *T, *p, *RH, *RH_max;
  int64_t *n_substeps, *n_activating, *n_deactivating, *n_ripening;
} sdm_parcel_profile;

/* `n_steps` further time steps of each of `n_parcel` parcels.  Parcel c owns rows
 * parcel_start[c] .. parcel_start[c + 1] of the per-droplet columns (length n_sd): water_mass
 * (in/out), multiplicity, vdry, kappa, f_org (read by every surface tension but Constant; may be
 * NULL otherwise) and v_cr (an output: the critical volume used in the last step).  The sums over
 * a parcel's droplets are formed in row order.  `w_mid` holds n_steps x n_parcel updraft
 * velocities, step-major: w((k + 1/2) dt) of step k of this call.  `formulae` NULL: PySDM's
 * default formulae and their kernel; otherwise the general kernel with that descriptor.
 *
 * A parcel whose solver fails keeps its state, records the step in failed_step and is skipped for
 * the rest of this call and in later calls; the other parcels go on; nothing traps.  A second call
 * continues where the first stopped: all state is in the arrays.  The call enqueues
 * ceil(n_steps / steps_per_launch) launches without synchronising between them.
 *
 * SDM_E_ARG: a parcel without rows (parcel_start not strictly increasing within [0, n_sd]), a
 * ventilation other than Neglect, dt_min == 0.                                                 */
int sdm_parcel_run(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, int64_t n_steps, int64_t n_parcel,
                   int64_t n_sd, const int64_t *parcel_start, double *water_mass,
                   const int64_t *multiplicity, const double *vdry, const double *kappa,
                   const double *f_org, double *v_cr, const sdm_parcel_state *state,
                   const double *w_mid, const sdm_parcel_profile *profile,
                   const double consts[34], const sdm_cond_formulae *formulae);

/* the `steps_per_launch` a cfg with 0 gets */
#define SDM_PARCEL_STEPS_PER_LAUNCH 16

/* The same call with statistical moments and a size spectrum of every parcel's droplets evaluated
 * after every step, inside the same loop: sdm_parcel_run_diag of sdm_parcel_diag.h (a header of
 * its own, so that an implementation of this one need not implement it). */

#ifdef __cplusplus
}
#endif
#endif

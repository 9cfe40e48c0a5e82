/*
 * sdm_parcel_ice.h -- C ABI of the mixed-phase parcel in libsdm_hip.so: the adiabatic parcel of
 * include/sdm_parcel.h whose super-droplets may be ice (PySDM's `Parcel(mixed_phase=True)` with the
 * dynamics `AmbientThermodynamics`, `Condensation`, then `Freezing` and / or
 * `VapourDepositionOnIce` in either order; environments/parcel.py:101-153,
 * environments/impl/moist.py:73-100, particulator.py:501-568, dynamics/freezing.py:62-87,
 * dynamics/vapour_deposition_on_ice.py).
 *
 * Same conventions as sdm_parcel.h, which it extends, sdm_freezing.h and sdm_deposition.h, whose
 * constants, codes and row arithmetic it uses.  A header of its own, as every path has, so that an
 * implementation of sdm_parcel.h need not implement it.  The per-droplet mass column is PySDM's
 * "signed water mass": > 0 liquid, < 0 ice.
 *
 * What the ice passes read.  `a_w_ice` and `RH_ice` are the environment's CURRENT values, which
 * the reference computes in `Moist.sync` - after the advance of rhod and BEFORE the condensation of
 * a step - and does not refresh when `update_TpRH` overwrites T, p and RH after the condensation
 * (it writes these three only).  `Particulator.deposition` and `immersion_freezing_*` /
 * `homogeneous_freezing_*` pass the environment's current T, p, RH, a_w_ice, RH_ice, qv, rhod and
 * thd (particulator.py:501-568), and the parcel's current values are those of the START of the step
 * until `Parcel.__call__` ... `post_register`'s swap at the end of it.  So both passes of step k
 * see the state of before step k, with the pair (a_w_ice, RH_ice) formed in step k - 1 from that
 * step's advanced rhod and the thd and qv of before its condensation; before the first step the
 * pair is that of the initial state.  Each parcel carries the pair from step to step, from launch
 * to launch and from call to call, like the air pair of sdm_parcel_vent.h.
 *
 * One time step of one parcel, in plain IEEE doubles, left to right, without contraction; what is
 * not written out is the step of sdm_parcel.h (whose names these are).  `current` = the state at
 * the start of the step; n_rows = the parcel's rows; position q = row parcel_start[c] + q.
 *
 *   1 delta .. dv, z  = the advance of sdm_parcel.h (parcel.py:101-134)
 *   2 (sync_T, sync_p, sync_RH) = sdm_temperature_pressure_rh(_f)(prhod, thd, qv)
 *     (a_w_ice_new, RH_ice_new) = sdm_a_w_ice(sync_T, sync_p, sync_RH, qv)     (moist.py:73-100)
 *   3 v_cr[row] as in sdm_parcel.h for the rows with m > 0 at the start of the step; a row with
 *     m <= 0 keeps the v_cr it had
 *   4 the solver of sdm_condensation(_f) as in sdm_parcel.h: it leaves rows with m <= 0 alone
 *     (condensation_methods.py:364, 432).  (pthd, pqv) are its outputs and
 *     (nT, np, nRH) = sdm_temperature_pressure_rh(_f)(prhod, pthd, pqv).
 *     If not success: failed_step = steps_done and the parcel stops with its state as before the
 *     step - water masses, the pair, rng_offset, n_exceeded and the optional columns included; no
 *     ice pass runs
 *   5 the ice passes that are switched on, in the order `order` names.  Both read the CURRENT
 *     T, p, RH, a_w_ice, RH_ice, qv, rhod, thd:
 *     freezing: sdm_freezing_step (sdm_freezing.h:110-123) with n_sd = n_rows, n_cell = 1,
 *       cell_id = 0, volume = NULL, timestep = dt, the parcel's own PCG64 stream
 *       rng_state_inc[4 c .. 4 c + 4) and rng_offset[c]: the row at position q takes uniform number
 *       rng_offset[c] + q in the time-dependent immersion pass, and in the homogeneous pass
 *       rng_offset[c] + n_rows + q if that immersion pass ran, else rng_offset[c] + q.  Then
 *       rng_offset[c] += n_rows per stochastic pass that is switched on, whether or not anything
 *       froze.  Thaw and temperature_of_last_freezing as there.
 *     deposition: sdm_deposition (sdm_deposition.h:86-105) with n_sd = n_rows, n_cell = 1,
 *       cell_id = 0, time_step = dt, cell_volume = dv, predicted pair (pqv, pthd) in / out.
 *       Rows with -delta > qv are ADDED to n_exceeded[c]; nothing traps.
 *   6 qv_prev = qv;  rhod, thd, qv = prhod, pthd, pqv (the deposition's additions included);
 *     T, p, RH = nT, np, nRH - NOT recomputed after the deposition: the reference leaves T, p and
 *     RH stale there (particulator.py:523, its TODO #1524), and so does this path;
 *     a_w_ice, RH_ice = a_w_ice_new, RH_ice_new;  counters and clamps as in sdm_parcel.h
 *   7 the ice profile row: a_w_ice, RH_ice (the new pair); n_ice = the int64 sum of multiplicity
 *     over the rows with m < 0 after the step (exact); ice_mass = the SUM of sdm_parcel_diag.h of
 *     multiplicity * (-m) over those rows (a row that is not ice adds +0.0); n_exceeded = the
 *     step's count; dv
 */
#ifndef SDM_PARCEL_ICE_H
#define SDM_PARCEL_ICE_H
#include "sdm_deposition.h"
#include "sdm_freezing.h"
#include "sdm_parcel.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDM_PARCEL_ICE_FREEZING_FIRST 0
#define SDM_PARCEL_ICE_DEPOSITION_FIRST 1

/* a HOST struct, read before the call returns */
typedef struct sdm_parcel_ice_cfg {
  int32_t freezing, deposition; /* the two passes: 0 off, otherwise on */
  int32_t order;                /* SDM_PARCEL_ICE_* */
  /* Freezing(...)'s keywords and the rate codes, as in sdm_freezing_cfg */
  int32_t singular, immersion_freezing, homogeneous_freezing, thaw;
  int32_t j_het, j_hom; /* SDM_FRZ_JHET_* / SDM_FRZ_JHOM_* */
  /* as in sdm_deposition_cfg: SDM_DEP_COORD_* / _CAPACITY_* / _KINETICS_* / _SUM_* */
  int32_t coordinate, capacity, kinetics, sum;
  int32_t reserved; /* 0 */
} sdm_parcel_ice_cfg;

/* DEVICE arrays (the struct itself is a host struct) */
typedef struct sdm_parcel_ice_state {
  double *a_w_ice, *RH_ice;      /* the carried pair: n_parcel, in / out */
  uint64_t *rng_offset;          /* n_parcel, in / out: uniforms drawn so far */
  const uint64_t *rng_state_inc; /* 4 x n_parcel: NumPy PCG64 {state_hi, state_lo, inc_hi, inc_lo} */
  int64_t *n_exceeded;           /* n_parcel, added to */
  /* per-row columns of n_sd; NULL where the configuration does not read them */
  const double *freezing_temperature, *immersed_surface_area;
  double *temperature_of_last_freezing; /* optional, in / out */
} sdm_parcel_ice_state;

/* optional record: DEVICE arrays of n_steps x n_parcel, step-major, as sdm_parcel_profile.  Any
 * member may be NULL; entries of steps a parcel did not carry out are left untouched. */
typedef struct sdm_parcel_ice_profile {
  double *a_w_ice, *RH_ice;
  int64_t *n_ice;
  double *ice_mass;
  int64_t *n_exceeded;
  double *dv;
} sdm_parcel_ice_profile;

/* sdm_parcel_run with the ice passes inside the same loop: one launch per steps_per_launch time
 * steps, no host round trip.  Everything is in the arrays, so a second call continues where the
 * first stopped, stream positions included.  `ice_profile` may be NULL.
 *
 * SDM_E_ARG, beyond sdm_parcel_run's: `ice_cfg` or `ice_state` NULL, both passes off (that is
 * sdm_parcel_run), an unknown order or code, a NULL a_w_ice, RH_ice or n_exceeded, a stochastic
 * pass without rng_offset / rng_state_inc, singular immersion freezing without
 * freezing_temperature, time-dependent immersion freezing without immersed_surface_area,
 * frz_consts NULL (the pair of point 2 reads them whichever pass is on), dep_consts NULL with the
 * deposition on. */
int sdm_parcel_run_ice(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, const sdm_parcel_ice_cfg *ice_cfg,
                       int64_t n_steps, int64_t n_parcel, int64_t n_sd,
                       const int64_t *parcel_start, double *signed_water_mass,
                       const int64_t *multiplicity, const double *vdry, const double *kappa,
                       const double *f_org, double *v_cr, const sdm_parcel_state *state,
                       const double *w_mid, const sdm_parcel_profile *profile,
                       const double consts[34], const sdm_cond_formulae *formulae,
                       const sdm_parcel_ice_state *ice_state,
                       const sdm_parcel_ice_profile *ice_profile, const double frz_consts[33],
                       const double dep_consts[39]);

#ifdef __cplusplus
}
#endif
#endif

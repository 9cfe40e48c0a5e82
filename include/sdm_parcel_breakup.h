/*
 * sdm_parcel_breakup.h -- C ABI of the adiabatic parcel with collisional breakup in libsdm_hip.so:
 * whole ascents of an ensemble of independent parcels under PySDM's dynamics
 * `AmbientThermodynamics`, `Condensation`, then `Collision` or `Breakup` (or `Coalescence`),
 * registered in that order, in one call.  A colliding pair bounces, coalesces or breaks up
 * (collision.py:174-234, collisions_methods.py:247-311): all eight fragmentation functions, the four
 * coalescence efficiencies, the limiters, `handle_all_breakups` and the overflow count of
 * sdm_collision_step (sdm_hip.h) are served.
 *
 * Same conventions as sdm_parcel_coal.h, whose structs, constants and definitions it uses.  A
 * header of its own, as every path has: sdm_parcel_run_coal goes on refusing enable_breakup, and
 * an implementation of that header need not implement this one.
 *
 * One time step of one parcel c (rows parcel_start[c] .. parcel_start[c + 1], N of them):
 *
 *   1. as point 1 of sdm_parcel_coal.h.
 *   2. the collision step: one `Collision.__call__` with coal_cfg->enable_breakup AS GIVEN on the
 *      parcel as ONE cell.  Bit for bit what sdm_collision_step (sdm_hip.h) gives for
 *        n_cell = 1, n_sd = N, the local croupier, no optimized_random;
 *        idx, ctl, cell_start, multiplicity and cfg.dt, cfg.dv as in point 2 of sdm_parcel_coal.h;
 *        attributes = three rows of N: water mass (mass_attr = 0), dry volume, kappa times dry
 *          volume - a breakup redistributes all three (collisions_methods.py:96-132);
 *        cfg.max_multiplicity = coal_cfg->max_multiplicity (the set-up's);
 *        cfg.rng_state_inc = rng_state_inc[4 c .. 4 c + 4), state.rng_offset = rng_offset[c]
 *          (advanced by N + N / 2 per sub-step) and, with enable_breakup,
 *          state.rng_offset_breakup = rng_offset_breakup[c]: the breakup stream is the parcel's own
 *          generator (same state and increment) at that position, advanced as
 *          sdm_step_result.rng_offset_breakup says: by N / 2 per sub-step.  ONE draw per pair slot
 *          serves the efficiency decision and the fragmentation (the reference's proc_rand and
 *          rand_frag generators share seed and position).
 *      Of coal_cfg these are read beyond what sdm_parcel_run_coal reads: enable_breakup,
 *      handle_all_breakups, ec, frag, ec_param, eb_const, frag_param, frag_vmin, frag_nfmax, rho_w,
 *      sgm_w, straub_consts, berry_params, berry_unit, max_multiplicity.
 *      Sub-steps, the compaction and the parcel of ONE row: as in sdm_parcel_coal.h.
 *   3. as point 3 of sdm_parcel_coal.h.
 *   4. as point 4 of sdm_parcel_coal.h, and with enable_breakup: breakup_rate[c] and
 *      breakup_rate_deficit[c] are ADDED to; the step's n_overflow (pairs whose breakup the
 *      multiplicity limit refused: what the reference warns "overflow" about) is added into
 *      events[c] at SDM_PARCEL_COAL_OVERFLOW_SHIFT; rng_offset_breakup[c] advances; the row of
 *      sdm_parcel_breakup_profile.
 *
 * With enable_breakup = 0 the call gives sdm_parcel_run_coal's results to the bit and neither
 * reads nor writes the arrays of sdm_parcel_breakup_state / _profile (they may be NULL).
 */
#ifndef SDM_PARCEL_BREAKUP_H
#define SDM_PARCEL_BREAKUP_H
#include "sdm_parcel_coal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what breakup adds to the parcels' state: DEVICE arrays (the struct is a host struct) */
typedef struct sdm_parcel_breakup_state {
  int64_t *breakup_rate, *breakup_rate_deficit; /* [n_parcel], added to */
  uint64_t *rng_offset_breakup;                 /* [n_parcel] draws taken from the proc/frag stream */
} sdm_parcel_breakup_state;

/* optional record: DEVICE arrays of n_steps x n_parcel, step-major like sdm_parcel_coal_profile:
 * what the step added to breakup_rate and breakup_rate_deficit, and its n_overflow.  Any member may
 * be NULL.  Entries of steps a parcel did not carry out are left untouched. */
typedef struct sdm_parcel_breakup_profile {
  int64_t *breakup_rate, *breakup_rate_deficit, *n_overflow;
} sdm_parcel_breakup_profile;

/* `n_steps` further time steps.  The arguments of sdm_parcel_run_coal, then the state `breakup`
 * and the record `breakup_profile` (each may be NULL without enable_breakup; the record always).
 * The cap stays SDM_PARCEL_COAL_MAX_ROWS.
 *
 * SDM_E_ARG: everything sdm_parcel_run_coal refuses except enable_breakup; and with
 * enable_breakup: an unknown ec or frag; max_multiplicity < 1; a set-up that needs a fall
 * velocity (SDM_EC_STRAUB2010, SDM_EC_LOWLIST1982, SDM_FRAG_STRAUB2010, SDM_FRAG_LOWLIST1982: they
 * form the pair's kinetic energy) without its table / numbers; `breakup` or one of its columns
 * missing. */
int sdm_parcel_run_collision(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, const sdm_step_cfg *coal_cfg,
                             int64_t n_steps, int64_t n_parcel, int64_t n_sd,
                             const int64_t *parcel_start, double *water_mass,
                             int64_t *multiplicity, double *vdry, double *kappa,
                             const double *f_org, double *v_cr, const sdm_parcel_state *state,
                             const double *w_mid, const sdm_parcel_profile *profile,
                             const double consts[34], const sdm_cond_formulae *formulae,
                             const sdm_parcel_coal_state *coal,
                             const sdm_parcel_coal_profile *coal_profile, int fresh_idx,
                             const sdm_parcel_breakup_state *breakup,
                             const sdm_parcel_breakup_profile *breakup_profile);

#ifdef __cplusplus
}
#endif
#endif

/*
 * sdm_parcel_coal.h -- C ABI of the adiabatic parcel with coalescence in libsdm_hip.so: whole
 * ascents of an ensemble of independent parcels under PySDM's dynamics `AmbientThermodynamics`,
 * `Condensation`, `Coalescence`, registered in that order (the only order served), in one call:
 * warm rain in a parcel (the reference's Jensen_and_Nugent_2017 with giant CCN, the coalescing
 * parcel of its seeding example).  The collisions change multiplicities, water masses and dry
 * volumes, shuffle the parcel's permutation and remove super-droplets; the next step's
 * condensation forms its sums in the order of that permutation over the live rows, as the
 * reference's does (dynamics/condensation.py reads `particulator.attributes._ParticleAttributes__idx`).
 *
 * Same conventions as sdm_parcel.h and sdm_parcel_diag.h, whose structs, constants and definitions
 * it uses, and sdm_hip.h's sdm_step_cfg for the collision set-up.  A header of its own, as every
 * path has, so that an implementation of those need not implement it.
 *
 * One time step of one parcel c (rows parcel_start[c] .. parcel_start[c + 1], N of them):
 *
 *   1. the step of sdm_parcel.h, carried out over the parcel's LIVE rows in the order of its
 *      permutation: position k of the parcel reads and writes row idx[parcel_start[c] + k], for
 *      k < n_live[c] (`idx` holds GLOBAL row numbers).  The sums are formed in position order.
 *      Rows that are not live are neither read nor written, v_cr included.  A parcel whose solver
 *      fails stops as it does in sdm_parcel.h; none of 2 - 4 happens for it, in this step or later.
 *   2. the collision step: one `Collision.__call__` (collision.py:174-194) with enable_breakup = 0
 *      on the parcel as ONE cell.  Bit for bit what sdm_collision_step (sdm_hip.h) gives for
 *        n_cell = 1, n_sd = N, the local croupier, no optimized_random;
 *        idx = the parcel's permutation relative to parcel_start[c], ctl = {n_live, n_live, 1, 1,
 *          0, ...} (fresh), cell_start = {0, n_live};
 *        multiplicity = the parcel's slice; attributes = three rows of N: water mass
 *          (mass_attr = 0), dry volume, kappa times dry volume;
 *        cfg.dt = the parcel's dt; cfg.dv = THIS step's dv = mass_of_dry_air / ((prhod + rhod) / 2)
 *          (particulator.py:95 reads mesh.dv, which parcel.py:132 sets);
 *        cfg.rng_state_inc = rng_state_inc[4 c .. 4 c + 4), state.rng_offset = rng_offset[c], which
 *          is advanced as sdm_step_result.rng_offset says: by N + N / 2 per sub-step.
 *      All sub-steps run: the adaptive loop until dt_left == 0, or `substeps` sub-steps.  A
 *      sub-step after which a multiplicity is zero ends with the reference's compaction
 *      (collisions_methods.py:664-680: holes are filled from the tail), and n_live[c] shrinks.
 *      A parcel of ONE row has no collision step (sdm_collision_step takes n_sd >= 2): nothing is
 *      drawn, no counter moves.
 *   3. kappa[row] = kappa_times_dry_volume[row] / vdry[row] for the live rows, as IEEE gives it
 *      (attributes/physics/hygroscopicity.py; point 4 of sdm_parcel_chem.h).  The next step reads it.
 *   4. per parcel, collision_rate, collision_rate_deficit and coalescence_rate are ADDED to;
 *      stats_n_substep and stats_dt_min are written as the collision step writes them; events[c]
 *      gets bit 8 (0x100) when stats_dt_min[c] equals dt_min after an adaptive sub-step, whether
 *      that sub-step or an earlier one (or the caller) put the value there (the event behind
 *      "adaptive time-step reached dt_min", control word 7 of sdm_step_state.ctl) and counts
 *      n_overflow in its bits 32 and up (breakup is refused, so these stay 0); the profile row of
 *      sdm_parcel.h; the row of sdm_parcel_coal_profile.
 *
 * A second call continues where the first stopped (run(9) == run(4); run(5)): all state, stream
 * positions included, is in the arrays.
 */
#ifndef SDM_PARCEL_COAL_H
#define SDM_PARCEL_COAL_H
#include "sdm_hip.h"
#include "sdm_parcel_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most rows a parcel may have: its permutation, multiplicities, three extensive rows and the
 * shuffle's tables live in the LDS of one workgroup for the whole time step (56 B per row) */
#define SDM_PARCEL_COAL_MAX_ROWS 2048
/* the workgroups of the collision kernel stride over the parcels: at most this many are launched */
#define SDM_PARCEL_COAL_MAX_GRID 1024
/* events[c]; _BOUND: the adaptive loop reached the bound on its sub-steps that sdm_hip.h derives
 * (where sdm_collision_step returns SDM_E_STATE) and the step's collisions stopped there */
#define SDM_PARCEL_COAL_EVENT_BOUND 0x1
#define SDM_PARCEL_COAL_EVENT_DT_MIN 0x100
#define SDM_PARCEL_COAL_OVERFLOW_SHIFT 32

/* what the third dynamic adds to the parcels' state: DEVICE arrays (the struct is a host struct) */
typedef struct sdm_parcel_coal_state {
  int64_t *idx;                    /* [n_sd] global row numbers; see point 1 */
  int64_t *n_live;                 /* [n_parcel] */
  double *kappa_times_dry_volume;  /* [n_sd] extensive */
  int64_t *collision_rate, *collision_rate_deficit, *coalescence_rate; /* [n_parcel], added to */
  int64_t *stats_n_substep;        /* [n_parcel] */
  double *stats_dt_min;            /* [n_parcel] */
  int64_t *events;                 /* [n_parcel] */
  uint64_t *rng_offset;            /* [n_parcel] doubles drawn so far from the parcel's stream */
  const uint64_t *rng_state_inc;   /* [4 n_parcel] numpy.random.PCG64(seed[c]).state per parcel */
  /* the fall velocity, as sdm_step_state carries it (NULL where the kernel needs none) */
  const double *gk_a, *gk_b, *velocity_params;
} sdm_parcel_coal_state;

/* optional record: DEVICE arrays of n_steps x n_parcel, step-major like sdm_parcel_profile; entry
 * (k * n_parcel + c) holds, for step k of the call and parcel c: n_live after the step, the
 * sub-steps of the step's collisions, what the step added to coalescence_rate and to
 * collision_rate_deficit, and the step's dv.  Any member may be NULL.  Entries of steps a parcel
 * did not carry out are left untouched. */
typedef struct sdm_parcel_coal_profile {
  int64_t *n_live, *n_substeps, *coalescence_rate, *collision_rate_deficit;
  double *dv;
} sdm_parcel_coal_profile;

/* `n_steps` further time steps.  The arguments of sdm_parcel_run with `multiplicity`, `vdry` and
 * `kappa` now in/out, and: the collision set-up `coal_cfg`, of which n_sd, n_cell, n_attr, dt, dv,
 * mass_attr, rng_state_inc and everything about breakup are IGNORED (the parcel's rows, cfg->dt,
 * the step's dv and the per-parcel streams are used); the state `coal`; the record (may be NULL);
 * `fresh_idx`: non-zero when the caller has written `idx` or `n_live` since the last call - they
 * are then read back and checked once, together with parcel_start.  cfg->steps_per_launch is
 * ignored: every step is one launch of the parcel kernel and one of the collision kernel,
 * enqueued without synchronising.
 *
 * SDM_E_ARG, beyond those of sdm_parcel_run: a ventilated descriptor; enable_breakup;
 * optimized_random; the global croupier; SDM_VELOCITY_MOMENTUM; an unknown kernel or law, or a
 * kernel that needs a fall velocity without its table / numbers; dt_min <= 0 or NaN; a parcel of
 * more than SDM_PARCEL_COAL_MAX_ROWS rows; with fresh_idx, an n_live outside 1 .. N or an idx entry
 * of a live position outside the parcel's rows. */
int sdm_parcel_run_coal(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, const sdm_step_cfg *coal_cfg,
                        int64_t n_steps, int64_t n_parcel, int64_t n_sd,
                        const int64_t *parcel_start, double *water_mass, int64_t *multiplicity,
                        double *vdry, double *kappa, const double *f_org, double *v_cr,
                        const sdm_parcel_state *state, const double *w_mid,
                        const sdm_parcel_profile *profile, const double consts[34],
                        const sdm_cond_formulae *formulae, const sdm_parcel_coal_state *coal,
                        const sdm_parcel_coal_profile *coal_profile, int fresh_idx);

#ifdef __cplusplus
}
#endif
#endif

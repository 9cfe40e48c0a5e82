/*
 * sdm_seeding.h -- C ABI of the seeding path of libsdm_hip.so: PySDM's `Seeding` dynamic
 * (PySDM/dynamics/seeding.py), i.e. the injection of super-droplets into free slots - slots whose
 * multiplicity is 0 (the reference's SeedingMethods.seeding,
 * PySDM/backends/impl_numba/methods/seeding_methods.py, and Particulator.seeding,
 * PySDM/particulator.py:447-499).
 *
 * Same conventions as sdm_hip.h (whose context, error codes and sdm_last_error() it uses): a
 * context first, DEVICE pointers owned by the caller (int64 / double), 0 = ok, negative =
 * SDM_E_*; work is enqueued on the context's stream.  A separate header so that implementations
 * of sdm_hip.h (the CPU oracle) need not implement this path.
 *
 * The contract.  The slots multiplicity[0 .. n_sd) are walked in SLOT order (not through idx).
 * The j-th slot i with multiplicity[i] == 0, for j < number_to_inject, receives
 *     s = seeded_particle_index[j]                      (repeats are legal)
 *     multiplicity[i] = seeded_particle_multiplicity[s]
 *     extensive_attributes[a, i] = seeded_particle_extensive_attributes[a, s]   for a < n_attr
 * where extensive_attributes is [n_attr, n_sd] and the seed columns are [n_seeds] and
 * [n_attr, n_seeds], read raw (not through an index).  Attribute values are copied as 8-byte
 * words: NaN payloads and the sign of zero survive.  Cell id and position of a slot are not
 * touched: a seed appears where the slot's previous owner was.
 *
 * THE ONE DELIBERATE DIFFERENCE.  The reference asserts that it injected as many as were asked for
 * only after it has written.  Here the number of free slots is known (a scan) before the first
 * store: with fewer free slots than number_to_inject NOTHING is stored - multiplicity, attributes
 * and idx stay as they are - and the shortfall is reported (see each symbol).  Likewise nothing is
 * stored if one of the first number_to_inject entries of seeded_particle_index lies outside
 * [0, n_seeds).
 */
#ifndef SDM_SEEDING_H
#define SDM_SEEDING_H
#include "sdm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* words of `status` */
#define SDM_SEED_STATUS_FREE 0      /* slots with multiplicity 0 found before the call's stores */
#define SDM_SEED_STATUS_INJECTED 1  /* number_to_inject, or 0: nothing was stored */
#define SDM_SEED_STATUS_BAD_SEED 2  /* entries of seeded_particle_index outside [0, n_seeds) */
#define SDM_SEED_STATUS_WORDS 4

/* ---- the stage: exactly the backend method (seeding_methods.py:12-68) ------------------------
 * The stores above plus idx[i] = -1 for every slot that received a seed (idx has n_sd entries).
 * Enqueues only.  `status`: int64[SDM_SEED_STATUS_WORDS] on the device, written by the call (may
 * be NULL); the caller reads it when it next synchronises: status[INJECTED] != number_to_inject
 * means that nothing was stored, for want of free slots (status[FREE] < number_to_inject) or
 * because of a seed index out of range (status[BAD_SEED] != 0).
 * number_to_inject == 0 returns before any launch (status is not written);
 * number_to_inject > n_seeds is SDM_E_ARG.                                                      */
int sdm_seeding(sdm_ctx *ctx, int64_t *idx, int64_t *multiplicity, double *extensive_attributes,
                int64_t n_attr, int64_t n_sd, const int64_t *seeded_particle_index,
                const int64_t *seeded_particle_multiplicity,
                const double *seeded_particle_extensive_attributes, int64_t n_seeds,
                int64_t number_to_inject, int64_t *status);

/* ---- the fused step: one call for one `Seeding.__call__` with a positive count ----------------
 * (dynamics/seeding.py:70-94 with particulator.py:447-499).  In this order:
 *   shuffle != 0 (the reference: a reservoir of more than one seed): seeded_particle_index, all
 *       n_seeds entries, goes through sdm_shuffle_global with u01[k] = uniform number
 *       rng_offset + k of the NumPy-PCG64 stream rng_state_inc = {state_hi, state_lo, inc_hi,
 *       inc_lo}; no uniform array comes from the caller, who advances its offset by n_seeds.  The
 *       shuffled index stays in seeded_particle_index for the next call, as in the reference.
 *   the injection of sdm_seeding (without the idx[i] = -1 stores, which the next line overwrites)
 *   idx = 0, 1, .., n_sd - 1                         (ParticleAttributes.reset_idx)
 *   sdm_remove_zero_n_or_flagged over all n_sd       (ParticleAttributes.sanitize)
 *   *new_length (host) = the number of live super-droplets, idx[0 .. *new_length) naming them in
 *       the reference's order.  The call synchronises, as sdm_remove_zero_n_or_flagged does.
 * Shortfall or a seed index out of range: multiplicity, attributes and idx are left as they were
 * (the identity and the compaction are gated on the device by the same word), the call returns
 * SDM_E_STATE with the counts in sdm_last_error(), *new_length is not written.  The seed index has
 * been shuffled by then.
 * number_to_inject == 0 returns before any launch; *new_length is not written.                  */
int sdm_seeding_step(sdm_ctx *ctx, int64_t *idx, int64_t *multiplicity,
                     double *extensive_attributes, int64_t n_attr, int64_t n_sd,
                     int64_t *seeded_particle_index, const int64_t *seeded_particle_multiplicity,
                     const double *seeded_particle_extensive_attributes, int64_t n_seeds,
                     int64_t number_to_inject, int shuffle, const uint64_t rng_state_inc[4],
                     uint64_t rng_offset, int64_t *new_length);

#ifdef __cplusplus
}
#endif
#endif

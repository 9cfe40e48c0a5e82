/*
 * sdm_parcel_chem.h -- C ABI of the adiabatic parcel with aqueous chemistry in libsdm_hip.so:
 * whole ascents of an ensemble of independent parcels under PySDM's dynamics
 * `AmbientThermodynamics`, `Condensation`, `AqueousChemistry`, registered in that order (the only
 * order served; dynamics/condensation.py:118-120 says why the order matters), in one call.  The
 * sulphate the chemistry produces in the activated droplets comes back as dry volume, which the
 * next step's critical volume and condensation solve read: cloud processing of aerosol.
 *
 * Same conventions as sdm_parcel.h, sdm_parcel_diag.h and sdm_chemistry.h, whose structs,
 * constants and definitions it uses.  A header of its own, as every path has, so that an
 * implementation of those need not implement it.
 *
 * One time step of one parcel:
 *
 *   1. the step of sdm_parcel.h, unchanged.  A parcel whose solver failed stops as it does there;
 *      the chemistry leaves its rows, mixing ratios and counters alone, in this and every later
 *      step (none of 2 - 6 happens for it).
 *   2. volume[row] = water_mass[row] / rho_w                      (the expression of sdm_parcel_diag.h)
 *   3. the chemistry of sdm_chemistry.h's sdm_chemistry_step DEFINITION (points 1-6, n_substep
 *      times, dt / n_substep each) with the parcel as ONE cell: T, p, rhod are the parcel's values
 *      AFTER the parcel step (the reference reads get_predicted("T" / "p" / "rhod"),
 *      particulator.py:270-272, 287, after update_TpRH()); cell_volume is this step's
 *      dv = mass_of_dry_air / ((prhod + rhod) / 2) (mesh.dv, particulator.py:274); the rows are in
 *      row order.  Within a sub-step every row's points 1-3 read the parcel's six mixing ratios as
 *      at the sub-step's entry; a closed system then forms the six `taken` sums over the flagged
 *      rows (SDM_CHEM_SUM_ORDERED or _BLOCKED, the shapes of that header) and applies
 *      chem_delta_mr, if at least one row is flagged; then every row's points 4-6.  This is bit for
 *      bit what sdm_chemistry_step gives for n_cell = 1, an identity idx over the parcel's rows and
 *      cfg.cell_volume = dv.
 *   4. vdry[row]  = moles_S_VI[row] * dry_factor     (dry_factor: one double formed by the caller as
 *                                                     dry_molar_mass / dry_rho, as the reference's
 *                                                     `*=` does; attributes/physics/dry_volume.py)
 *      kappa[row] = kappa_times_dry_volume[row] / vdry[row]   (as IEEE gives it, zero and NaN
 *                                                     included; attributes/physics/hygroscopicity.py)
 *      both written to the columns the next step reads.
 *   5. the per-parcel counters n_failed, n_negative, n_exceeded (what sdm_chemistry_step counts)
 *      are ADDED to.  Nothing traps.
 *   6. the profile row of sdm_parcel.h; the chemistry profile row; with a request table, the
 *      table on the columns AFTER point 4 at the temperature after the step: exactly what
 *      sdm_parcel_diagnose writes for that state, bit for bit (what a PySDM product sees at output
 *      time; the dry-volume spectrum of that table is the Hoppel-gap figure).
 */
#ifndef SDM_PARCEL_CHEM_H
#define SDM_PARCEL_CHEM_H
#include "sdm_chemistry.h"
#include "sdm_parcel_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the workgroups of the chemistry kernel stride over the parcels: at most this many are launched */
#define SDM_PARCEL_CHEM_MAX_GRID 1024

/* optional record of the chemistry: DEVICE arrays of n_steps x n_parcel, step-major like
 * sdm_parcel_profile; entry (k * n_parcel + c) holds, for step k of the call and parcel c:
 *   mixing_ratio[g]  the parcel's mixing ratio of gas g after the step (SDM_CHEM_GAS_* order)
 *   aq_total[a]      the SUM of sdm_parcel_diag.h (its fixed 256-partial shape) of
 *                    (double)n_q * moles[a][q] over ALL rows of the parcel (SDM_CHEM_AQ_* order)
 *   n_flagged        the number of rows with do_chemistry_flag set after the step
 *   dv               the step's dv
 * Any member may be NULL.  Entries of steps a parcel did not carry out are left untouched. */
typedef struct sdm_parcel_chem_profile {
  double *mixing_ratio[6];
  double *aq_total[7];
  int64_t *n_flagged;
  double *dv;
} sdm_parcel_chem_profile;

/* `n_steps` further time steps.  The arguments of sdm_parcel_run_diag, with `vdry` and `kappa` now
 * in/out, and: kappa_times_dry_volume (read only), the seven `moles` columns (SDM_CHEM_AQ_*
 * order), pH and do_chemistry_flag (per droplet, length n_sd, in/out); env_mixing_ratio (six
 * DEVICE arrays of n_parcel, gas order; written by a closed system only); the 62 chemistry
 * constants; dry_factor; the counters (DEVICE arrays of n_parcel, any may be NULL); the chemistry
 * profile (may be NULL).  Of `chem_cfg`, cell_volume and timestep are IGNORED (the step's dv and
 * cfg->dt are used), and so is `constants` (the parcel's 17 constants are evaluated once per step).
 * cfg->steps_per_launch is ignored too: every step is one launch of the parcel kernel, one of the
 * chemistry kernel and, with a request table, one of the diagnostics kernel, enqueued without
 * synchronising.  `diag->dv`, if given, is written as in sdm_parcel_run_diag.
 *
 * A second call continues where the first stopped (run(9) == run(4); run(5)), as in sdm_parcel.h:
 * all state is in the arrays.
 *
 * SDM_E_ARG, beyond those of sdm_parcel_run_diag: a surface tension other than Constant (the
 * organic fraction would have to follow the dry volume), n_substep < 1, an unknown system or sum
 * mode, a missing column. */
int sdm_parcel_run_chem(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, const sdm_chemistry_cfg *chem_cfg,
                        int64_t n_steps, int64_t n_parcel, int64_t n_sd,
                        const int64_t *parcel_start, double *water_mass,
                        const int64_t *multiplicity, double *vdry, double *kappa,
                        const double *f_org, double *v_cr, const sdm_parcel_state *state,
                        const double *w_mid, const sdm_parcel_profile *profile,
                        const double consts[34], const sdm_cond_formulae *formulae,
                        const sdm_parcel_requests *requests, const sdm_parcel_diag *diag,
                        const double *kappa_times_dry_volume, double *const moles[7], double *pH,
                        uint8_t *do_chemistry_flag, double *const env_mixing_ratio[6],
                        const double chem_consts[62], double dry_factor, int64_t *n_failed,
                        int64_t *n_negative, int64_t *n_exceeded,
                        const sdm_parcel_chem_profile *chem_profile);

#ifdef __cplusplus
}
#endif
#endif

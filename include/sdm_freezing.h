/*
 * sdm_freezing.h -- C ABI of the freezing path of libsdm_hip.so: PySDM's `Freezing` dynamic
 * (singular and time-dependent immersion freezing, homogeneous freezing, thaw; the reference's
 * FreezingMethods, PySDM/backends/impl_numba/methods/freezing_methods.py), the water activity
 * with respect to ice that `Moist` keeps per cell (impl_numba/methods/physics_methods.py:78-105)
 * and the mass / volume conversions of particle_shape_and_density MixedPhaseSpheres.
 *
 * Same conventions as sdm_hip.h (whose context, error codes and sdm_last_error() it uses): a
 * context first, DEVICE pointers owned by the caller (int64 / double), 0 = ok, negative =
 * SDM_E_*; every function only enqueues work on the context's stream.  A separate header so that
 * implementations of sdm_hip.h (the CPU oracle) need not implement this path.
 *
 * A super-droplet's phase is the sign of its `signed_water_mass`: > 0 liquid, < 0 ice; freezing
 * and thawing are m = -1 * m.  The constants travel in `consts`, a host array of SDM_FRZ_N_CONSTS
 * doubles in the order of the SDM_FRZ_K_* indices, so that a user's constants override applies.
 * The nucleation-rate formulae travel as integer codes (SDM_FRZ_JHET_*, SDM_FRZ_JHOM_*).
 */
#ifndef SDM_FREEZING_H
#define SDM_FREEZING_H
#include "sdm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDM_FRZ_K_T0 0
#define SDM_FRZ_K_RHO_W 1
#define SDM_FRZ_K_RHO_I 2
#define SDM_FRZ_K_EPS 3
#define SDM_FRZ_K_FWC_I0 4 /* .. FWC_I8 = 12 */
#define SDM_FRZ_K_J_HET 13
#define SDM_FRZ_K_ABIFM_M 14
#define SDM_FRZ_K_ABIFM_C 15
#define SDM_FRZ_K_ABIFM_UNIT 16
#define SDM_FRZ_K_J_HOM 17
#define SDM_FRZ_K_KOOP_2000_C1 18 /* .. KOOP_2000_C4 = 21 */
#define SDM_FRZ_K_KOOP_CORR 22
#define SDM_FRZ_K_KOOP_UNIT 23
#define SDM_FRZ_K_KOOP_MIN_DA_W_ICE 24
#define SDM_FRZ_K_KOOP_MAX_DA_W_ICE 25
#define SDM_FRZ_K_KOOP_MURRAY_C0 26 /* .. KOOP_MURRAY_C6 = 32 */
#define SDM_FRZ_N_CONSTS 33

/* heterogeneous_ice_nucleation_rate (physics/heterogeneous_ice_nucleation_rate/) */
#define SDM_FRZ_JHET_CONSTANT 0 /* J_HET; a_w_ice is not read */
#define SDM_FRZ_JHET_ABIFM 1    /* 10^(ABIFM_M (1 - a_w_ice) + ABIFM_C) ABIFM_UNIT */
/* homogeneous_ice_nucleation_rate (physics/homogeneous_ice_nucleation_rate/) */
#define SDM_FRZ_JHOM_CONSTANT 0        /* J_HOM; every d_a_w_ice is in range, a_w_ice not read */
#define SDM_FRZ_JHOM_KOOP2000 1        /* Koop et al. 2000 */
#define SDM_FRZ_JHOM_KOOP_CORRECTION 2 /* ... with the correction of Spichtinger et al. 2023 */
#define SDM_FRZ_JHOM_KOOPMURRAY2016 3  /* Koop & Murray 2016 (a function of T) */

/* how sdm_freezing_step obtains the nucleation rates, which depend on the cell only */
#define SDM_FRZ_RATES_AUTO 0        /* per cell while n_cell <= SDM_FRZ_RATES_MAX_CELLS (measured: */
                                    /* faster up to that many cells)       */
#define SDM_FRZ_RATES_PER_DROPLET 1 /* evaluated for every eligible super-droplet */
#define SDM_FRZ_RATES_PER_CELL 2    /* once per cell and workgroup, kept in LDS */
#define SDM_FRZ_RATES_MAX_CELLS 1024 /* SDM_FRZ_RATES_PER_CELL beyond this is SDM_E_ARG */

/* ---- stage by stage: one launch each, the reference method of the same name ----------------- */
/* freezing_methods.py:40-66.  Rows with freezing_temperature == 0 are skipped.  Thaw first:
 * thaw && m < 0 && T[cell] > T0; else freezing: m > 0 && RH[cell] > 1 && T[cell] <= T_fz.      */
int sdm_freeze_singular(sdm_ctx *ctx, double *signed_water_mass,
                        const double *freezing_temperature, const double *temperature,
                        const double *relative_humidity, const int64_t *cell, int64_t n_sd,
                        int thaw, const double consts[33]);
/* :68-111.  Rows with immersed_surface_area == 0 are skipped.  Thaw as above; else, for m > 0 &&
 * RH[cell] > 1: prob = 1 - exp(-(j_het(a_w_ice[cell]) * area) * timestep), frozen if rand < prob */
int sdm_freeze_time_dependent(sdm_ctx *ctx, const double *rand, double *signed_water_mass,
                              const double *immersed_surface_area, double timestep,
                              const int64_t *cell, const double *a_w_ice,
                              const double *temperature, const double *relative_humidity,
                              int64_t n_sd, int thaw, int j_het, const double consts[33]);
/* :113-168.  No row is skipped.  Thaw as above; else, for m > 0 && RH_ice[cell] > 1:
 * d = (RH_ice - 1) * a_w_ice; if d is within the formula's range (Koop*: d >= KOOP_MIN_DA_W_ICE),
 * d is limited to its maximum (Koop*: KOOP_MAX_DA_W_ICE) and
 * prob = 1 - exp(-(j_hom(T[cell], d) * volume) * timestep), frozen if rand < prob              */
int sdm_freeze_time_dependent_homogeneous(sdm_ctx *ctx, const double *rand,
                                          double *signed_water_mass, const double *volume,
                                          double timestep, const int64_t *cell,
                                          const double *a_w_ice, const double *temperature,
                                          const double *relative_humidity_ice, int64_t n_sd,
                                          int thaw, int j_hom, const double consts[33]);
/* :236-260.  m > 0 (unfrozen): data > 0 becomes NaN; otherwise: a NaN data becomes T[cell]     */
int sdm_record_freezing_temperatures(sdm_ctx *ctx, double *data, const int64_t *cell_id,
                                     const double *temperature, const double *signed_water_mass,
                                     int64_t n_sd);
/* physics_methods.py:78-105, per cell: pvi = pvs_ice(T) (Flatau-Walko-Cotton), pv = p qv /
 * (qv + eps), pvs = pv / RH; a_w_ice = pvi / pvs, RH_ice = pv / pvi                            */
int sdm_a_w_ice(sdm_ctx *ctx, const double *T, const double *p, const double *RH,
                const double *water_vapour_mixing_ratio, double *a_w_ice, double *RH_ice,
                int64_t n, const double consts[33]);
/* mixed_phase_spheres.py: max(0, m) / rho_w + min(0, m) / rho_i, and
 * max(0, v) * rho_w + min(0, v) * rho_i                                                        */
int sdm_volume_of_signed_water_mass(sdm_ctx *ctx, double *volume, const double *mass, int64_t n,
                                    const double consts[33]);
int sdm_signed_water_mass_of_volume(sdm_ctx *ctx, double *mass, const double *volume, int64_t n,
                                    const double consts[33]);

/* ---- the fused step: one launch for one `Freezing.__call__` (dynamics/freezing.py:62-87) ----- */
typedef struct sdm_freezing_cfg {
  int32_t singular, immersion_freezing, homogeneous_freezing, thaw; /* Freezing(...)'s keywords */
  int32_t j_het, j_hom;  /* SDM_FRZ_JHET_* / SDM_FRZ_JHOM_* */
  int32_t rates;         /* SDM_FRZ_RATES_* */
  int32_t reserved;      /* 0 */
  double timestep;
  uint64_t rng_state_inc[4]; /* NumPy PCG64: {state_hi, state_lo, inc_hi, inc_lo} */
} sdm_freezing_cfg;

/* Exactly this stage sequence, one thread carrying a super-droplet through all of it:
 *   immersion_freezing &&  singular: sdm_freeze_singular
 *   immersion_freezing && !singular: sdm_freeze_time_dependent with rand[i] = uniform number
 *                                    rng_offset + i of the PCG64 stream
 *   homogeneous_freezing:            sdm_freeze_time_dependent_homogeneous on the masses that
 *                                    left, with rand[i] = uniform number rng_offset + n_sd + i if
 *                                    the time-dependent immersion pass ran, else rng_offset + i
 *   temperature_of_last_freezing:    sdm_record_freezing_temperatures on it, if not NULL
 * No uniform array exists in memory; the caller advances its offset by n_sd per stochastic pass.
 * A per-droplet column may be NULL where the configuration does not read it
 * (freezing_temperature, immersed_surface_area), likewise RH / a_w_ice / RH_ice.  `volume` NULL
 * with homogeneous_freezing: the MixedPhaseSpheres volume of the mass the droplet has when the
 * homogeneous pass reaches it, which is what PySDM's `volume` attribute holds at that point (it
 * follows the signed water mass).  Rows that do not change are not stored.                     */
int sdm_freezing_step(sdm_ctx *ctx, const sdm_freezing_cfg *cfg, uint64_t rng_offset,
                      int64_t n_sd, int64_t n_cell, double *signed_water_mass,
                      const double *freezing_temperature, const double *immersed_surface_area,
                      const double *volume, const int64_t *cell_id,
                      double *temperature_of_last_freezing, const double *T, const double *RH,
                      const double *a_w_ice, const double *RH_ice, const double consts[33]);

#ifdef __cplusplus
}
#endif
#endif

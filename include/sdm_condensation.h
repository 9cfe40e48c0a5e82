/*
 * sdm_condensation.h -- C ABI of the condensation path of libsdm_hip.so: PySDM's `Condensation`
 * dynamic (the reference's CondensationMethods, PySDM/backends/impl_numba/methods/
 * condensation_methods.py) and the elementwise ambient-thermodynamics methods that `Parcel`,
 * `Moist` and the attributes of `Condensation` call (impl_numba/methods/physics_methods.py).
 *
 * Same conventions as sdm_hip.h (whose context, error codes and sdm_last_error() it uses): a
 * context first, DEVICE pointers owned by the caller (int64 / double / uint8), 0 = ok, negative =
 * SDM_E_*; every function only enqueues work on the context's stream.  A separate header so that
 * implementations of sdm_hip.h (the CPU oracle) need not implement this path.
 *
 * Physics: PySDM's DEFAULT Formulae only (diffusion_coordinate WaterMassLogarithm,
 * saturation_vapour_pressure FlatauWalkoCotton, latent_heat_vapourisation Kirchhoff,
 * hygroscopicity KappaKoehlerLeadingTerms, drop_growth Mason1971, surface_tension Constant,
 * diffusion_kinetics FuchsSutugin, diffusion_thermics Neglect, ventilation Neglect,
 * state_variable_triplet LibcloudphPlusPlus, air_dynamic_viscosity ZografosEtAl1987,
 * particle_shape_and_density LiquidSpheres).  The constants travel in `consts`, a host array of
 * SDM_COND_N_CONSTS doubles in the order of the SDM_COND_K_* indices, so that a user's constants
 * override applies.
 */
#ifndef SDM_CONDENSATION_H
#define SDM_CONDENSATION_H
#include "sdm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDM_COND_K_RHO_W 0
#define SDM_COND_K_RV 1
#define SDM_COND_K_RD 2
#define SDM_COND_K_C_PD 3
#define SDM_COND_K_C_PV 4
#define SDM_COND_K_C_PW 5
#define SDM_COND_K_L_TRI 6
#define SDM_COND_K_T_TRI 7
#define SDM_COND_K_T0 8
#define SDM_COND_K_P1000 9
#define SDM_COND_K_EPS 10
#define SDM_COND_K_SGM_W 11
#define SDM_COND_K_D0 12
#define SDM_COND_K_K0 13
#define SDM_COND_K_MAC 14
#define SDM_COND_K_HAC 15
#define SDM_COND_K_PI 16
#define SDM_COND_K_PI_4_3 17
#define SDM_COND_K_RD_OVER_C_PD 18
#define SDM_COND_K_ONE_THIRD 19
#define SDM_COND_K_THREE 20
#define SDM_COND_K_FWC_C0 21 /* .. FWC_C8 = 29 */
#define SDM_COND_K_ZOGRAFOS_T3 30
#define SDM_COND_K_ZOGRAFOS_T2 31
#define SDM_COND_K_ZOGRAFOS_T1 32
#define SDM_COND_K_ZOGRAFOS_T0 33
#define SDM_COND_N_CONSTS 34

/* ---- condensation (condensation_methods.py:52-176 `condensation` / `_condensation`, with the
 * solver of `make_condensation_solver`, :575-700) --------------------------------------------
 * PySDM's keyword set of Particulator.condensation (particulator.py:112-154) plus the solver's
 * parameters (dt_min, dt_max = `dt_range`, adaptive, fuse, multiplier, RH_rtol, max_iters).
 * For every cell of `cell_order` with super-droplets (positions cell_start[c] .. cell_start[c+1]
 * of `idx`): the adaptive sub-step count (fake steps), then the trapezoidal sub-steps; writes
 * water_mass of the cell's droplets, pthd[c], predicted_water_vapour_mixing_ratio[c],
 * n_substeps[c] (read as the previous count), n_activating[c], n_deactivating[c],
 * n_ripening[c], RH_max[c], success[c].  Empty cells are left untouched.  A failed root bracket
 * or TOMS748 run sets success[c] = 0 (it does not abort).  Per-cell sums of n * m are formed
 * serially in the order of `idx`, as in the reference.  `n_sd` is the length of the per-droplet
 * arrays; `reynolds_number` is unused while ventilation is Neglect (it may be NULL).          */
int sdm_condensation(sdm_ctx *ctx, int64_t n_sd, int64_t n_cell, const int64_t *cell_start_arg,
                     double *water_mass, const double *v_cr, const int64_t *multiplicity,
                     const double *vdry, const int64_t *idx, const double *rhod,
                     const double *thd, const double *water_vapour_mixing_ratio, double dv,
                     const double *prhod, double *pthd,
                     double *predicted_water_vapour_mixing_ratio, const double *kappa,
                     const double *f_org, double rtol_x, double rtol_thd, double timestep,
                     int64_t *n_substeps, int64_t *n_activating, int64_t *n_deactivating,
                     int64_t *n_ripening, const int64_t *cell_order, double *RH_max,
                     uint8_t *success, const double *reynolds_number, const double *air_density,
                     const double *air_dynamic_viscosity, double dt_min, double dt_max,
                     int adaptive, int fuse, int multiplier, double RH_rtol, int max_iters,
                     const double consts[34]);

/* ---- ambient methods (physics_methods.py) ------------------------------------------------- */
/* :46-73: T, p and RH of every cell from rhod, thd and the water vapour mixing ratio */
int sdm_temperature_pressure_rh(sdm_ctx *ctx, const double *rhod, const double *thd,
                                const double *water_vapour_mixing_ratio, double *T, double *p,
                                double *RH, int64_t n, const double consts[34]);
/* :131-146: output = rhod * (1 + water vapour mixing ratio) */
int sdm_air_density(sdm_ctx *ctx, double *output, const double *rhod,
                    const double *water_vapour_mixing_ratio, int64_t n);
/* :148-160: Zografos et al. 1987 */
int sdm_air_dynamic_viscosity(sdm_ctx *ctx, double *output, const double *temperature,
                              int64_t n, const double consts[34]);
/* :17-44: critical wet volume of every droplet at the temperature of its cell (`cell`) */
int sdm_critical_volume(sdm_ctx *ctx, double *v_cr, const double *kappa, const double *f_org,
                        const double *v_dry, const double *v_wet, const double *T,
                        const int64_t *cell, int64_t n, const double consts[34]);
/* :162-194: 2 r u rho / eta, the air's values of each droplet's cell */
int sdm_reynolds_number(sdm_ctx *ctx, double *output, const int64_t *cell_id,
                        const double *dynamic_viscosity, const double *density,
                        const double *radius, const double *velocity_wrt_air, int64_t n);
/* :196-205: y[i] += dt * dy_dt (a scalar rate, as Parcel passes it) */
int sdm_explicit_euler(sdm_ctx *ctx, double *y, int64_t n, double dt, double dy_dt);

#ifdef __cplusplus
}
#endif
#endif

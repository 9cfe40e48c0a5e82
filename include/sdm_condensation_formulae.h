/*
 * sdm_condensation_formulae.h -- C ABI of the condensation path of libsdm_hip.so for formulae
 * other than PySDM's defaults: the `_f` counterparts of sdm_condensation,
 * sdm_temperature_pressure_rh and sdm_critical_volume (include/sdm_condensation.h), each taking an
 * options descriptor next to the default path's arguments.
 *
 * A header of its own so that implementations of sdm_condensation.h need not implement it.  Same
 * conventions as sdm_hip.h: a context first, DEVICE pointers owned by the caller, 0 = ok, negative
 * = SDM_E_*; every function only enqueues work on the context's stream.
 *
 * The descriptor names one choice per option (the reference's class names in
 * PySDM/physics/<option>/; code 0 is PySDM's default) and carries the constants the non-default
 * choices read, in the order of the SDM_COND_F_* indices; the constants of the default path stay
 * in `consts` (SDM_COND_K_*).  Any choice combines with any other.  Not served here (one choice
 * each in the reference, or another path's business): state_variable_triplet,
 * air_dynamic_viscosity, pvs_ice, particle_shape_and_density other than LiquidSpheres.
 */
#ifndef SDM_CONDENSATION_FORMULAE_H
#define SDM_CONDENSATION_FORMULAE_H
#include "sdm_condensation.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the options: indices into sdm_cond_formulae.option ------------------------------------ */
#define SDM_COND_OPT_DIFFUSION_COORDINATE 0
#define SDM_COND_OPT_SATURATION_VAPOUR_PRESSURE 1
#define SDM_COND_OPT_LATENT_HEAT_VAPOURISATION 2
#define SDM_COND_OPT_HYGROSCOPICITY 3
#define SDM_COND_OPT_DROP_GROWTH 4
#define SDM_COND_OPT_SURFACE_TENSION 5
#define SDM_COND_OPT_DIFFUSION_KINETICS 6
#define SDM_COND_OPT_DIFFUSION_THERMICS 7
#define SDM_COND_OPT_VENTILATION 8
#define SDM_COND_N_OPTS 9

/* ---- the choices (PySDM's default is 0 in every row) --------------------------------------- */
enum sdm_cond_diffusion_coordinate { SDM_COND_COORD_WATER_MASS_LOGARITHM = 0,
                                     SDM_COND_COORD_WATER_MASS = 1 };
enum sdm_cond_saturation_vapour_pressure { SDM_COND_PVS_FLATAU_WALKO_COTTON = 0,
                                           SDM_COND_PVS_AUGUST_ROCHE_MAGNUS = 1,
                                           SDM_COND_PVS_BOLTON_1980 = 2,
                                           SDM_COND_PVS_LOWE_1977 = 3,
                                           SDM_COND_PVS_MURPHY_KOOP_2005 = 4,
                                           SDM_COND_PVS_WEXLER_1976 = 5 };
enum sdm_cond_latent_heat_vapourisation { SDM_COND_LV_KIRCHHOFF = 0, SDM_COND_LV_CONSTANT = 1,
                                          SDM_COND_LV_LOWE_2019 = 2 };
enum sdm_cond_hygroscopicity { SDM_COND_HYGRO_KAPPA_KOEHLER_LEADING_TERMS = 0,
                               SDM_COND_HYGRO_KAPPA_KOEHLER = 1 };
enum sdm_cond_drop_growth { SDM_COND_GROWTH_MASON_1971 = 0, SDM_COND_GROWTH_HOWELL_1949 = 1,
                            SDM_COND_GROWTH_FICK = 2 };
enum sdm_cond_surface_tension { SDM_COND_SGM_CONSTANT = 0,
                                SDM_COND_SGM_COMPRESSED_FILM_OVADNEVAITE = 1,
                                SDM_COND_SGM_SZYSZKOWSKI_LANGMUIR = 2,
                                SDM_COND_SGM_COMPRESSED_FILM_RUEHL = 3 };
enum sdm_cond_diffusion_kinetics { SDM_COND_KIN_FUCHS_SUTUGIN = 0, SDM_COND_KIN_NEGLECT = 1,
                                   SDM_COND_KIN_LOWE_ET_AL_2019 = 2,
                                   SDM_COND_KIN_GRABOWSKI_ET_AL_2011 = 3 };
enum sdm_cond_diffusion_thermics { SDM_COND_THERM_NEGLECT = 0,
                                   SDM_COND_THERM_TRACY_WELCH_PORTER = 1,
                                   SDM_COND_THERM_LOWE_ET_AL_2019 = 2,
                                   SDM_COND_THERM_GRABOWSKI_ET_AL_2011 = 3 };
enum sdm_cond_ventilation { SDM_COND_VENT_NEGLECT = 0, SDM_COND_VENT_FROESSLING_1938 = 1,
                            SDM_COND_VENT_PRUPPACHER_AND_RASMUSSEN_1979 = 2 };

/* ---- the constants of the non-default choices: indices into sdm_cond_formulae.consts -------- */
#define SDM_COND_F_SGM_ORG 0
#define SDM_COND_F_DELTA_MIN 1
#define SDM_COND_F_RUEHL_NU_ORG 2
#define SDM_COND_F_RUEHL_A0 3
#define SDM_COND_F_RUEHL_C0 4
#define SDM_COND_F_RUEHL_M_SIGMA 5
#define SDM_COND_F_RUEHL_SGM_MIN 6
#define SDM_COND_F_N_A 7
#define SDM_COND_F_R_STR 8
#define SDM_COND_F_WATER_MOLAR_VOLUME 9
#define SDM_COND_F_ARM_C1 10 /* .. ARM_C3 = 12 */
#define SDM_COND_F_B80W_G0 13 /* .. B80W_G2 = 15 */
#define SDM_COND_F_L77W_A0 16 /* .. L77W_A6 = 22 */
#define SDM_COND_F_MK05_LIQ_C1 23 /* .. MK05_LIQ_C13 = 35 */
#define SDM_COND_F_W76W_G0 36 /* .. W76W_G8 = 44 */
#define SDM_COND_F_ONE_KELVIN 45
#define SDM_COND_F_L_L19_A 46
#define SDM_COND_F_L_L19_B 47
#define SDM_COND_F_D_L19_A 48
#define SDM_COND_F_D_L19_B 49
#define SDM_COND_F_K_L19_A 50
#define SDM_COND_F_K_L19_B 51
#define SDM_COND_F_K_L19_C 52
#define SDM_COND_F_P_STP 53
#define SDM_COND_F_D_EXP 54
#define SDM_COND_F_D_G11_A 55 /* diffusion_thermics_D_G11_A .. _C = 57 */
#define SDM_COND_F_K_G11_A 58 /* diffusion_thermics_K_G11_A .. _D = 61 */
#define SDM_COND_F_DV_PK05 62
#define SDM_COND_F_FROESSLING_1938_A 63
#define SDM_COND_F_FROESSLING_1938_B 64
#define SDM_COND_F_PR79_XTHRES 65 /* PRUPPACHER_RASMUSSEN_1979_XTHRES */
#define SDM_COND_F_PR79_CONSTSMALL 66
#define SDM_COND_F_PR79_COEFFSMALL 67
#define SDM_COND_F_PR79_POWSMALL 68
#define SDM_COND_F_PR79_CONSTBIG 69
#define SDM_COND_F_PR79_COEFFBIG 70
#define SDM_COND_F_ONE_HALF 71
#define SDM_COND_F_N_CONSTS 72

typedef struct sdm_cond_formulae {
  int32_t option[10]; /* SDM_COND_OPT_* -> the choice's code; [9] is reserved (0) */
  double consts[72];  /* SDM_COND_F_* */
} sdm_cond_formulae;

/* sdm_condensation with the formulae of `formulae` (a HOST struct, read before the call
 * returns).  As sdm_condensation, and: `f_org` (the organic fraction of the dry volume, per
 * droplet) is read by every surface tension but Constant; `reynolds_number` (per droplet) is read
 * by every ventilation but Neglect and may be NULL only with Neglect; `air_density` and
 * `air_dynamic_viscosity` (per cell) are read with ventilation too (the Schmidt number of each
 * sub-step).  CompressedFilmRuehl solves its isotherm with TOMS748 (bracket (1e-16, 1), rtol 1e-6,
 * at most 100 iterations) in every evaluation; where the reference asserts that the iterations
 * were not used up, the droplet counts as failed here (success[c] = 0, nothing traps).         */
int sdm_condensation_f(sdm_ctx *ctx, int64_t n_sd, int64_t n_cell, const int64_t *cell_start_arg,
                       double *water_mass, const double *v_cr, const int64_t *multiplicity,
                       const double *vdry, const int64_t *idx, const double *rhod,
                       const double *thd, const double *water_vapour_mixing_ratio, double dv,
                       const double *prhod, double *pthd,
                       double *predicted_water_vapour_mixing_ratio, const double *kappa,
                       const double *f_org, double rtol_x, double rtol_thd, double timestep,
                       int64_t *n_substeps, int64_t *n_activating, int64_t *n_deactivating,
                       int64_t *n_ripening, const int64_t *cell_order, double *RH_max,
                       uint8_t *success, const double *reynolds_number,
                       const double *air_density, const double *air_dynamic_viscosity,
                       double dt_min, double dt_max, int adaptive, int fuse, int multiplier,
                       double RH_rtol, int max_iters, const double consts[34],
                       const sdm_cond_formulae *formulae);

/* sdm_temperature_pressure_rh with the saturation vapour pressure over water of `formulae` */
int sdm_temperature_pressure_rh_f(sdm_ctx *ctx, const double *rhod, const double *thd,
                                  const double *water_vapour_mixing_ratio, double *T, double *p,
                                  double *RH, int64_t n, const double consts[34],
                                  const sdm_cond_formulae *formulae);

/* sdm_critical_volume with the surface tension (at v_wet, v_dry, f_org of each droplet) and the
 * hygroscopicity of `formulae`; a droplet whose CompressedFilmRuehl search uses up its iterations
 * gets v_cr = NaN                                                                              */
int sdm_critical_volume_f(sdm_ctx *ctx, double *v_cr, const double *kappa, const double *f_org,
                          const double *v_dry, const double *v_wet, const double *T,
                          const int64_t *cell, int64_t n, const double consts[34],
                          const sdm_cond_formulae *formulae);

#ifdef __cplusplus
}
#endif
#endif

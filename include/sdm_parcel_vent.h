/*
 * sdm_parcel_vent.h -- C ABI of the ventilated parcel in libsdm_hip.so: the adiabatic parcel of
 * include/sdm_parcel.h (with the diagnostics of include/sdm_parcel_diag.h) whose condensation is
 * ventilated, i.e. whose formulae name a ventilation other than Neglect.  Every droplet's Reynolds
 * number is formed inside the time-step loop from its radius, the terminal velocity of that radius
 * and the environment's air density and dynamic viscosity
 * (PySDM/attributes/physics/reynolds_number.py, environments/impl/moist.py:26-37,73-100,110-116,
 * environments/parcel.py:51-71,142-153, particulator.py:151-153).
 *
 * Same conventions as sdm_parcel.h, which it extends.  A header of its own, as every path has, so
 * that an implementation of sdm_parcel_diag.h need not implement it.
 *
 * The air the Reynolds number reads.  `air_density` and `air_dynamic_viscosity` are the
 * environment's CURRENT values, which the reference computes in `Moist.sync` - after the advance of
 * rhod and BEFORE the condensation of a step - and does not refresh when `update_TpRH` overwrites
 * T after the condensation.  The droplets' Reynolds numbers of step k are evaluated before that
 * step's sync.  So step k reads the pair formed in step k - 1 from that step's advanced rhod and
 * the thd and qv of before its condensation; before the first step the pair is that of the
 * initial state (`Parcel.register`: rhod0, thd0, qv0).  Each parcel carries the pair from step to
 * step, from launch to launch and from call to call.
 *
 * One time step of one parcel, in plain IEEE doubles, left to right, without contraction; what is
 * not written out is the step of sdm_parcel.h (whose names these are), the transcendentals those
 * of the library (csrc/sdm_math.h):
 *
 *   (rho_air, eta_air) = the carried pair
 *   delta .. dv        = the advance of sdm_parcel.h
 *   T_sync       = the T of sdm_temperature_pressure_rh_f(prhod, thd, qv)
 *   rho_air_new  = prhod * (1 + qv)                                          (sdm_air_density)
 *   eta_air_new  = Z3 * sdm_pow(T_sync, 3) + Z2 * sdm_pow(T_sync, 2) + Z1 * T_sync + Z0
 *                                                                  (sdm_air_dynamic_viscosity)
 *   radius[row]  = sign(v) * sdm_pow(|v * (1 / PI_4_3)|, 1 / 3) of v = water_mass / rho_w
 *   with the table law: if any radius[row] > gk_top: failed_step = steps_done, out_of_table = 1,
 *           and the parcel stops with its state (v_cr, reynolds_number and the pair included) as
 *           before the step
 *   u[row]       = the law's velocity of radius[row]: sdm_interpolation, sdm_terminal_velocity or
 *                  sdm_power_series
 *   reynolds_number[row] = 2 * radius[row] * u[row] * rho_air / eta_air   (sdm_reynolds_number)
 *   v_cr[row]    = as in sdm_parcel.h
 *   the solver of sdm_condensation_f as in sdm_parcel.h, with reynolds_number and, through all its
 *           sub-steps, the carried pair (rho_air, eta_air) as the cell's air
 *   if not success: as in sdm_parcel.h; the carried pair stays (reynolds_number, like v_cr, holds
 *           the values of the failed step)
 *   the rest of the step of sdm_parcel.h
 *   the carried pair = (rho_air_new, eta_air_new)
 */
#ifndef SDM_PARCEL_VENT_H
#define SDM_PARCEL_VENT_H
#include "sdm_hip.h"
#include "sdm_parcel_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a HOST struct, read before the call returns; the pointers are DEVICE pointers */
typedef struct sdm_parcel_vent {
  /* SDM_VELOCITY_LAW_* of sdm_hip.h; velocity_terms: terms of the power series,
   * 0 .. SDM_VELOCITY_MAX_TERMS */
  int32_t velocity_law, velocity_terms;
  /* laid out as sdm_step_state.velocity_params: Rogers-Yau 5 doubles, power series velocity_terms
   * prefactors, then velocity_terms powers; not read by the table law */
  const double *velocity_params;
  /* the Gunn-Kinzer table as sdm_interpolation takes it (b, c, table_len, factor), and the radius
   * above which it must not be read; read by the table law only.  The closed forms have no range
   * check, as in the reference */
  const double *gk_a, *gk_b;
  int64_t gk_table_len;
  double gk_factor, gk_top;
  /* the carried pair: arrays of n_parcel, in/out */
  double *air_density, *air_dynamic_viscosity;
  /* a column of n_sd, an output: the values used in the last step (like v_cr) */
  double *reynolds_number;
  /* array of n_parcel or NULL: set to 1 for a parcel stopped by the table's range (never
   * cleared) */
  int64_t *out_of_table;
} sdm_parcel_vent;

/* sdm_parcel_run_diag (`requests` and `diag` may be NULL) with ventilated condensation.  Kernels of
 * its own: those of sdm_parcel_run, sdm_parcel_run_diag and sdm_parcel_run_chem do not change, and
 * these three go on refusing a ventilation other than Neglect.
 *
 * SDM_E_ARG, beyond sdm_parcel_run_diag's: `formulae` NULL or naming the ventilation Neglect,
 * `vent` NULL, an unknown law, more than SDM_VELOCITY_MAX_TERMS terms, a law that reads
 * velocity_params without them, the table law without gk_a, gk_b or a table_len >= 1, a NULL
 * air_density, air_dynamic_viscosity or reynolds_number. */
int sdm_parcel_run_vent(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, int64_t n_steps,
                        int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start,
                        double *water_mass, const int64_t *multiplicity, const double *vdry,
                        const double *kappa, const double *f_org, double *v_cr,
                        const sdm_parcel_state *state, const double *w_mid,
                        const sdm_parcel_profile *profile, const double consts[34],
                        const sdm_cond_formulae *formulae, const sdm_parcel_requests *requests,
                        const sdm_parcel_diag *diag, const sdm_parcel_vent *vent);

#ifdef __cplusplus
}
#endif
#endif

/*
 * sdm_deposition.h -- C ABI of the vapour-deposition path of libsdm_hip.so: PySDM's
 * `VapourDepositionOnIce` dynamic (growth and sublimation of ice by vapour diffusion; the
 * reference's DepositionMethods, PySDM/backends/impl_numba/methods/deposition_methods.py, called
 * by Particulator.deposition, particulator.py:501-522).
 *
 * Same conventions as sdm_hip.h (whose context, error codes and sdm_last_error() it uses): a
 * context first, DEVICE pointers owned by the caller (int64 / double), 0 = ok, negative =
 * SDM_E_*; the call only enqueues work on the context's stream and does not synchronise.  A
 * separate header so that implementations of sdm_hip.h (the CPU oracle) need not implement it.
 *
 * A super-droplet is ice where its `signed_water_mass` is not > 0.  The constants travel in
 * `consts`, a host array of SDM_DEP_N_CONSTS doubles in the order of the SDM_DEP_K_* indices, so
 * that a user's constants override applies.  The formulae choices travel as integer codes.
 * Fixed: saturation_vapour_pressure FlatauWalkoCotton (pvs_ice), latent_heat_sublimation
 * MurphyKoop2005, diffusion_thermics Neglect (D0, K0), drop_growth Mason1971,
 * state_variable_triplet LibcloudphPlusPlus (dthd_dt), both ventilation factors 1.
 */
#ifndef SDM_DEPOSITION_H
#define SDM_DEPOSITION_H
#include "sdm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDM_DEP_K_RHO_W 0
#define SDM_DEP_K_RHO_I 1
#define SDM_DEP_K_RV 2
#define SDM_DEP_K_RD 3
#define SDM_DEP_K_C_PD 4
#define SDM_DEP_K_EPS 5
#define SDM_DEP_K_P1000 6
#define SDM_DEP_K_RD_OVER_C_PD 7
#define SDM_DEP_K_PI 8
#define SDM_DEP_K_PI_4_3 9
#define SDM_DEP_K_ONE_THIRD 10
#define SDM_DEP_K_T0 11
#define SDM_DEP_K_FWC_I0 12 /* .. FWC_I8 = 20 */
#define SDM_DEP_K_MV 21
#define SDM_DEP_K_MK05_SUB_C1 22 /* .. MK05_SUB_C5 = 26 */
#define SDM_DEP_K_D0 27
#define SDM_DEP_K_K0 28
#define SDM_DEP_K_LMBD_W_0 29
#define SDM_DEP_K_T_STP 30
#define SDM_DEP_K_P_STP 31
#define SDM_DEP_K_C_CUNN 32
#define SDM_DEP_K_MAC_ICE 33
#define SDM_DEP_K_HAC_ICE 34
#define SDM_DEP_K_CAPACITY_COLUMNAR_ICE_A1 35
#define SDM_DEP_K_CAPACITY_COLUMNAR_ICE_B1 36
#define SDM_DEP_K_CAPACITY_COLUMNAR_ICE_A2 37
#define SDM_DEP_K_CAPACITY_COLUMNAR_ICE_B2 38
#define SDM_DEP_N_CONSTS 39

/* diffusion_coordinate (physics/diffusion_coordinate/) */
#define SDM_DEP_COORD_WATER_MASS_LOGARITHM 0 /* x = ln(m): m_new = exp(ln(m) + dt dm_dt / m) */
#define SDM_DEP_COORD_WATER_MASS 1           /* x = m: m_new = m + dt dm_dt; a sublimating crystal
                                                may pass through zero and come out positive */
/* diffusion_ice_capacity (physics/diffusion_ice_capacity/) */
#define SDM_DEP_CAPACITY_SPHERICAL 0
#define SDM_DEP_CAPACITY_COLUMNAR 1
/* diffusion_ice_kinetics (physics/diffusion_ice_kinetics/) */
#define SDM_DEP_KINETICS_STANDARD 0
#define SDM_DEP_KINETICS_NEGLECT 1
/* how the contributions of a cell's super-droplets are added to its two predicted values */
#define SDM_DEP_SUM_ORDERED 0 /* acc = predicted[c], then one by one in ascending row order: the
                                 reference's serial loop, the reference's bits */
#define SDM_DEP_SUM_BLOCKED 1 /* a fixed-shape sum that depends on the inputs only: the cell's
                                 contributing rows in ascending row order are cut into blocks of
                                 SDM_DEP_SUM_BLOCK consecutive entries (the last may be short); a
                                 block `a` of `len` entries is reduced as
                                   for (h = 128; h >= 1; h /= 2)
                                     for (j = 0; j < h; ++j) if (j + h < len) a[j] += a[j + h];
                                 to a[0]; then acc = predicted[c] and the block values are added
                                 in block order.  Same bits run to run and on every
                                 implementation, not the reference's */
#define SDM_DEP_SUM_BLOCK 256

typedef struct sdm_deposition_cfg {
  int32_t coordinate, capacity, kinetics, sum; /* SDM_DEP_COORD_* / _CAPACITY_* / _KINETICS_* /
                                                  _SUM_* */
  double time_step, cell_volume;
} sdm_deposition_cfg;

/* deposition_methods.py:40-130.  For every row i with signed_water_mass[i] not > 0 (no index is
 * involved: rows of multiplicity 0 are processed like any other), c = cell_id[i], in a cell with
 * S_ice = RH[c] / a_w_ice[c] != 1:
 *   dm_dt = 4 pi capacity(-m) ((S_ice - 1) / (Fk + Fd) rho_w)   (Mason1971 with ls and pvs_ice)
 *   delta = -dm_dt multiplicity[i] time_step / (cell_volume rhod[c])
 *   predicted_qv[c]  += delta
 *   predicted_thd[c] += dthd_dt(rhod[c], thd[c], T[c], delta / time_step, ls(T[c])) time_step
 *   signed_water_mass[i] = -mass(x(-m) + time_step dx_dt(-m, dm_dt))
 * Rows of a cell with S_ice == 1 and liquid rows contribute nothing and are not stored; cells
 * without a contributing row keep their predicted values bit for bit.  A row whose cell_id is
 * outside [0, n_cell) is skipped.  The additions to a cell follow cfg->sum.
 *
 * n_exceeded (a device int64, may be NULL) is SET to the number of rows with -delta > qv[c],
 * where the reference asserts.  Nothing traps and every row is processed as if the assertion
 * were absent; what to do with the count is left to the caller.
 *
 * predicted_qv == qv or predicted_thd == thd is SDM_E_ARG: with aliased arrays the reference's
 * serial loop reads a thd that earlier rows have already changed, which this path - every row
 * evaluated from the current columns, then the sums - does not reproduce.
 * n_sd == 0 is ok and touches nothing.  Scratch comes from the context's arena. */
int sdm_deposition(sdm_ctx *ctx, const sdm_deposition_cfg *cfg, int64_t n_sd, int64_t n_cell,
                   const int64_t *multiplicity, double *signed_water_mass,
                   const int64_t *cell_id, const double *T, const double *p, const double *RH,
                   const double *a_w_ice, const double *qv, const double *rhod,
                   const double *thd, double *predicted_qv, double *predicted_thd,
                   int64_t *n_exceeded, const double consts[39]);

#ifdef __cplusplus
}
#endif
#endif

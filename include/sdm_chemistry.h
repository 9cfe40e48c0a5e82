/*
 * sdm_chemistry.h -- C ABI of the aqueous-chemistry path of libsdm_hip.so: PySDM's
 * `AqueousChemistry` dynamic (pH by charge balance, Henry-law dissolution of six gases, oxidation
 * of S(IV) by O3 and H2O2; the reference's ChemistryMethods,
 * PySDM/backends/impl_numba/methods/chemistry_methods.py, called by
 * PySDM/dynamics/aqueous_chemistry.py through particulator.py:215-296).
 *
 * Same conventions as sdm_hip.h (whose context, error codes and sdm_last_error() it uses): a
 * context first, DEVICE pointers owned by the caller (int64 / double / uint8), 0 = ok, negative =
 * SDM_E_*; a call only enqueues work on the context's stream and does not synchronise.  A
 * separate header so that implementations of sdm_hip.h (the CPU oracle) need not implement it.
 *
 * Groups of columns are passed as HOST arrays of device pointers in the fixed orders below.  The
 * constants travel in `consts`, a host array of SDM_CHEM_N_CONSTS doubles in the order of the
 * SDM_CHEM_K_* indices, so that a user's constants override applies.  Amounts are in mol,
 * concentrations in mol / m3, pH = -log10(H / (1000 mol / m3)).
 */
#ifndef SDM_CHEMISTRY_H
#define SDM_CHEMISTRY_H
#include "sdm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gases, the order of the reference's GASEOUS_COMPOUNDS (key / compound) */
#define SDM_CHEM_GAS_HNO3 0 /* N_V */
#define SDM_CHEM_GAS_H2O2 1 /* H2O2 */
#define SDM_CHEM_GAS_NH3 2  /* N_mIII */
#define SDM_CHEM_GAS_SO2 3  /* S_IV */
#define SDM_CHEM_GAS_CO2 4  /* C_IV */
#define SDM_CHEM_GAS_O3 5   /* O3 */
#define SDM_CHEM_N_GAS 6
/* aqueous mole columns, the order of the reference's AQUEOUS_COMPOUNDS */
#define SDM_CHEM_AQ_S_IV 0
#define SDM_CHEM_AQ_O3 1
#define SDM_CHEM_AQ_H2O2 2
#define SDM_CHEM_AQ_C_IV 3
#define SDM_CHEM_AQ_N_V 4
#define SDM_CHEM_AQ_N_MIII 5
#define SDM_CHEM_AQ_S_VI 6
#define SDM_CHEM_N_AQ 7
/* equilibrium constants, the order of EquilibriumConsts.EQUILIBRIUM_CONST */
#define SDM_CHEM_EQ_HNO3 0
#define SDM_CHEM_EQ_SO2 1
#define SDM_CHEM_EQ_NH3 2
#define SDM_CHEM_EQ_CO2 3
#define SDM_CHEM_EQ_HSO3 4
#define SDM_CHEM_EQ_HCO3 5
#define SDM_CHEM_EQ_HSO4 6
#define SDM_CHEM_N_EQ 7
#define SDM_CHEM_N_KIN 4 /* k0 .. k3 */
/* the concentrations the pH depends on, the order of chemistry_methods.py `_conc` */
#define SDM_CHEM_CONC_N_MIII 0
#define SDM_CHEM_CONC_N_V 1
#define SDM_CHEM_CONC_C_IV 2
#define SDM_CHEM_CONC_S_IV 3
#define SDM_CHEM_CONC_S_VI 4
#define SDM_CHEM_N_CONC 5

#define SDM_CHEM_K_R_STR 0
#define SDM_CHEM_K_MD 1
#define SDM_CHEM_K_RD 2
#define SDM_CHEM_K_ROOM_TEMP 3
#define SDM_CHEM_K_K_H2O 4
#define SDM_CHEM_K_M 5
#define SDM_CHEM_K_PI_4_3 6
#define SDM_CHEM_K_ONE_THIRD 7
#define SDM_CHEM_K_PI 8
#define SDM_CHEM_K_K4 9
#define SDM_CHEM_K_DIFFUSION 10     /* .. 15, gas order: DIFFUSION_CONST */
#define SDM_CHEM_K_ACCOMMODATION 16 /* .. 21: MASS_ACCOMMODATION_COEFFICIENTS */
#define SDM_CHEM_K_MOLAR_MASS 22    /* .. 27: g / mol; specific gravity = mass * 1e-3 / Md */
#define SDM_CHEM_K_EQ_K 28          /* .. 34: K(ROOM_TEMP), SDM_CHEM_EQ_* order */
#define SDM_CHEM_K_EQ_DT 35         /* .. 41: its dT (enthalpy = -dT R_str) */
#define SDM_CHEM_K_HENRY_K 42       /* .. 47, gas order */
#define SDM_CHEM_K_HENRY_DT 48      /* .. 53 */
#define SDM_CHEM_K_KIN_K 54         /* .. 57: k(ROOM_TEMP) of k0 .. k3 */
#define SDM_CHEM_K_KIN_DT 58        /* .. 61 */
#define SDM_CHEM_N_CONSTS 62

#define SDM_CHEM_SYSTEM_OPEN 0
#define SDM_CHEM_SYSTEM_CLOSED 1
/* how `taken`, the sum over a cell's flagged rows of multiplicity * (new - old), is formed */
#define SDM_CHEM_SUM_ORDERED 0 /* acc = 0, then one by one in idx order: the reference's serial
                                  loop, the reference's bits */
#define SDM_CHEM_SUM_BLOCKED 1 /* a fixed-shape sum that depends on the inputs only: the cell's
                                  contributing rows in idx order are cut into blocks of
                                  SDM_CHEM_SUM_BLOCK consecutive entries (the last may be short); a
                                  block `a` of `len` entries is reduced as
                                    for (h = 128; h >= 1; h /= 2)
                                      for (j = 0; j < h; ++j) if (j + h < len) a[j] += a[j + h];
                                  to a[0]; then acc = 0 and the block values are added
                                  in block order.  Same bits run to run and on every
                                  implementation, not the reference's */
#define SDM_CHEM_SUM_BLOCK 256

/* where sdm_chemistry_step gets a cell's 17 temperature-dependent constants from (the same bits
 * either way; the stage symbols do not read this) */
#define SDM_CHEM_CONSTS_AUTO 0     /* as the library chooses */
#define SDM_CHEM_CONSTS_PER_ROW 1  /* every row evaluates its cell's */
#define SDM_CHEM_CONSTS_PER_CELL 2 /* once per cell and workgroup into LDS; n_cell <=
                                      SDM_CHEM_LDS_CELLS, else SDM_E_ARG */
#define SDM_CHEM_LDS_CELLS 256

typedef struct sdm_chemistry_cfg {
  int32_t n_substep, system_type, sum, constants; /* SDM_CHEM_SYSTEM_* / _SUM_* / _CONSTS_* */
  double timestep;    /* of the whole step (sdm_chemistry_step) or of the call (sdm_dissolution) */
  double cell_volume; /* dv */
  double H_min, H_max, ionic_strength_threshold, rtol; /* equilibrate_H */
} sdm_chemistry_cfg;

/* chem_recalculate_cell_data (chemistry_methods.py:292-305).  Per cell c < n_cell, from T[c]:
 *   equilibrium[e][c] = K_e exp(-(-dT_e R_str) / R_str (1 / T - 1 / ROOM_TEMP))       (vant_hoff)
 *   kinetic[k][c]     = A_k exp(-Ea_k / (R_str T)), Ea_k = -dT_k R_str,
 *                       A_k = k_k exp(Ea_k / (R_str ROOM_TEMP))                       (arrhenius)
 *   henry[g][c]       like equilibrium with the Henry constants - an output the reference does not
 *                     have (it evaluates HENRY_CONST[..].at(T) per call): sdm_dissolution reads it */
int sdm_chem_recalculate_cell_data(sdm_ctx *ctx, int64_t n_cell, const double *T,
                                   double *const equilibrium[7], double *const kinetic[4],
                                   double *const henry[6], const double consts[62]);

/* chem_recalculate_drop_data (chemistry_methods.py:282-290).  Per row i < n_sd, c = cell_id[i],
 * H = pH2H(pH[i]) = pow(10, -pH) * 1e3: the six DISSOCIATION_FACTORS in gas order; the H2O2 and O3
 * columns are set to 1. */
int sdm_chem_recalculate_drop_data(sdm_ctx *ctx, int64_t n_sd, const double *pH,
                                   const int64_t *cell_id, const double *const equilibrium[7],
                                   double *const dissociation_factors[6],
                                   const double consts[62]);

/* equilibrate_H (chemistry_methods.py:307-429), for every row i < n_sd (no index), c = cell_id[i],
 * f = acidity_minfun of conc[.][i] and equilibrium[.][c]:
 *   a = pH2H(pH[i]); |f(a)| < 1e-6: the row is left alone, its flag included;
 *   |f(a)| < 1: bracket a .. 2a, else a/4 .. a (where f changes sign), 8 iterations at most;
 *   otherwise cfg->H_min .. cfg->H_max, 32 iterations at most;
 *   H = TOMS748(f, bracket, cfg->rtol); pH[i] = H2pH(H) = -log10(H * 1e-3);
 *   do_chemistry_flag[i] = calc_ionic_strength(H) <= cfg->ionic_strength_threshold.
 * Where the solver refuses its bracket (not a < b, or no sign change) H is NaN as in the
 * reference.  n_failed (a device int64, may be NULL) is SET to the number of rows whose solve did
 * not converge: it used all its iterations, where the reference asserts, or the solver refused
 * its bracket, where the reference warns and goes on with NaN.  Nothing traps. */
int sdm_equilibrate_H(sdm_ctx *ctx, const sdm_chemistry_cfg *cfg, int64_t n_sd,
                      const int64_t *cell_id, const double *const conc[5],
                      const double *const equilibrium[7], double *pH, uint8_t *do_chemistry_flag,
                      int64_t *n_failed, const double consts[62]);

/* dissolution (chemistry_methods.py:44-156) for any n_cell.  The rows of cell c are
 * i = idx[q], cell_start[c] <= q < cell_start[c + 1] (all < n_sd, the length of the columns), with
 * do_chemistry_flag[i] set.  For every gas g, with the cell's env_mixing_ratio[g][c] AS AT ENTRY
 * (the reference changes it after its loop over the rows):
 *   moles[g][i] = A_new volume[i]                                (dissolution_body, line for line)
 *   taken[g][c] = sum over the cell's rows of multiplicity[i] * (new - old), shaped by cfg->sum
 * and, cfg->system_type closed, in cells with at least one flagged row
 *   env_mixing_ratio[g][c] -= taken * sg * Md / (cfg->cell_volume * rhod[c]).
 * Open system: no sum is formed, no scratch is written, env_mixing_ratio is not written.  Cells
 * without a flagged row keep their mixing ratios bit for bit.  `moles` are the six columns in GAS
 * order (N_V, H2O2, N_mIII, S_IV, C_IV, O3).  cfg->timestep is the time step of this call.
 * n_negative (device int64, may be NULL) is SET to the number of (row, gas) with a new amount not
 * >= 0, n_exceeded to the number of (cell, gas) of a closed system whose decrement is not <= the
 * mixing ratio: the reference's two assertions.  Nothing traps and everything is processed as if
 * the assertions were absent. */
int sdm_dissolution(sdm_ctx *ctx, const sdm_chemistry_cfg *cfg, int64_t n_sd, int64_t n_cell,
                    const int64_t *idx, const int64_t *cell_start,
                    const uint8_t *do_chemistry_flag, double *const moles[6],
                    double *const env_mixing_ratio[6], const double *T, const double *p,
                    const double *rhod, const double *const henry[6],
                    const double *const dissociation_factors[6], const double *volume,
                    const int64_t *multiplicity, int64_t *n_negative, int64_t *n_exceeded,
                    const double consts[62]);

/* oxidation (chemistry_methods.py:158-280): per row i < n_sd with the flag set, an explicit Euler
 * step of `timestep`; a row that would drive any of the four amounts negative is skipped.
 * `equilibrium` has the seven slots of the other symbols; only equilibrium[SDM_CHEM_EQ_SO2] and
 * equilibrium[SDM_CHEM_EQ_HSO3] are read, the other five must be non-NULL and are never loaded. */
int sdm_oxidation(sdm_ctx *ctx, int64_t n_sd, const int64_t *cell_id,
                  const uint8_t *do_chemistry_flag, const double *const kinetic[4],
                  const double *const equilibrium[7], double timestep, const double *volume,
                  const double *pH, const double *dissociation_factor_SO2, double *moles_O3,
                  double *moles_H2O2, double *moles_S_IV, double *moles_S_VI,
                  const double consts[62]);

/* One AqueousChemistry.__call__ (aqueous_chemistry.py:101-129).  DEFINITION: exactly this stage
 * sequence - cell data once, then cfg->n_substep times, with dt = cfg->timestep / cfg->n_substep:
 *   1. conc = moles / volume for the five species of attributes/chemistry/acidity.py; equilibrate_H
 *   2. drop data
 *   3. dissolution with dt
 *   4. conc again; equilibrate_H
 *   5. drop data
 *   6. oxidation with dt
 * The two solves are what PySDM's lazy `pH` attribute runs when moles or volume changed since it
 * was last read.  A front end whose state did NOT change since the last solve gets one more solve
 * at point 1 of the first sub-step than PySDM would run (it starts from the solved pH, so it
 * mostly leaves the row alone).
 * Read and written: pH, do_chemistry_flag, the seven `moles` columns (SDM_CHEM_AQ_* order) and, in
 * a closed system, env_mixing_ratio.  Read: volume, multiplicity, cell_id, idx / cell_start (a
 * permutation of ALL n_sd rows sorted by cell, as sdm_dissolution takes it), T, p, rhod.  No conc,
 * dissociation-factor or constant column exists in memory: a lane carries one super-droplet with
 * its amounts, pH and volume in registers; the 17 temperature-dependent constants of its cell are
 * evaluated per row at the start of the kernel, or once per cell and workgroup into LDS
 * (cfg->constants).
 * Open system: ONE launch for all sub-steps.  Closed system: the row kernel once per sub-step,
 * each followed by the sum kernel that applies the six decrements to the cells.
 * counts (device int64[3], may be NULL) is SET to {n_failed, n_negative, n_exceeded} summed over
 * the step. */
int sdm_chemistry_step(sdm_ctx *ctx, const sdm_chemistry_cfg *cfg, int64_t n_sd, int64_t n_cell,
                       const int64_t *idx, const int64_t *cell_start, const int64_t *cell_id,
                       const int64_t *multiplicity, const double *volume, double *const moles[7],
                       double *pH, uint8_t *do_chemistry_flag, const double *T, const double *p,
                       const double *rhod, double *const env_mixing_ratio[6], int64_t *counts,
                       const double consts[62]);

#ifdef __cplusplus
}
#endif
#endif

// deposition_rows.h -- the cell and row code of vapour deposition on ice (include/
// sdm_deposition.h), shared by the kernels of deposition.hip and the ice passes of the mixed-phase
// parcel (parcel_solver.h, include/sdm_parcel_ice.h): both translation units evaluate a cell's
// record and a row with this text, so the fused parcel equals the stages to the bit by
// construction.
//
// Reference: PySDM/backends/impl_numba/methods/deposition_methods.py ("dm.py" below), with the
// formulae it calls (listed at the head of deposition.hip).  Python evaluates left to right; every
// expression keeps that order, nothing is contracted (-ffp-contract=off), and pow / exp / log are
// csrc/sdm_math.h.
#ifndef SDM_DEPOSITION_ROWS_H
#define SDM_DEPOSITION_ROWS_H
#include "common.h"
#include "../../include/sdm_deposition.h"

#define DEP_CV 16     // doubles per cell record (one 128-byte line)
#ifndef DF
#define DF __device__ __forceinline__
#endif

namespace {

enum {  // the cell record
  CV_S, CV_T, CV_PVS, CV_NEG_LS, CV_LAMD_C, CV_LAMK, CV_D_B, CV_K_B, CV_RHO, CV_VOL_RHO, CV_THD,
  CV_QV, CV_FK_A, CV_FK_B, CV_FD_A, CV_UNUSED
};

struct Kd {
  double rho_w, rho_i, Rv, Rd, c_pd, PI, PI_4_3, ONE_THIRD, T0, FWC_I[9], Mv, SUB[5], D0, K0,
      lmbd_w_0, T_STP, p_STP, C_cunn, MAC_ice, HAC_ice, A1, B1, A2, B2;
};

Kd dep_consts_of(const double *c) {
  Kd k;
  k.rho_w = c[SDM_DEP_K_RHO_W]; k.rho_i = c[SDM_DEP_K_RHO_I]; k.Rv = c[SDM_DEP_K_RV];
  k.Rd = c[SDM_DEP_K_RD]; k.c_pd = c[SDM_DEP_K_C_PD]; k.PI = c[SDM_DEP_K_PI];
  k.PI_4_3 = c[SDM_DEP_K_PI_4_3]; k.ONE_THIRD = c[SDM_DEP_K_ONE_THIRD]; k.T0 = c[SDM_DEP_K_T0];
  for (int i = 0; i < 9; ++i) k.FWC_I[i] = c[SDM_DEP_K_FWC_I0 + i];
  k.Mv = c[SDM_DEP_K_MV];
  for (int i = 0; i < 5; ++i) k.SUB[i] = c[SDM_DEP_K_MK05_SUB_C1 + i];
  k.D0 = c[SDM_DEP_K_D0]; k.K0 = c[SDM_DEP_K_K0]; k.lmbd_w_0 = c[SDM_DEP_K_LMBD_W_0];
  k.T_STP = c[SDM_DEP_K_T_STP]; k.p_STP = c[SDM_DEP_K_P_STP]; k.C_cunn = c[SDM_DEP_K_C_CUNN];
  k.MAC_ice = c[SDM_DEP_K_MAC_ICE]; k.HAC_ice = c[SDM_DEP_K_HAC_ICE];
  k.A1 = c[SDM_DEP_K_CAPACITY_COLUMNAR_ICE_A1]; k.B1 = c[SDM_DEP_K_CAPACITY_COLUMNAR_ICE_B1];
  k.A2 = c[SDM_DEP_K_CAPACITY_COLUMNAR_ICE_A2]; k.B2 = c[SDM_DEP_K_CAPACITY_COLUMNAR_ICE_B2];
  return k;
}

struct DepArgs {
  int64_t n_sd, n_cell;
  const int64_t *multiplicity;
  double *m;
  const int64_t *cell;
  const double *T, *p, *RH, *a_w_ice, *qv, *rhod, *thd;
  int coordinate, capacity, kinetics;
  double dt, dv;
  // arena
  double *cv, *dq, *dth;
  int64_t *key, *ident, *cidx, *p_len;
  int64_t *n_exceeded;
  Kd k;
};

// ---- per cell ------------------------------------------------------------------------------------
// Every value is either a whole sub-expression of dm.py's loop body that does not contain the
// row, or the leading operands of a left-to-right chain up to the first one that does: the row
// code continues the chain, so the bits are those of evaluating it per row.
// (`dv`: the cell volume - g.dv for the stage kernels, the step's for a parcel)
DF void dep_cell_record(const DepArgs &g, double dv, double T, double p, double RH, double a_w_ice,
                        double qv, double rho, double thd, double *cv) {
  const Kd &k = g.k;
  // flatau_walko_cotton.py: pvs_ice
  const double t = T - k.T0;
  double pvs = k.FWC_I[7] + t * k.FWC_I[8];
  for (int i = 6; i >= 0; --i) pvs = k.FWC_I[i] + t * pvs;
  // murphy_koop_2005.py: ls
  const double ls = (k.SUB[0] + k.SUB[1] * T - k.SUB[2] * sdm_pow(T, 2.0) +
                     k.SUB[3] * sdm_exp(-sdm_pow(T / k.SUB[4], 2.0))) /
                    k.Mv;
  cv[CV_S] = RH / a_w_ice;  // dm.py:76-78
  cv[CV_T] = T;
  cv[CV_PVS] = pvs;
  cv[CV_NEG_LS] = -ls;
  if (g.kinetics == SDM_DEP_KINETICS_STANDARD) {  // standard.py
    const double lambdaD = k.lmbd_w_0 * T / k.T_STP * k.p_STP / p;
    const double lambdaK = k.lmbd_w_0 * T / k.T_STP * k.p_STP / p;
    cv[CV_LAMD_C] = lambdaD * k.C_cunn;
    cv[CV_LAMK] = lambdaK;
    // D: 4.0 * D / MAC_ice / sqrt(8.0 * Rv * T / PI) [/ r];  K: K / HAC_ice / sqrt(8.0 * Rd * T /
    // PI) / c_pd / rho [/ r]
    cv[CV_D_B] = 4.0 * k.D0 / k.MAC_ice / SDM_MATH_SQRT(8.0 * k.Rv * T / k.PI);
    cv[CV_K_B] = k.K0 / k.HAC_ice / SDM_MATH_SQRT(8.0 * k.Rd * T / k.PI) / k.c_pd / rho;
  } else {
    cv[CV_LAMD_C] = cv[CV_LAMK] = cv[CV_D_B] = cv[CV_K_B] = 0.0;  // not read
  }
  cv[CV_RHO] = rho;
  cv[CV_VOL_RHO] = dv * rho;  // dm.py:110
  cv[CV_THD] = thd;
  cv[CV_QV] = qv;
  cv[CV_FK_A] = k.rho_w * ls / T;      // mason_1971.py Fk: rho_w * lv / T [/ K * (...)]
  cv[CV_FK_B] = ls / T / k.Rv - 1;     // ... (lv / T / Rv - 1)
  cv[CV_FD_A] = k.rho_w * k.Rv * T;    // fick.py Fd: rho_w * Rv * T [/ D / pvs]
  cv[CV_UNUSED] = 0.0;
}

// ---- per row -------------------------------------------------------------------------------------
// dm.py:43-130 for one ice row of a cell with S_ice != 1; true if -delta_rv_i > qv[cid]
DF bool dep_row(const DepArgs &g, const double *__restrict__ cv, double m, int64_t mult,
                double *m_new, double *dq, double *dth) {
  const Kd &k = g.k;
  const double ice_mass = -m;
  // mixed_phase_spheres.py mass_to_radius: the liquid term is pow(0 / PI_4_3 / rho_w, ONE_THIRD)
  // = 0 for every row that gets here
  const double r_ice = sdm_pow(ice_mass / k.PI_4_3 / k.rho_i, k.ONE_THIRD);
  const double radius = 0.0 + r_ice;
  double capacity;
  if (g.capacity == SDM_DEP_CAPACITY_SPHERICAL)
    capacity = r_ice;  // spherical.py: the same expression
  else  // columnar.py
    capacity = k.A1 * sdm_pow(ice_mass, k.B1) + k.A2 * sdm_pow(ice_mass, k.B2);
  double D = k.D0, K = k.K0;  // diffusion_thermics/neglect.py; diffusion_ice_kinetics/neglect.py
  if (g.kinetics == SDM_DEP_KINETICS_STANDARD) {
    D = k.D0 / (radius / (radius + cv[CV_LAMD_C]) + cv[CV_D_B] / radius);
    K = k.K0 / (radius / (radius + cv[CV_LAMK]) + cv[CV_K_B] / radius);
  }
  const double Fk = cv[CV_FK_A] / K * cv[CV_FK_B];
  const double Fd = cv[CV_FD_A] / D / cv[CV_PVS];
  const double howell = (cv[CV_S] - 1) / (Fk + Fd) * k.rho_w;  // r_dr_dt(RH_eq=1, ...) * rho_w
  const double dm_dt = 4 * 3.141592653589793 * capacity * howell;  // dm.py:102-107 (np.pi)
  const double delta = -dm_dt * (double)mult * g.dt / cv[CV_VOL_RHO];
  *dq = delta;
  // libcloudphplusplus.py dthd_dt: -lv * dqv_dt / c_pd / T * thd * rhod, then * time_step
  *dth = cv[CV_NEG_LS] * (delta / g.dt) / k.c_pd / cv[CV_T] * cv[CV_THD] * cv[CV_RHO] * g.dt;
  if (g.coordinate == SDM_DEP_COORD_WATER_MASS_LOGARITHM) {
    const double x_old = sdm_log(ice_mass);
    const double x_new = x_old + g.dt * (dm_dt / ice_mass);
    *m_new = -sdm_exp(x_new);
  } else {
    *m_new = -(ice_mass + g.dt * dm_dt);
  }
  return -delta > cv[CV_QV];
}

}  // namespace

#endif  // SDM_DEPOSITION_ROWS_H

// parcel_solver.h -- whole ascents of adiabatic parcels (include/sdm_parcel.h) for gfx950: the
// time-step loop of PySDM's `Parcel` + `AmbientThermodynamics` + `Condensation` around the solve
// proper of condensation_solver.h, as a template over the same formulae policy.  Instantiated next
// to each instantiation of the solver (condensation.hip, condensation_formulae.hip); the entry
// point is parcel.hip, which reaches both through the two launchers declared below.
//
// References: environments/parcel.py:101-153, environments/impl/moist.py:73-100,
// dynamics/condensation.py:95-131; the step is written out in include/sdm_parcel.h.
//
// One workgroup of COND_CB lanes per parcel (the cells of k_condensation are the parcels here:
// rows parcel_start[c] .. parcel_start[c + 1], in row order - `idx` is the identity), the loop
// over the launch's time steps inside the kernel.  Parcels never communicate: no grid barrier, no
// residency assumption; the workgroups stride over the parcels, so any grid size is correct.
// Every loop has a static bound (steps per launch, fuse, n_max, max_iters).
//
// The parcel's scalars live in LDS between the steps (the solver leaves no registers: it already
// fills the budget of one workgroup per CU): every lane reads what the step needs, lane 0 alone
// writes the new state - to LDS, to the profile row, and at the end of the launch to the state
// arrays.  Per droplet, every global location (water mass, v_cr, the backup) is written and read
// by the same lane (row q of the parcel belongs to lane q % COND_CB, as in the solver), so program
// order is all the ordering they need.  cs.init() is repeated every step: the columns sit in L2.
//
// A step whose solver fails leaves the parcel as before the step: the register-cached masses are
// not written back, and the rows past COND_CH, which the solver writes in place, are restored
// from a copy taken before the step (`mass_backup`, the context's arena).
//
// What the policies provide beyond condensation_solver.h's list:
//   tprh                   T, p, RH of (rhod, thd, qv): the body of k_temperature_pressure_rh(_f)
//   lv                     the latent heat of vapourisation
//   critical_volume        the body of k_critical_volume(_f) for one row
//   Rv, Rd, c_pv           the constants the hydrostatics reads (c_pd, rho_w are there already)
#ifndef SDM_PARCEL_SOLVER_H
#define SDM_PARCEL_SOLVER_H
#include "condensation_solver.h"
#include "../../include/sdm_parcel.h"

// one sdm_parcel_run call as the launchers take it (host struct; pointers are device pointers)
struct ParcelCall {
  sdm_parcel_cfg cfg;
  int64_t n_parcel, n_sd;
  const int64_t *parcel_start, *identity, *multiplicity;
  double *water_mass, *v_cr, *mass_backup;
  const double *vdry, *kappa, *f_org, *w_mid, *consts;
  sdm_parcel_state state;
  sdm_parcel_profile profile;
  int64_t k0, k_count;  // the steps of this launch: rows k0 .. k0 + k_count of w_mid / the profile
};
// condensation.hip / condensation_formulae.hip: one launch of the default / general kernel
int sdm_parcel_launch_default(sdm_ctx *ctx, const ParcelCall &call);
int sdm_parcel_launch_general(sdm_ctx *ctx, const ParcelCall &call,
                              const sdm_cond_formulae *formulae);

#ifdef __HIPCC__
namespace {

template <class P>
struct ParcelArgs {
  CondArgs<P> c;  // the solver's parameters and the per-droplet columns (idx: the identity)
  int64_t n_parcel;
  const int64_t *parcel_start;
  double *v_cr, *mass_backup;
  const double *w_mid;
  sdm_parcel_state st;
  sdm_parcel_profile pr;
  int64_t k0, k_count, n_clamp_lo, n_clamp_hi;
  double dt, g_std;
};

// the slots of the parcel's scalars in LDS
enum { PS_Z, PS_RHOD, PS_THD, PS_QV, PS_T, PS_P, PS_RH, PS_QV_PREV, PS_PRHOD, PS_PZ, PS_N };

template <class P>
DF void parcel_steps(const ParcelArgs<P> &a) {
  __shared__ double s_par[PS_N];
  __shared__ int64_t s_nsub;
  const CondArgs<P> &g = a.c;
  const typename P::K &k = g.k;
  const int tid = (int)threadIdx.x;
  for (int64_t c = blockIdx.x; c < a.n_parcel; c += gridDim.x) {
    const int64_t row0 = a.parcel_start[c], n = a.parcel_start[c + 1] - row0;
    // (checked on the host too; failed parcels are skipped for good)
    if (row0 < 0 || n <= 0 || row0 + n > g.n_sd || a.st.failed_step[c] >= 0) continue;
    CellSolver<P> cs{g, g.idx + row0, n, c, tid};
    attach_lds<P>(cs);
    __syncthreads();  // the previous parcel's reads of s_par are over
    if (tid == 0) {
      s_par[PS_Z] = a.st.z[c];
      s_par[PS_RHOD] = a.st.rhod[c];
      s_par[PS_THD] = a.st.thd[c];
      s_par[PS_QV] = a.st.qv[c];
      s_par[PS_T] = a.st.T[c];
      s_par[PS_P] = a.st.p[c];
      s_par[PS_RH] = a.st.RH[c];
      s_par[PS_QV_PREV] = a.st.qv_prev[c];
      s_nsub = a.st.n_substeps[c];
    }
    const double mass_of_dry_air = a.st.mass_of_dry_air[c];
    int64_t done = a.st.steps_done[c];
    int64_t failed = -1;
    for (int64_t j = 0; j < a.k_count; ++j) {
      __syncthreads();  // lane 0's state of the previous step (or the load above) is in LDS
      const double thd = s_par[PS_THD], qv = s_par[PS_QV], rhod = s_par[PS_RHOD];
      const double T = s_par[PS_T];
      double prhod, dv;
      {  // advance_parcel_vars, parcel.py:101-134 (hydrostatics.drho_dz inlined)
        const double p = s_par[PS_P];
        const double w = a.w_mid[(a.k0 + j) * a.n_parcel + c];
        const double delta = s_par[PS_QV_PREV] - qv;
        const double qv_mid = qv - delta / 2;
        const double lv = P::lv(k, T);
        const double Rq = P::Rv(k) / (1 / qv_mid + 1) + P::Rd(k) / (1 + qv_mid);
        const double cp = P::c_pv(k) / (1 / qv_mid + 1) + P::c_pd(k) / (1 + qv_mid);
        const double rho = p / Rq / T;
        const double dql_dz = delta / w / a.dt;
        const double drho_dz =
            (a.g_std / T * rho * (Rq / cp - 1) - p * lv / cp / (T * T) * dql_dz) / Rq;
        prhod = rhod + a.dt * (w * drho_dz);
        dv = mass_of_dry_air / ((prhod + rhod) / 2);
        if (tid == 0) {
          s_par[PS_PZ] = s_par[PS_Z] + a.dt * w;  // (lane 0 alone reads these two again)
          s_par[PS_PRHOD] = prhod;
        }
      }
      // the critical volume of every row at the parcel's temperature; the copy of the masses the
      // solver writes in place
      for (int64_t q = tid; q < n; q += COND_CB) {
        const int64_t row = row0 + q;
        const double m = g.water_mass[row];
        a.v_cr[row] = P::critical_volume(k, row, g.kappa[row], g.vdry[row], m / P::rho_w(k), T);
        if (q >= COND_CH) a.mass_backup[row] = m;
      }
      cs.init();
      const SolveOut s = solve_cell<P>(cs, g, thd, qv, rhod, prhod, thd, qv, dv, s_nsub);
      if (!s.o.success) {  // uniform: the solver's results come from LDS after a barrier
        for (int64_t q = COND_CH + tid; q < n; q += COND_CB)
          g.water_mass[row0 + q] = a.mass_backup[row0 + q];
        failed = done;
        break;
      }
      cs.write_back();
      done += 1;
      if (tid == 0) {
        const double new_rhod = s_par[PS_PRHOD];
        double nT, np, nRH;
        P::tprh(k, new_rhod, s.o.thd, s.o.qv, nT, np, nRH);
        int64_t ns = s.n;
        if (g.adaptive) {  // dynamics/condensation.py:122-131
          ns = ns > a.n_clamp_lo ? ns : a.n_clamp_lo;
          ns = ns < a.n_clamp_hi ? ns : a.n_clamp_hi;
        }
        s_par[PS_QV_PREV] = s_par[PS_QV];
        s_par[PS_Z] = s_par[PS_PZ];
        s_par[PS_RHOD] = new_rhod;
        s_par[PS_THD] = s.o.thd;
        s_par[PS_QV] = s.o.qv;
        s_par[PS_T] = nT;
        s_par[PS_P] = np;
        s_par[PS_RH] = nRH;
        s_nsub = ns;
        // the counters and RH_max are not read by the next step: straight to the state arrays
        a.st.n_activating[c] = s.o.n_activating;
        a.st.n_deactivating[c] = s.o.n_deactivating;
        a.st.n_ripening[c] = s.o.n_ripening;
        a.st.RH_max[c] = s.o.RH_max;
        const int64_t at = (a.k0 + j) * a.n_parcel + c;
        if (a.pr.z) a.pr.z[at] = s_par[PS_Z];
        if (a.pr.rhod) a.pr.rhod[at] = new_rhod;
        if (a.pr.thd) a.pr.thd[at] = s.o.thd;
        if (a.pr.qv) a.pr.qv[at] = s.o.qv;
        if (a.pr.T) a.pr.T[at] = nT;
        if (a.pr.p) a.pr.p[at] = np;
        if (a.pr.RH) a.pr.RH[at] = nRH;
        if (a.pr.RH_max) a.pr.RH_max[at] = s.o.RH_max;
        if (a.pr.n_substeps) a.pr.n_substeps[at] = ns;
        if (a.pr.n_activating) a.pr.n_activating[at] = s.o.n_activating;
        if (a.pr.n_deactivating) a.pr.n_deactivating[at] = s.o.n_deactivating;
        if (a.pr.n_ripening) a.pr.n_ripening[at] = s.o.n_ripening;
      }
    }
    if (tid == 0) {  // (lane 0 wrote s_par itself: program order)
      if (failed >= 0) a.st.failed_step[c] = failed;  // (the failed step left s_par as it was)
      a.st.z[c] = s_par[PS_Z];
      a.st.rhod[c] = s_par[PS_RHOD];
      a.st.thd[c] = s_par[PS_THD];
      a.st.qv[c] = s_par[PS_QV];
      a.st.T[c] = s_par[PS_T];
      a.st.p[c] = s_par[PS_P];
      a.st.RH[c] = s_par[PS_RH];
      a.st.qv_prev[c] = s_par[PS_QV_PREV];
      a.st.n_substeps[c] = s_nsub;
      a.st.steps_done[c] = done;
    }
  }
}

}  // namespace

// what both launchers do with a ParcelCall: the fields of ParcelArgs<P> and of its CondArgs<P>
// (`a.c.k` is the caller's)
#define SDM_PARCEL_FILL_ARGS(a, call)                                                          \
  do {                                                                                         \
    const sdm_parcel_cfg &cfg__ = (call).cfg;                                                  \
    double dt_max__ = cfg__.dt_max;                                                            \
    if (dt_max__ > cfg__.dt) dt_max__ = cfg__.dt; /* make_adapt_substeps, cm.py:181-188 */     \
    (a).c.n_sd = (call).n_sd;                                                                  \
    (a).c.n_cell = (call).n_parcel;                                                            \
    (a).c.cell_start = (call).parcel_start;                                                    \
    (a).c.idx = (call).identity;                                                               \
    (a).c.multiplicity = (call).multiplicity;                                                  \
    (a).c.cell_order = nullptr;                                                                \
    (a).c.water_mass = (call).water_mass;                                                      \
    (a).c.v_cr = (call).v_cr;                                                                  \
    (a).c.vdry = (call).vdry;                                                                  \
    (a).c.kappa = (call).kappa;                                                                \
    (a).c.rhod = (a).c.thd = (a).c.qv = (a).c.prhod = nullptr;                                 \
    (a).c.pthd = (a).c.pqv = (a).c.RH_max = nullptr;                                           \
    (a).c.n_substeps = (a).c.n_activating = (a).c.n_deactivating = (a).c.n_ripening = nullptr; \
    (a).c.success = nullptr;                                                                   \
    (a).c.dv = 0;                                                                              \
    (a).c.rtol_x = cfg__.rtol_x;                                                               \
    (a).c.rtol_thd = cfg__.rtol_thd;                                                           \
    (a).c.timestep = cfg__.dt;                                                                 \
    (a).c.RH_rtol = cfg__.RH_rtol;                                                             \
    (a).c.n_min = (int64_t)ceil(cfg__.dt / dt_max__);                                          \
    (a).c.n_max = (int64_t)floor(cfg__.dt / cfg__.dt_min);                                     \
    (a).c.adaptive = cfg__.adaptive;                                                           \
    (a).c.fuse = cfg__.fuse;                                                                   \
    (a).c.multiplier = cfg__.multiplier;                                                       \
    (a).c.max_iters = cfg__.max_iters;                                                         \
    (a).n_parcel = (call).n_parcel;                                                            \
    (a).parcel_start = (call).parcel_start;                                                    \
    (a).v_cr = (call).v_cr;                                                                    \
    (a).mass_backup = (call).mass_backup;                                                      \
    (a).w_mid = (call).w_mid;                                                                  \
    (a).st = (call).state;                                                                     \
    (a).pr = (call).profile;                                                                   \
    (a).k0 = (call).k0;                                                                        \
    (a).k_count = (call).k_count;                                                              \
    (a).n_clamp_lo = cfg__.n_clamp_lo;                                                         \
    (a).n_clamp_hi = cfg__.n_clamp_hi;                                                         \
    (a).dt = cfg__.dt;                                                                         \
    (a).g_std = cfg__.g_std;                                                                   \
  } while (0)
#endif  // __HIPCC__

#endif  // SDM_PARCEL_SOLVER_H

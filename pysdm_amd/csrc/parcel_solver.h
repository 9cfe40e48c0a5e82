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
//
// The diagnostics (include/sdm_parcel_diag.h, where the arithmetic and the shape of the sums are
// written out): parcel_diagnose evaluates a request table for one parcel in one pass over its
// rows.  It runs in the step loop of `parcel_steps<P, true>` (k_parcel_d, k_parcel_f_d) after
// cs.write_back(), where every row's mass was last written by the lane that reads it here, and in
// k_parcel_diagnose(_f), the stage kernel.  parcel_steps<P, false> is the code it was before:
// k_parcel and k_parcel_f do not change.  Per lane the pass keeps one partial sum per request in
// registers (the solver's register cache is dead by then: cs.init() refills it every step); the
// 256 partials of four sums at a time meet in 8 KiB of LDS (strides 128 and 64 cross the waves),
// the strides from 32 down are wave shuffles in wave 0.  The spectrum is counted with 64-bit LDS
// atomics on 2 KiB, its edges sit beside them (2 KiB).  12.1 KiB of LDS beyond the solver's.
#ifndef SDM_PARCEL_SOLVER_H
#define SDM_PARCEL_SOLVER_H
#include "condensation_solver.h"
#include "physics.h"
#include "freezing_rows.h"
#include "deposition_rows.h"
#include "../../include/sdm_parcel_vent.h"
#include "../../include/sdm_parcel_ice.h"

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
  // sdm_parcel_run_diag: the table in device memory (nullptr: the kernels without diagnostics)
  const sdm_parcel_requests *requests;
  sdm_parcel_diag diag;
};
// one sdm_parcel_diagnose call (pointers are device pointers, `requests` included)
struct ParcelDiagnoseCall {
  int64_t n_parcel, n_sd;
  const int64_t *parcel_start, *multiplicity;
  const double *water_mass, *vdry, *kappa, *f_org, *T, *consts;
  const sdm_parcel_requests *requests;
  sdm_parcel_diag diag;
  // sdm_parcel_run_chem: parcels with failed_step[c] >= 0 are skipped (nullptr: none is)
  const int64_t *failed_step = nullptr;
};
// parcel.hip: the checks of sdm_parcel_run_diag and the ParcelCall of its arguments (k0 / k_count
// left to the caller); *with_diag: the request table is in device memory and `diag` has outputs.
// It synchronises the stream once (parcel_start is read back).  n_parcel or n_steps 0: SDM_OK with
// *nothing_to_do set.  `ventilated`: the caller is sdm_parcel_run_vent, the only entry that takes
// (and then demands) a ventilation other than Neglect
int sdm_parcel_prepare(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, int64_t n_steps, int64_t n_parcel,
                       int64_t n_sd, const int64_t *parcel_start, double *water_mass,
                       const int64_t *multiplicity, const double *vdry, const double *kappa,
                       const double *f_org, double *v_cr, const sdm_parcel_state *state,
                       const double *w_mid, const sdm_parcel_profile *profile,
                       const double consts[34], const sdm_cond_formulae *formulae,
                       const sdm_parcel_requests *requests, const sdm_parcel_diag *diag,
                       ParcelCall *call, bool *with_diag, bool *nothing_to_do,
                       bool ventilated = false);
// condensation.hip / condensation_formulae.hip: one launch of the default / general kernel
int sdm_parcel_launch_default(sdm_ctx *ctx, const ParcelCall &call);
int sdm_parcel_launch_general(sdm_ctx *ctx, const ParcelCall &call,
                              const sdm_cond_formulae *formulae);
// ... and of their siblings over a real permutation (include/sdm_parcel_coal.h: k_parcel_p,
// k_parcel_f_p): `call.identity` then holds the caller's permutation of global row numbers,
// `n_live` the live positions per parcel, and `dv` (n_parcel doubles) takes the step's dv
int sdm_parcel_launch_default_perm(sdm_ctx *ctx, const ParcelCall &call, const int64_t *n_live,
                                   double *dv);
int sdm_parcel_launch_general_perm(sdm_ctx *ctx, const ParcelCall &call,
                                   const sdm_cond_formulae *formulae, const int64_t *n_live,
                                   double *dv);
// condensation_formulae.hip: one launch of the ventilated kernel (include/sdm_parcel_vent.h;
// `vent` was checked by the caller)
int sdm_parcel_launch_vent(sdm_ctx *ctx, const ParcelCall &call,
                           const sdm_cond_formulae *formulae, const sdm_parcel_vent *vent);
int sdm_parcel_diagnose_default(sdm_ctx *ctx, const ParcelDiagnoseCall &call);
int sdm_parcel_diagnose_general(sdm_ctx *ctx, const ParcelDiagnoseCall &call,
                                const sdm_cond_formulae *formulae);
// the ice part of one sdm_parcel_run_ice call (include/sdm_parcel_ice.h; checked by the caller;
// the constants of a pass that is switched off may be nullptr)
struct ParcelIceCall {
  sdm_parcel_ice_cfg cfg;
  sdm_parcel_ice_state st;
  sdm_parcel_ice_profile pr;
  const double *frz_consts, *dep_consts;
};
// condensation.hip / condensation_formulae.hip: one launch of k_parcel_i / k_parcel_f_i
int sdm_parcel_launch_default_ice(sdm_ctx *ctx, const ParcelCall &call, const ParcelIceCall &ice);
int sdm_parcel_launch_general_ice(sdm_ctx *ctx, const ParcelCall &call,
                                  const sdm_cond_formulae *formulae, const ParcelIceCall &ice);

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

// what the kernels with diagnostics take beside ParcelArgs<P>
struct ParcelDiag {
  const sdm_parcel_requests *req;  // device memory
  sdm_parcel_diag out;
};

template <class P>
struct ParcelDiagnoseArgs {
  typename P::K k;
  int64_t n_parcel, n_sd;
  const int64_t *parcel_start, *multiplicity;
  const double *water_mass, *vdry, *kappa, *T;
  ParcelDiag d;
  const int64_t *failed_step;
};

#define DIAG_ROUND 4  // sums reduced at a time: moment_0 and moments of two requests

// the LDS of one workgroup's diagnostics (declared where this is inlined: once per kernel)
struct DiagLds {
  double *red;               // DIAG_ROUND x COND_CB partials
  unsigned long long *bins;  // SDM_PARCEL_MAX_BINS counts
  double *edges;             // SDM_PARCEL_MAX_BINS + 1
};
DF void attach_diag_lds(DiagLds &l) {
  __shared__ double s_red[DIAG_ROUND * COND_CB];
  __shared__ unsigned long long s_bins[SDM_PARCEL_MAX_BINS];
  __shared__ double s_edges[SDM_PARCEL_MAX_BINS + 1];
  l.red = s_red;
  l.bins = s_bins;
  l.edges = s_edges;
}

DF double diag_power(double x, double rank) {
  return rank == 0 ? 1.0 : (rank == 1 ? x : sdm_pow(x, rank));
}

// include/sdm_parcel_diag.h for one parcel: rows row0 .. row0 + n at temperature T; out_* point at
// the parcel's row of the outputs (or are nullptr).  Every lane of the workgroup calls it; the
// table was checked on the host (counts within the maxima, enums known).
template <class P>
DF void parcel_diagnose(const typename P::K &k, const sdm_parcel_requests *rq, const DiagLds &l,
                        int64_t row0, int64_t n, double T, const double *water_mass,
                        const int64_t *multiplicity, const double *vdry, const double *kappa,
                        double *out_m0, double *out_m, double *out_spectrum, int tid) {
  const int nm = rq->n_moments, nb = rq->n_bins, bin_attr = rq->bin_attr;
  bool need_r = false, need_rd = false;  // the derived attributes some request reads (uniform)
  bool need_ratio = nb > 0 && bin_attr == SDM_PARCEL_FILTER_VOLUME_RATIO;
  for (int i = 0; i < nm; ++i) {
    need_r = need_r || rq->moment[i].attr == SDM_PARCEL_ATTR_RADIUS;
    need_rd = need_rd || rq->moment[i].attr == SDM_PARCEL_ATTR_DRY_RADIUS;
    need_ratio = need_ratio || rq->moment[i].filter_attr == SDM_PARCEL_FILTER_VOLUME_RATIO;
  }
  __syncthreads();  // the previous evaluation's reads of this LDS are over; lane 0's T is in LDS
  for (int b = tid; b < nb; b += COND_CB) l.bins[b] = 0;
  for (int b = tid; b <= nb; b += COND_CB) l.edges[b] = rq->edges[b];
  __syncthreads();
  const double rho_w = P::rho_w(k), inv_pi_4_3 = 1 / P::pi_4_3(k);
  double acc_0[SDM_PARCEL_MAX_MOMENTS], acc_m[SDM_PARCEL_MAX_MOMENTS];
#pragma unroll
  for (int u = 0; u < SDM_PARCEL_MAX_MOMENTS; ++u) acc_0[u] = acc_m[u] = 0.0;
  for (int64_t q = tid; q < n; q += COND_CB) {
    const int64_t row = row0 + q;
    const int64_t mult = multiplicity[row];
    const double m = water_mass[row], vd = vdry[row], nn = (double)mult;
    const double v = volume_of_mass(m, rho_w);
    const double r = need_r ? radius_of_volume(v, inv_pi_4_3) : 0.0;
    const double rd = need_rd ? radius_of_volume(vd, inv_pi_4_3) : 0.0;
    const double ratio = need_ratio ? v / P::critical_volume(k, row, kappa[row], vd, v, T) : 0.0;
    const double filters[SDM_PARCEL_N_FILTERS] = {m, v, vd, ratio};
    const double attrs[SDM_PARCEL_N_ATTRS] = {m, v, r, vd, rd};
#pragma unroll 1
    for (int i = 0; i < nm; ++i) {
      const sdm_parcel_moment_request &mr = rq->moment[i];
      double f = filters[0], x = attrs[0];
#pragma unroll
      for (int u = 1; u < SDM_PARCEL_N_FILTERS; ++u) f = mr.filter_attr == u ? filters[u] : f;
#pragma unroll
      for (int u = 1; u < SDM_PARCEL_N_ATTRS; ++u) x = mr.attr == u ? attrs[u] : x;
      if (mr.min_x <= f && f < mr.max_x) {
        const double term = nn * diag_power(x, mr.rank);
#pragma unroll
        for (int u = 0; u < SDM_PARCEL_MAX_MOMENTS; ++u) {
          acc_0[u] = u == i ? acc_0[u] + nn : acc_0[u];
          acc_m[u] = u == i ? acc_m[u] + term : acc_m[u];
        }
      }
    }
    if (nb > 0) {
      double f = filters[0];
#pragma unroll
      for (int u = 1; u < SDM_PARCEL_N_FILTERS; ++u) f = bin_attr == u ? filters[u] : f;
      if (l.edges[0] <= f && f < l.edges[nb]) {
        int lo = 0, hi = nb;  // edges[lo] <= f < edges[hi]
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (l.edges[mid] <= f) lo = mid;
          else hi = mid;
        }
        atomicAdd(&l.bins[lo], (unsigned long long)mult);
      }
    }
  }
#pragma unroll
  for (int r0 = 0; r0 < SDM_PARCEL_MAX_MOMENTS; r0 += DIAG_ROUND / 2) {
    if (r0 >= nm) break;  // (uniform)
    if (r0 > 0) __syncthreads();  // wave 0 has read the previous round
#pragma unroll
    for (int u = 0; u < DIAG_ROUND / 2; ++u) {
      l.red[(2 * u) * COND_CB + tid] = acc_0[r0 + u];
      l.red[(2 * u + 1) * COND_CB + tid] = acc_m[r0 + u];
    }
    __syncthreads();
    if (tid < 64) {
#pragma unroll
      for (int u = 0; u < DIAG_ROUND / 2; ++u) {
        double s[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double *p = l.red + (2 * u + h) * COND_CB + tid;
          double part = (p[0] + p[128]) + (p[64] + p[192]);  // strides 128, then 64
#pragma unroll
          for (int stride = 32; stride >= 1; stride >>= 1) part += __shfl_down(part, stride, 64);
          s[h] = part;
        }
        const int i = r0 + u;
        if (tid == 0 && i < nm) {
          if (out_m0) out_m0[i] = s[0];
          if (out_m)
            out_m[i] = rq->moment[i].skip_division_by_m0 ? s[1] : (s[0] != 0 ? s[1] / s[0] : 0.0);
        }
      }
    }
  }
  __syncthreads();  // every lane's atomics on the bins are done
  if (out_spectrum)
    for (int b = tid; b < nb; b += COND_CB) out_spectrum[b] = (double)l.bins[b];
}

// the stage kernel of sdm_parcel_diagnose: one workgroup per parcel, striding
template <class P>
DF void parcel_diagnose_cells(const ParcelDiagnoseArgs<P> &a) {
  DiagLds l;
  attach_diag_lds(l);
  const int nm = a.d.req->n_moments, nb = a.d.req->n_bins;
  for (int64_t c = blockIdx.x; c < a.n_parcel; c += gridDim.x) {
    const int64_t row0 = a.parcel_start[c], n = a.parcel_start[c + 1] - row0;
    if (row0 < 0 || n <= 0 || row0 + n > a.n_sd) continue;  // (checked on the host too)
    if (a.failed_step && a.failed_step[c] >= 0) continue;   // (uniform over the workgroup)
    parcel_diagnose<P>(a.k, a.d.req, l, row0, n, a.T[c], a.water_mass, a.multiplicity, a.vdry,
                       a.kappa, a.d.out.moment_0 ? a.d.out.moment_0 + c * nm : nullptr,
                       a.d.out.moments ? a.d.out.moments + c * nm : nullptr,
                       a.d.out.spectrum ? a.d.out.spectrum + c * nb : nullptr,
                       (int)threadIdx.x);
  }
}

// the slots of the parcel's scalars in LDS
enum { PS_Z, PS_RHOD, PS_THD, PS_QV, PS_T, PS_P, PS_RH, PS_QV_PREV, PS_PRHOD, PS_PZ, PS_N };

// ---- ventilation (include/sdm_parcel_vent.h) -------------------------------------------------
// parcel_steps<P, DIAG, true> (k_parcel_v, k_parcel_v_d) forms every row's Reynolds number in the
// pass that forms its critical volume: radius, fall velocity and Re by the device functions the
// stage kernels run (physics.h), written to the `reynolds_number` column the solver's policy reads
// back - row q by lane q % COND_CB on both sides, so program order is all the ordering.  The
// parcel's air density and viscosity live in LDS beside s_par: the pair the step reads, and the
// pair lane 0 forms after the advance, which replaces the first only when the step has succeeded.
// The policy's cellwide() finds the first pair through vent_lds() (a function-scope __shared__
// object is one object however often the function is inlined).
struct ParcelVent {  // == sdm_parcel_vent
  int32_t law, terms;
  const double *params, *gk_a, *gk_b;
  int64_t gk_len;
  double gk_factor, gk_top;
  double *air_density, *air_dynamic_viscosity, *reynolds_number;
  int64_t *out_of_table;
};
enum { PA_RHO, PA_ETA, PA_NEW_RHO, PA_NEW_ETA, PA_N };
struct VentLds {
  double air[PA_N];
  int out_of_range;
};
DF VentLds *vent_lds() {
  __shared__ VentLds s_vent;
  return &s_vent;
}
// the law is uniform over the launch; each branch is the device function of its stage kernel
DF double vent_velocity(const ParcelVent &v, double r) {
  if (v.law == SDM_VELOCITY_LAW_GUNN_KINZER)
    return gk_interpolate(r, v.gk_factor, v.gk_a, v.gk_b, v.gk_len);
  if (v.law == SDM_VELOCITY_LAW_ROGERS_YAU) return rogers_yau_velocity(r, v.params);
  return power_series_velocity(r, v.terms, v.params, v.params + v.terms);
}

// ---- a real permutation (include/sdm_parcel_coal.h) ---------------------------------------------
// parcel_steps<P, false, false, true> (k_parcel_p, k_parcel_f_p) carries the step out over the
// parcel's LIVE rows in the order of its permutation: position q of the parcel is row
// idx[parcel_start[c] + q] (a global row number, as the identity's entries are), q < n_live[c].
// The solver always went through `cidx`; here the row loops around it do too.  Rows that are not
// live are neither read nor written.  The step's dv goes to `dv[c]` for the collision kernel that
// follows in the stream.
struct ParcelPerm {
  const int64_t *n_live;
  double *dv;
};

// the jump by `delta` draws of the LCG with increment `inc` as an affine map: state * m + p (every
// parcel has its own PCG64 increment, so the context's jump table - one increment - does not apply)
struct PcgAff { u128 m, p; };
__device__ __forceinline__ PcgAff pcg_affine(u128 inc, uint64_t delta) {
  u128 acc_mult = 1, acc_plus = 0, cur_mult = pcg_mult(), cur_plus = inc;
  while (delta) {
    if (delta & 1) {
      acc_mult *= cur_mult;
      acc_plus = acc_plus * cur_mult + cur_plus;
    }
    cur_plus = (cur_mult + 1) * cur_plus;
    cur_mult *= cur_mult;
    delta >>= 1;
  }
  return {acc_mult, acc_plus};
}

// ---- ice (include/sdm_parcel_ice.h) ---------------------------------------------------------------
// parcel_steps<P, false, false, false, true> (k_parcel_i, k_parcel_f_i) runs the freezing and
// deposition passes in the step loop after cs.write_back() and before lane 0 overwrites s_par, so
// the ascent stays one launch per steps_per_launch steps.  The row arithmetic is the text the stage
// kernels compile (freezing_rows.h, deposition_rows.h).  What depends on the parcel only - the two
// nucleation rates and the deposition's cell record - is formed once per parcel and step by lane 0
// into LDS.  Position q of the parcel belongs to lane q % COND_CB in both passes, as in the solver:
// a row is read once, carried through the passes in the order the call names and stored if it
// changed.  The deposition's two sums ride the solver's LDS column, ICE_CH positions at a time
// (first half dq, second half dth, a byte per position telling whether the row contributes), and
// lane 0 adds them up in position order: serially (ORDERED, the reference's bits), or block by
// block in the header's fixed tree shape (BLOCKED), carried out by lane 0 alone so that blocks may
// span chunks.  The uniforms are the parcel's own PCG64 stream: a lane jumps to its first position
// once per step (pcg_affine) and from there by COND_CB.  The carried pair (a_w_ice, RH_ice), the
// stream position and the count of exceeded rows live in LDS between the steps; a failed step
// leaves them as they were.
#define ICE_CH (COND_CH / 2)
struct ParcelIce {
  int freezing, deposition, dep_first;
  int imm_singular, imm_time_dependent, hom, thaw, j_het, j_hom, blocked;
  sdm_parcel_ice_state st;
  sdm_parcel_ice_profile pr;
  Kf kf;
  DepArgs dep;  // what dep_cell_record and dep_row read: k, coordinate, capacity, kinetics, dt
};
enum { PI_A_W_ICE, PI_RH_ICE, PI_NEW_A_W_ICE, PI_NEW_RH_ICE, PI_N };
struct IceLds {
  double pair[PI_N];
  double T, p, RH;  // the current values, where the rate functions find them
  double rate[2];   // immersion, homogeneous
  double cv[DEP_CV];
  double blk[2][SDM_DEP_SUM_BLOCK];
  unsigned long long offset, n_exceeded, n_exceeded_step, n_ice;
  unsigned char contributes[ICE_CH];
};
DF IceLds *ice_lds() {
  __shared__ IceLds s_ice;
  return &s_ice;
}

// the header's block reduction, by one lane
DF double ice_block_sum(double *a, int len) {
  for (int h = SDM_DEP_SUM_BLOCK / 2; h >= 1; h /= 2)
    for (int j = 0; j < h; ++j)
      if (j + h < len) a[j] += a[j + h];
  return a[0];
}

// sdm_freezing_step for one row of a parcel (n_cell = 1, volume = NULL): the enabled passes in the
// stage sequence's order, then the record of the temperature of last freezing; returns the mass.
// `u_imm`, `u_hom`: the row's uniforms of the two stochastic passes
DF double ice_freeze_row(const ParcelIce &ic, const IceLds *il, double m, int64_t row, double T,
                         double RH, double dt, double u_imm, double u_hom) {
  const int thaw = ic.thaw;
  const double T0 = ic.kf.T0;
  double mass = m;
  if (ic.imm_singular) {
    double x = mass;
    if (freeze_singular_row(x, ic.st.freezing_temperature[row], T, RH, thaw, T0)) mass = x;
  }
  if (ic.imm_time_dependent) {
    double x = mass;
    if (freeze_time_dependent_row(x, ic.st.immersed_surface_area[row], T, il->rate[0], dt, u_imm,
                                  thaw, T0))
      mass = x;
  }
  if (ic.hom) {
    double x = mass;
    if (freeze_homogeneous_row(x, liquid_volume_of(ic.kf, mass), T, il->rate[1], dt, u_hom, thaw,
                               T0))
      mass = x;
  }
  if (ic.st.temperature_of_last_freezing) {
    double data = ic.st.temperature_of_last_freezing[row];
    if (record_one(data, mass, T)) ic.st.temperature_of_last_freezing[row] = data;
  }
  return mass;
}

// point 5 of the header for one parcel and step, and the sums of point 7.  Every lane of the
// workgroup calls it; `pqv`, `pthd` (in: the solver's, out: with the deposition's additions),
// `n_ice` and `ice_mass` are lane 0's.
template <class P>
DF void parcel_ice_passes(const ParcelIce &ic, IceLds *il, const CondArgs<P> &g, double *col,
                          int64_t row0, int64_t n, int64_t c, int tid, double T, double p,
                          double RH, double qv, double rhod, double thd, double dv, double dt,
                          double &pqv, double &pthd, int64_t &n_ice, double &ice_mass) {
  const bool stochastic = ic.freezing && (ic.imm_time_dependent || ic.hom);
  if (tid == 0) {
    il->T = T;
    il->p = p;
    il->RH = RH;
    if (ic.freezing && ic.imm_time_dependent)
      il->rate[0] = het_rate_of_cell(ic.kf, ic.j_het, &il->RH, &il->pair[PI_A_W_ICE], 0);
    if (ic.freezing && ic.hom)
      il->rate[1] = hom_rate_of_cell(ic.kf, ic.j_hom, &il->T, &il->pair[PI_RH_ICE],
                                     &il->pair[PI_A_W_ICE], 0);
    if (ic.deposition)
      dep_cell_record(ic.dep, dv, T, p, RH, il->pair[PI_A_W_ICE], qv, rhod, thd, il->cv);
    il->n_exceeded_step = 0;
    il->n_ice = 0;
  }
  __syncthreads();
  // the lane's generator at its first position of each stochastic pass
  u128 st_imm = 0, st_hom = 0, inc = 0;
  PcgAff over = {1, 0};
  if (stochastic) {
    const uint64_t *w = ic.st.rng_state_inc + 4 * c;
    const u128 base = (((u128)w[0]) << 64) | w[1];
    inc = (((u128)w[2]) << 64) | w[3];
    const uint64_t off = (uint64_t)il->offset;
    over = pcg_affine(inc, (uint64_t)COND_CB);
    const PcgAff first = pcg_affine(inc, off + (uint64_t)tid);
    st_imm = st_hom = base * first.m + first.p;
    if (ic.imm_time_dependent && ic.hom) {
      const PcgAff second = pcg_affine(inc, off + (uint64_t)n + (uint64_t)tid);
      st_hom = base * second.m + second.p;
    }
  }
  double accq = pqv, acct = pthd;  // (lane 0's)
  int filled = 0;                  // entries of the open block (lane 0's, BLOCKED)
  unsigned long long exceeded = 0, ice_count = 0;
  double ice_part = 0.0;
  for (int64_t base = 0; base < n; base += ICE_CH) {
    const int len = (int)(n - base < ICE_CH ? n - base : ICE_CH);
#pragma unroll
    for (int s = 0; s < ICE_CH / COND_CB; ++s) {
      const int slot = tid + s * COND_CB;
      const int64_t q = base + slot;
      double u_imm = 0, u_hom = 0;
      if (stochastic) {  // (every lane advances by COND_CB positions, rows or not)
        if (ic.imm_time_dependent) {
          u_imm = pcg_output(st_imm * pcg_mult() + inc);
          st_imm = st_imm * over.m + over.p;
        }
        if (ic.hom) {
          u_hom = pcg_output(st_hom * pcg_mult() + inc);
          st_hom = st_hom * over.m + over.p;
        }
      }
      double dq = 0.0, dth = 0.0;
      bool contributes = false;
      if (q < n) {
        const int64_t row = row0 + q;
        const int64_t mult = g.multiplicity[row];
        const double m_read = g.water_mass[row];
        double m = m_read;
        if (ic.freezing && !ic.dep_first)
          m = ice_freeze_row(ic, il, m, row, T, RH, dt, u_imm, u_hom);
        // sdm_deposition for one row (dm.py:42 `not unfrozen`: m > 0 is liquid; :79-80)
        if (ic.deposition && !(m > 0) && !(il->cv[CV_S] == 1)) {
          double m_new;
          exceeded += dep_row(ic.dep, il->cv, m, mult, &m_new, &dq, &dth) ? 1 : 0;
          m = m_new;
          contributes = true;
        }
        if (ic.freezing && ic.dep_first)
          m = ice_freeze_row(ic, il, m, row, T, RH, dt, u_imm, u_hom);
        // (rows that do not change are not stored; a row the deposition evaluated is)
        if (contributes || m != m_read) g.water_mass[row] = m;
        if (m < 0) {
          ice_count += (unsigned long long)mult;
          ice_part += (double)mult * (-m);
        }
      }
      col[slot] = dq;
      col[ICE_CH + slot] = dth;
      il->contributes[slot] = contributes ? 1 : 0;
    }
    if (ic.deposition) {  // (uniform)
      __syncthreads();
      if (tid == 0) {
        for (int j = 0; j < len; ++j) {
          if (!il->contributes[j]) continue;
          if (!ic.blocked) {
            accq += col[j];
            acct += col[ICE_CH + j];
            continue;
          }
          il->blk[0][filled] = col[j];
          il->blk[1][filled] = col[ICE_CH + j];
          if (++filled == SDM_DEP_SUM_BLOCK) {
            accq += ice_block_sum(il->blk[0], filled);
            acct += ice_block_sum(il->blk[1], filled);
            filled = 0;
          }
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0 && filled > 0) {
    accq += ice_block_sum(il->blk[0], filled);
    acct += ice_block_sum(il->blk[1], filled);
  }
  // the SUM of sdm_parcel_diag.h of the lanes' partials; the two counts
  if (exceeded) atomicAdd(&il->n_exceeded_step, exceeded);
  if (ice_count) atomicAdd(&il->n_ice, ice_count);
  col[tid] = ice_part;
  __syncthreads();
  if (tid < 64) {
    const double *part = col + tid;
    double sum = (part[0] + part[128]) + (part[64] + part[192]);  // strides 128, then 64
#pragma unroll
    for (int stride = 32; stride >= 1; stride >>= 1) sum += __shfl_down(sum, stride, 64);
    if (tid == 0) {
      ice_mass = sum;
      n_ice = (int64_t)il->n_ice;
      pqv = accq;
      pthd = acct;
      il->n_exceeded += il->n_exceeded_step;
      if (stochastic)
        il->offset += (unsigned long long)n * (unsigned long long)((ic.imm_time_dependent ? 1 : 0) +
                                                                   (ic.hom ? 1 : 0));
    }
  }
}

template <class P, bool DIAG = false, bool VENT = false, bool PERM = false, bool ICE = false>
DF void parcel_steps(const ParcelArgs<P> &a, const ParcelDiag *d = nullptr,
                     const ParcelVent *v = nullptr, const ParcelPerm *pp = nullptr,
                     const ParcelIce *ic = nullptr) {
  __shared__ double s_par[PS_N];
  __shared__ int64_t s_nsub;
  DiagLds dl;
  if constexpr (DIAG) attach_diag_lds(dl);
  [[maybe_unused]] VentLds *vl = nullptr;
  if constexpr (VENT) vl = vent_lds();
  [[maybe_unused]] IceLds *il = nullptr;
  if constexpr (ICE) il = ice_lds();
  const CondArgs<P> &g = a.c;
  const typename P::K &k = g.k;
  const int tid = (int)threadIdx.x;
  for (int64_t c = blockIdx.x; c < a.n_parcel; c += gridDim.x) {
    const int64_t row0 = a.parcel_start[c];
    int64_t n = a.parcel_start[c + 1] - row0;
    // (checked on the host too; failed parcels are skipped for good)
    if (row0 < 0 || n <= 0 || row0 + n > g.n_sd || a.st.failed_step[c] >= 0) continue;
    if constexpr (PERM) {  // the live positions (uniform over the workgroup)
      const int64_t live = pp->n_live[c];
      if (live <= 0 || live > n) continue;
      n = live;
    }
    // the row at position q of the parcel (PERM: a word the host has checked, checked again here)
    auto row_at = [&](int64_t q) -> int64_t {
      if constexpr (PERM) {
        const int64_t row = g.idx[row0 + q];
        return row >= 0 && row < g.n_sd ? row : -1;
      } else {
        return row0 + q;
      }
    };
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
      if constexpr (VENT) {
        vl->air[PA_RHO] = v->air_density[c];
        vl->air[PA_ETA] = v->air_dynamic_viscosity[c];
        vl->out_of_range = 0;
      }
      if constexpr (ICE) {
        il->pair[PI_A_W_ICE] = ic->st.a_w_ice[c];
        il->pair[PI_RH_ICE] = ic->st.RH_ice[c];
        il->offset = ic->st.rng_offset ? ic->st.rng_offset[c] : 0;
        il->n_exceeded = 0;
      }
    }
    const double mass_of_dry_air = a.st.mass_of_dry_air[c];
    int64_t done = a.st.steps_done[c];
    int64_t failed = -1;
    [[maybe_unused]] bool out_of_table = false;
    for (int64_t j = 0; j < a.k_count; ++j) {
      __syncthreads();  // lane 0's state of the previous step (or the load above) is in LDS
      const double thd = s_par[PS_THD], qv = s_par[PS_QV], rhod = s_par[PS_RHOD];
      const double T = s_par[PS_T];
      [[maybe_unused]] double air_rho = 0, air_eta = 0;  // the pair this step's Re reads
      if constexpr (VENT) {
        air_rho = vl->air[PA_RHO];
        air_eta = vl->air[PA_ETA];
      }
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
        if constexpr (PERM)
          if (tid == 0) pp->dv[c] = dv;
        if (tid == 0) {
          s_par[PS_PZ] = s_par[PS_Z] + a.dt * w;  // (lane 0 alone reads these two again)
          s_par[PS_PRHOD] = prhod;
        }
      }
      if constexpr (VENT) {
        // Moist.sync of this step (moist.py:73-100): the pair the NEXT step reads, from the
        // advanced rhod and the thd and qv of before this step's condensation
        if (tid == 0) {
          double sync_T, sync_p, sync_RH;
          P::tprh(k, prhod, thd, qv, sync_T, sync_p, sync_RH);
          vl->air[PA_NEW_RHO] = air_density_of(prhod, qv);
          vl->air[PA_NEW_ETA] = P::air_dynamic_viscosity(k, sync_T);
        }
        // the table's range, before anything of the step is written
        if (v->law == SDM_VELOCITY_LAW_GUNN_KINZER) {  // (uniform)
          const double inv_pi_4_3 = 1 / P::pi_4_3(k);
          bool over = false;
          for (int64_t q = tid; q < n; q += COND_CB) {
            const int64_t row = row_at(q);
            if (PERM && row < 0) continue;
            over = over || radius_of_volume(volume_of_mass(g.water_mass[row], P::rho_w(k)),
                                            inv_pi_4_3) > v->gk_top;
          }
          if (over) vl->out_of_range = 1;
          __syncthreads();
          if (vl->out_of_range) {  // uniform; lane 0 clears the flag when it loads the next parcel
            failed = done;
            out_of_table = true;
            break;
          }
        }
      }
      if constexpr (ICE) {
        // Moist.sync of this step (moist.py:73-100): the pair the NEXT step's ice passes read, from
        // the advanced rhod and the thd and qv of before this step's condensation
        if (tid == 0) {
          double sync_T, sync_p, sync_RH;
          P::tprh(k, prhod, thd, qv, sync_T, sync_p, sync_RH);
          a_w_ice_of(ic->kf, sync_T, sync_p, sync_RH, qv, il->pair[PI_NEW_A_W_ICE],
                     il->pair[PI_NEW_RH_ICE]);
        }
      }
      // the critical volume of every row at the parcel's temperature (ICE: of every liquid row);
      // the copy of the masses the solver writes in place
      for (int64_t q = tid; q < n; q += COND_CB) {
        const int64_t row = row_at(q);
        if (PERM && row < 0) continue;
        const double m = g.water_mass[row];
        if (!ICE || m > 0)
          a.v_cr[row] = P::critical_volume(k, row, g.kappa[row], g.vdry[row], m / P::rho_w(k), T);
        if (q >= COND_CH) a.mass_backup[row] = m;
        if constexpr (VENT) {  // attributes/physics/reynolds_number.py of the mass before the step
          const double r = radius_of_volume(volume_of_mass(m, P::rho_w(k)), 1 / P::pi_4_3(k));
          v->reynolds_number[row] = reynolds_number_of(r, vent_velocity(*v, r), air_rho, air_eta);
        }
      }
      cs.init();
      const SolveOut s = solve_cell<P>(cs, g, thd, qv, rhod, prhod, thd, qv, dv, s_nsub);
      if (!s.o.success) {  // uniform: the solver's results come from LDS after a barrier
        for (int64_t q = COND_CH + tid; q < n; q += COND_CB) {
          const int64_t row = row_at(q);
          if (PERM && row < 0) continue;
          g.water_mass[row] = a.mass_backup[row];
        }
        failed = done;
        break;
      }
      cs.write_back();
      done += 1;
      double pthd = s.o.thd, pqv = s.o.qv;  // (with the deposition's additions: lane 0's)
      [[maybe_unused]] int64_t n_ice = 0;
      [[maybe_unused]] double ice_mass = 0;
      [[maybe_unused]] double nT_ice = 0, np_ice = 0, nRH_ice = 0;
      if constexpr (ICE) {
        // T, p, RH of the state after the condensation alone: the deposition leaves them stale
        // (include/sdm_parcel_ice.h, point 6)
        if (tid == 0) P::tprh(k, prhod, pthd, pqv, nT_ice, np_ice, nRH_ice);
        // the passes read the state of before the step: every lane's p and RH before lane 0
        // overwrites s_par (the passes end with barriers)
        parcel_ice_passes<P>(*ic, il, g, cs.col, row0, n, c, tid, T, s_par[PS_P], s_par[PS_RH], qv,
                             rhod, thd, dv, a.dt, pqv, pthd, n_ice, ice_mass);
      }
      if (tid == 0) {
        const double new_rhod = s_par[PS_PRHOD];
        double nT, np, nRH;
        if constexpr (ICE) {
          nT = nT_ice;
          np = np_ice;
          nRH = nRH_ice;
        } else {
          P::tprh(k, new_rhod, pthd, pqv, nT, np, nRH);
        }
        int64_t ns = s.n;
        if (g.adaptive) {  // dynamics/condensation.py:122-131
          ns = ns > a.n_clamp_lo ? ns : a.n_clamp_lo;
          ns = ns < a.n_clamp_hi ? ns : a.n_clamp_hi;
        }
        s_par[PS_QV_PREV] = s_par[PS_QV];
        s_par[PS_Z] = s_par[PS_PZ];
        s_par[PS_RHOD] = new_rhod;
        s_par[PS_THD] = pthd;
        s_par[PS_QV] = pqv;
        s_par[PS_T] = nT;
        s_par[PS_P] = np;
        s_par[PS_RH] = nRH;
        s_nsub = ns;
        if constexpr (VENT) {  // (every lane's reads of the old pair ended before the solver's
          vl->air[PA_RHO] = vl->air[PA_NEW_RHO];  // last barrier)
          vl->air[PA_ETA] = vl->air[PA_NEW_ETA];
        }
        // the counters and RH_max are not read by the next step: straight to the state arrays
        a.st.n_activating[c] = s.o.n_activating;
        a.st.n_deactivating[c] = s.o.n_deactivating;
        a.st.n_ripening[c] = s.o.n_ripening;
        a.st.RH_max[c] = s.o.RH_max;
        const int64_t at = (a.k0 + j) * a.n_parcel + c;
        if (a.pr.z) a.pr.z[at] = s_par[PS_Z];
        if (a.pr.rhod) a.pr.rhod[at] = new_rhod;
        if (a.pr.thd) a.pr.thd[at] = pthd;
        if (a.pr.qv) a.pr.qv[at] = pqv;
        if constexpr (ICE) {
          il->pair[PI_A_W_ICE] = il->pair[PI_NEW_A_W_ICE];
          il->pair[PI_RH_ICE] = il->pair[PI_NEW_RH_ICE];
          if (ic->pr.a_w_ice) ic->pr.a_w_ice[at] = il->pair[PI_A_W_ICE];
          if (ic->pr.RH_ice) ic->pr.RH_ice[at] = il->pair[PI_RH_ICE];
          if (ic->pr.n_ice) ic->pr.n_ice[at] = n_ice;
          if (ic->pr.ice_mass) ic->pr.ice_mass[at] = ice_mass;
          if (ic->pr.n_exceeded) ic->pr.n_exceeded[at] = (int64_t)il->n_exceeded_step;
          if (ic->pr.dv) ic->pr.dv[at] = dv;
        }
        if (a.pr.T) a.pr.T[at] = nT;
        if (a.pr.p) a.pr.p[at] = np;
        if (a.pr.RH) a.pr.RH[at] = nRH;
        if (a.pr.RH_max) a.pr.RH_max[at] = s.o.RH_max;
        if (a.pr.n_substeps) a.pr.n_substeps[at] = ns;
        if (a.pr.n_activating) a.pr.n_activating[at] = s.o.n_activating;
        if (a.pr.n_deactivating) a.pr.n_deactivating[at] = s.o.n_deactivating;
        if (a.pr.n_ripening) a.pr.n_ripening[at] = s.o.n_ripening;
      }
      if constexpr (DIAG) {  // the products of the state after the step, at its temperature
        const int64_t at = (a.k0 + j) * a.n_parcel + c;
        const int nm = d->req->n_moments, nb = d->req->n_bins;
        if (tid == 0 && d->out.dv) d->out.dv[at] = dv;
        __syncthreads();  // lane 0's new T is in LDS
        parcel_diagnose<P>(k, d->req, dl, row0, n, s_par[PS_T], g.water_mass, g.multiplicity,
                           g.vdry, g.kappa, d->out.moment_0 ? d->out.moment_0 + at * nm : nullptr,
                           d->out.moments ? d->out.moments + at * nm : nullptr,
                           d->out.spectrum ? d->out.spectrum + at * nb : nullptr, tid);
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
      if constexpr (VENT) {  // (a failed step left the pair as it was)
        v->air_density[c] = vl->air[PA_RHO];
        v->air_dynamic_viscosity[c] = vl->air[PA_ETA];
        if (out_of_table && v->out_of_table) v->out_of_table[c] = 1;
      }
      if constexpr (ICE) {  // (a failed step left all of it as it was)
        ic->st.a_w_ice[c] = il->pair[PI_A_W_ICE];
        ic->st.RH_ice[c] = il->pair[PI_RH_ICE];
        if (ic->st.rng_offset) ic->st.rng_offset[c] = (uint64_t)il->offset;
        ic->st.n_exceeded[c] += (int64_t)il->n_exceeded;
      }
    }
  }
}

// what both ice launchers do with a ParcelIceCall: the kernels' ParcelIce
inline ParcelIce parcel_ice_of(const ParcelIceCall &ice, double dt) {
  ParcelIce ic;
  memset(&ic, 0, sizeof(ic));
  const sdm_parcel_ice_cfg &cfg = ice.cfg;
  ic.freezing = cfg.freezing != 0;
  ic.deposition = cfg.deposition != 0;
  ic.dep_first = cfg.order == SDM_PARCEL_ICE_DEPOSITION_FIRST;
  ic.imm_singular = cfg.immersion_freezing && cfg.singular;
  ic.imm_time_dependent = cfg.immersion_freezing && !cfg.singular;
  ic.hom = cfg.homogeneous_freezing != 0;
  ic.thaw = cfg.thaw != 0;
  ic.j_het = cfg.j_het;
  ic.j_hom = cfg.j_hom;
  ic.blocked = cfg.sum == SDM_DEP_SUM_BLOCKED;
  ic.st = ice.st;
  ic.pr = ice.pr;
  // (Moist.sync's a_w_ice reads T0, eps and the ice saturation polynomial of the freezing
  // constants also where only the deposition is switched on)
  ic.kf = frz_consts_of(ice.frz_consts);
  if (ic.deposition) ic.dep.k = dep_consts_of(ice.dep_consts);
  ic.dep.coordinate = cfg.coordinate;
  ic.dep.capacity = cfg.capacity;
  ic.dep.kinetics = cfg.kinetics;
  ic.dep.dt = dt;
  return ic;
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

// the fields of ParcelDiagnoseArgs<P> but `k`
#define SDM_PARCEL_FILL_DIAGNOSE_ARGS(a, call) \
  do {                                         \
    (a).n_parcel = (call).n_parcel;            \
    (a).n_sd = (call).n_sd;                    \
    (a).parcel_start = (call).parcel_start;    \
    (a).multiplicity = (call).multiplicity;    \
    (a).water_mass = (call).water_mass;        \
    (a).vdry = (call).vdry;                    \
    (a).kappa = (call).kappa;                  \
    (a).T = (call).T;                          \
    (a).d.req = (call).requests;               \
    (a).d.out = (call).diag;                   \
    (a).failed_step = (call).failed_step;      \
  } while (0)
#endif  // __HIPCC__

#endif  // SDM_PARCEL_SOLVER_H

// parcel.hip -- the entry point of include/sdm_parcel.h: argument checks, the two buffers the
// kernels need beyond the caller's arrays, and the chunking of a call into launches.  The kernels
// are the instantiations of parcel_solver.h (where their design is described) next to those of the
// condensation solver: k_parcel in condensation.hip (PySDM's default formulae), k_parcel_f in
// condensation_formulae.hip (a descriptor); this file reaches both through their launchers.
// Likewise include/sdm_parcel_diag.h: its request table is checked here and copied to device
// memory once per call; k_parcel_d / k_parcel_f_d and k_parcel_diagnose(_f) read it there.
// And include/sdm_parcel_vent.h: the same checks and chunking for formulae with a ventilation, on
// k_parcel_v / k_parcel_v_d (condensation_formulae.hip).
// And include/sdm_parcel_ice.h: the mixed-phase parcel, on k_parcel_i / k_parcel_f_i.
//
// A call of n_steps enqueues ceil(n_steps / steps_per_launch) launches back to back on the
// context's stream, without synchronising between them: one launch stays short on a shared card,
// and nothing but the stream orders them (launch k + 1 reads the state arrays launch k wrote).
#include <vector>

#include "parcel_solver.h"

namespace {

// the identity permutation (written once per growth) and the backup column, n_sd entries each
int reserve_rows(sdm_ctx *ctx, int64_t n_sd) {
  if (n_sd <= ctx->parcel_rows) return SDM_OK;
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // earlier launches may still read the old ones
  if (ctx->parcel_identity) HIP_TRY(hipFree(ctx->parcel_identity));
  if (ctx->parcel_backup) HIP_TRY(hipFree(ctx->parcel_backup));
  ctx->parcel_identity = nullptr;
  ctx->parcel_backup = nullptr;
  ctx->parcel_rows = 0;
  const int64_t want = n_sd + n_sd / 4 + 1024;
  if (hipMalloc((void **)&ctx->parcel_identity, (size_t)want * sizeof(int64_t)) != hipSuccess ||
      hipMalloc((void **)&ctx->parcel_backup, (size_t)want * sizeof(double)) != hipSuccess) {
    sdm_set_error("sdm_parcel_run: hipMalloc of 2 x %lld words failed", (long long)want);
    return SDM_E_NOMEM;
  }
  ctx->parcel_rows = want;
  return sdm_identity_index(ctx, ctx->parcel_identity, want);
}

// every parcel has rows, and they lie within the columns: the kernels index by these words
int check_starts(sdm_ctx *ctx, const int64_t *parcel_start, int64_t n_parcel, int64_t n_sd) {
  std::vector<int64_t> starts((size_t)n_parcel + 1);
  HIP_TRY(hipMemcpyAsync(starts.data(), parcel_start, starts.size() * sizeof(int64_t),
                         hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ARG_TRY(starts[0] >= 0 && starts[(size_t)n_parcel] <= n_sd);
  for (int64_t c = 0; c < n_parcel; ++c)
    if (starts[(size_t)c + 1] <= starts[(size_t)c]) {
      sdm_set_error("sdm_parcel_run: parcel %lld has no rows", (long long)c);
      return SDM_E_ARG;
    }
  return SDM_OK;
}

// the refusals of include/sdm_parcel_diag.h (comparisons written so that a NaN fails them)
int check_requests(const sdm_parcel_requests *rq) {
  ARG_TRY(rq->n_moments >= 0 && rq->n_moments <= SDM_PARCEL_MAX_MOMENTS);
  ARG_TRY(rq->n_bins >= 0 && rq->n_bins <= SDM_PARCEL_MAX_BINS);
  for (int i = 0; i < rq->n_moments; ++i) {
    const sdm_parcel_moment_request &m = rq->moment[i];
    ARG_TRY(m.attr >= 0 && m.attr < SDM_PARCEL_N_ATTRS);
    ARG_TRY(m.filter_attr >= 0 && m.filter_attr < SDM_PARCEL_N_FILTERS);
    ARG_TRY(m.min_x <= m.max_x);
    ARG_TRY(m.rank == m.rank);
  }
  if (rq->n_bins > 0) {
    ARG_TRY(rq->bin_attr >= 0 && rq->bin_attr < SDM_PARCEL_N_FILTERS);
    for (int b = 0; b < rq->n_bins; ++b) ARG_TRY(rq->edges[b] < rq->edges[b + 1]);
  }
  return SDM_OK;
}

// the table to device memory, behind whatever still reads the previous one on the stream; the
// caller synchronises the stream before it returns (the source is the caller's host struct)
int upload_requests(sdm_ctx *ctx, const sdm_parcel_requests *rq) {
  if (!ctx->parcel_requests)
    HIP_TRY(hipMalloc(&ctx->parcel_requests, sizeof(sdm_parcel_requests)));
  HIP_TRY(hipMemcpyAsync(ctx->parcel_requests, rq, sizeof(sdm_parcel_requests),
                         hipMemcpyHostToDevice, ctx->stream));
  return SDM_OK;
}

bool wants_output(const sdm_parcel_diag *diag) {
  return diag && (diag->moment_0 || diag->moments || diag->spectrum || diag->dv);
}

}  // namespace

extern "C" int sdm_parcel_run(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, int64_t n_steps,
                              int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start,
                              double *water_mass, const int64_t *multiplicity,
                              const double *vdry, const double *kappa, const double *f_org,
                              double *v_cr, const sdm_parcel_state *state, const double *w_mid,
                              const sdm_parcel_profile *profile, const double consts[34],
                              const sdm_cond_formulae *formulae) {
  return sdm_parcel_run_diag(ctx, cfg, n_steps, n_parcel, n_sd, parcel_start, water_mass,
                             multiplicity, vdry, kappa, f_org, v_cr, state, w_mid, profile, consts,
                             formulae, nullptr, nullptr);
}

int sdm_parcel_prepare(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, int64_t n_steps, int64_t n_parcel,
                       int64_t n_sd, const int64_t *parcel_start, double *water_mass,
                       const int64_t *multiplicity, const double *vdry, const double *kappa,
                       const double *f_org, double *v_cr, const sdm_parcel_state *state,
                       const double *w_mid, const sdm_parcel_profile *profile,
                       const double consts[34], const sdm_cond_formulae *formulae,
                       const sdm_parcel_requests *requests, const sdm_parcel_diag *diag,
                       ParcelCall *out, bool *with_diag_out, bool *nothing_to_do,
                       bool ventilated) {
  *nothing_to_do = true;
  *with_diag_out = false;
  ARG_TRY(ctx && cfg && consts && state);
  ARG_TRY(n_steps >= 0 && n_parcel >= 0 && n_sd >= 0 && n_parcel <= 0x7fffffff);
  ARG_TRY(cfg->multiplier >= 1 && cfg->fuse >= 0 && cfg->max_iters >= 0 && cfg->dt > 0);
  ARG_TRY(cfg->dt_min != 0);
  ARG_TRY(cfg->steps_per_launch >= 0);
  if (ventilated)  // (the launchers check the rest of the descriptor)
    ARG_TRY(formulae && formulae->option[SDM_COND_OPT_VENTILATION] != SDM_COND_VENT_NEGLECT);
  else if (formulae)
    ARG_TRY(formulae->option[SDM_COND_OPT_VENTILATION] == SDM_COND_VENT_NEGLECT);
  const bool with_diag = wants_output(diag);  // otherwise: the kernels of sdm_parcel_run
  if (requests) {
    const int checked = check_requests(requests);
    if (checked != SDM_OK) return checked;
  }
  ARG_TRY(!with_diag || requests);
  if (n_parcel == 0 || n_steps == 0) return SDM_OK;
  ARG_TRY(parcel_start && water_mass && multiplicity && vdry && kappa && v_cr && w_mid);
  ARG_TRY(state->z && state->rhod && state->thd && state->qv && state->T && state->p &&
          state->RH && state->qv_prev && state->mass_of_dry_air && state->n_substeps &&
          state->n_activating && state->n_deactivating && state->n_ripening && state->RH_max &&
          state->steps_done && state->failed_step);
  if (with_diag) {
    const int uploaded = upload_requests(ctx, requests);
    if (uploaded != SDM_OK) return uploaded;
  }
  const int starts_ok = check_starts(ctx, parcel_start, n_parcel, n_sd);  // (synchronises)
  if (starts_ok != SDM_OK) return starts_ok;
  const int rc = reserve_rows(ctx, n_sd);
  if (rc != SDM_OK) return rc;

  ParcelCall &call = *out;
  call.cfg = *cfg;
  call.n_parcel = n_parcel;
  call.n_sd = n_sd;
  call.parcel_start = parcel_start;
  call.identity = ctx->parcel_identity;
  call.multiplicity = multiplicity;
  call.water_mass = water_mass;
  call.v_cr = v_cr;
  call.mass_backup = ctx->parcel_backup;
  call.vdry = vdry;
  call.kappa = kappa;
  call.f_org = f_org;
  call.w_mid = w_mid;
  call.consts = consts;
  call.state = *state;
  if (profile) call.profile = *profile;
  else memset(&call.profile, 0, sizeof(call.profile));
  call.requests = with_diag ? (const sdm_parcel_requests *)ctx->parcel_requests : nullptr;
  if (with_diag) call.diag = *diag;
  else memset(&call.diag, 0, sizeof(call.diag));
  call.k0 = call.k_count = 0;
  *with_diag_out = with_diag;
  *nothing_to_do = false;
  return SDM_OK;
}

extern "C" int sdm_parcel_run_diag(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, int64_t n_steps,
                                   int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start,
                                   double *water_mass, const int64_t *multiplicity,
                                   const double *vdry, const double *kappa, const double *f_org,
                                   double *v_cr, const sdm_parcel_state *state,
                                   const double *w_mid, const sdm_parcel_profile *profile,
                                   const double consts[34], const sdm_cond_formulae *formulae,
                                   const sdm_parcel_requests *requests,
                                   const sdm_parcel_diag *diag) {
  ParcelCall call;
  bool with_diag, nothing_to_do;
  const int prepared = sdm_parcel_prepare(ctx, cfg, n_steps, n_parcel, n_sd, parcel_start,
                                          water_mass, multiplicity, vdry, kappa, f_org, v_cr, state,
                                          w_mid, profile, consts, formulae, requests, diag, &call,
                                          &with_diag, &nothing_to_do);
  if (prepared != SDM_OK || nothing_to_do) return prepared;
  const int64_t per_launch =
      cfg->steps_per_launch > 0 ? cfg->steps_per_launch : SDM_PARCEL_STEPS_PER_LAUNCH;
  for (int64_t k0 = 0; k0 < n_steps; k0 += per_launch) {
    call.k0 = k0;
    call.k_count = n_steps - k0 < per_launch ? n_steps - k0 : per_launch;
    const int launched = formulae ? sdm_parcel_launch_general(ctx, call, formulae)
                                  : sdm_parcel_launch_default(ctx, call);
    if (launched != SDM_OK) return launched;
  }
  return SDM_OK;
}

// include/sdm_parcel_vent.h: the same chunking on the ventilated kernels
extern "C" int sdm_parcel_run_vent(sdm_ctx *ctx, const sdm_parcel_cfg *cfg, int64_t n_steps,
                                   int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start,
                                   double *water_mass, const int64_t *multiplicity,
                                   const double *vdry, const double *kappa, const double *f_org,
                                   double *v_cr, const sdm_parcel_state *state,
                                   const double *w_mid, const sdm_parcel_profile *profile,
                                   const double consts[34], const sdm_cond_formulae *formulae,
                                   const sdm_parcel_requests *requests,
                                   const sdm_parcel_diag *diag, const sdm_parcel_vent *vent) {
  ARG_TRY(formulae && vent);
  ARG_TRY(formulae->option[SDM_COND_OPT_VENTILATION] != SDM_COND_VENT_NEGLECT);
  const int law = vent->velocity_law;
  ARG_TRY(law >= SDM_VELOCITY_LAW_GUNN_KINZER && law <= SDM_VELOCITY_LAW_POWER_SERIES);
  if (law == SDM_VELOCITY_LAW_GUNN_KINZER)
    ARG_TRY(vent->gk_a && vent->gk_b && vent->gk_table_len >= 1);
  if (law == SDM_VELOCITY_LAW_ROGERS_YAU) ARG_TRY(vent->velocity_params);
  if (law == SDM_VELOCITY_LAW_POWER_SERIES)
    ARG_TRY(vent->velocity_terms >= 0 && vent->velocity_terms <= SDM_VELOCITY_MAX_TERMS &&
            (vent->velocity_terms == 0 || vent->velocity_params));
  ARG_TRY(vent->air_density && vent->air_dynamic_viscosity && vent->reynolds_number);
  ParcelCall call;
  bool with_diag, nothing_to_do;
  const int prepared = sdm_parcel_prepare(ctx, cfg, n_steps, n_parcel, n_sd, parcel_start,
                                          water_mass, multiplicity, vdry, kappa, f_org, v_cr, state,
                                          w_mid, profile, consts, formulae, requests, diag, &call,
                                          &with_diag, &nothing_to_do, true);
  if (prepared != SDM_OK || nothing_to_do) return prepared;
  const int64_t per_launch =
      cfg->steps_per_launch > 0 ? cfg->steps_per_launch : SDM_PARCEL_STEPS_PER_LAUNCH;
  for (int64_t k0 = 0; k0 < n_steps; k0 += per_launch) {
    call.k0 = k0;
    call.k_count = n_steps - k0 < per_launch ? n_steps - k0 : per_launch;
    const int launched = sdm_parcel_launch_vent(ctx, call, formulae, vent);
    if (launched != SDM_OK) return launched;
  }
  return SDM_OK;
}

// include/sdm_parcel_ice.h: the same chunking on the kernels with the ice passes
extern "C" int sdm_parcel_run_ice(sdm_ctx *ctx, const sdm_parcel_cfg *cfg,
                                  const sdm_parcel_ice_cfg *ice_cfg, int64_t n_steps,
                                  int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start,
                                  double *signed_water_mass, const int64_t *multiplicity,
                                  const double *vdry, const double *kappa, const double *f_org,
                                  double *v_cr, const sdm_parcel_state *state,
                                  const double *w_mid, const sdm_parcel_profile *profile,
                                  const double consts[34], const sdm_cond_formulae *formulae,
                                  const sdm_parcel_ice_state *ice_state,
                                  const sdm_parcel_ice_profile *ice_profile,
                                  const double frz_consts[33], const double dep_consts[39]) {
  ARG_TRY(ice_cfg && ice_state && frz_consts);
  const bool freezing = ice_cfg->freezing != 0, deposition = ice_cfg->deposition != 0;
  ARG_TRY(freezing || deposition);  // (neither: that is sdm_parcel_run)
  ARG_TRY(ice_cfg->order == SDM_PARCEL_ICE_FREEZING_FIRST ||
          ice_cfg->order == SDM_PARCEL_ICE_DEPOSITION_FIRST);
  ARG_TRY(ice_state->a_w_ice && ice_state->RH_ice && ice_state->n_exceeded);
  if (freezing) {
    const bool immersion = ice_cfg->immersion_freezing != 0, singular = ice_cfg->singular != 0;
    const bool hom = ice_cfg->homogeneous_freezing != 0;
    if (immersion && !singular)
      ARG_TRY(ice_cfg->j_het == SDM_FRZ_JHET_CONSTANT || ice_cfg->j_het == SDM_FRZ_JHET_ABIFM);
    if (hom)
      ARG_TRY(ice_cfg->j_hom >= SDM_FRZ_JHOM_CONSTANT &&
              ice_cfg->j_hom <= SDM_FRZ_JHOM_KOOPMURRAY2016);
    ARG_TRY(!(immersion && singular) || ice_state->freezing_temperature);
    ARG_TRY(!(immersion && !singular) || ice_state->immersed_surface_area);
    if ((immersion && !singular) || hom)
      ARG_TRY(ice_state->rng_offset && ice_state->rng_state_inc);
  }
  if (deposition) {
    ARG_TRY(dep_consts);
    ARG_TRY(ice_cfg->coordinate == SDM_DEP_COORD_WATER_MASS_LOGARITHM ||
            ice_cfg->coordinate == SDM_DEP_COORD_WATER_MASS);
    ARG_TRY(ice_cfg->capacity == SDM_DEP_CAPACITY_SPHERICAL ||
            ice_cfg->capacity == SDM_DEP_CAPACITY_COLUMNAR);
    ARG_TRY(ice_cfg->kinetics == SDM_DEP_KINETICS_STANDARD ||
            ice_cfg->kinetics == SDM_DEP_KINETICS_NEGLECT);
    ARG_TRY(ice_cfg->sum == SDM_DEP_SUM_ORDERED || ice_cfg->sum == SDM_DEP_SUM_BLOCKED);
  }
  ParcelCall call;
  bool with_diag, nothing_to_do;
  // (a ventilation other than Neglect is refused there)
  const int prepared = sdm_parcel_prepare(ctx, cfg, n_steps, n_parcel, n_sd, parcel_start,
                                          signed_water_mass, multiplicity, vdry, kappa, f_org, v_cr,
                                          state, w_mid, profile, consts, formulae, nullptr, nullptr,
                                          &call, &with_diag, &nothing_to_do);
  if (prepared != SDM_OK || nothing_to_do) return prepared;
  ParcelIceCall ice;
  ice.cfg = *ice_cfg;
  ice.st = *ice_state;
  if (ice_profile) ice.pr = *ice_profile;
  else memset(&ice.pr, 0, sizeof(ice.pr));
  ice.frz_consts = frz_consts;
  ice.dep_consts = dep_consts;
  const int64_t per_launch =
      cfg->steps_per_launch > 0 ? cfg->steps_per_launch : SDM_PARCEL_STEPS_PER_LAUNCH;
  for (int64_t k0 = 0; k0 < n_steps; k0 += per_launch) {
    call.k0 = k0;
    call.k_count = n_steps - k0 < per_launch ? n_steps - k0 : per_launch;
    const int launched = formulae ? sdm_parcel_launch_general_ice(ctx, call, formulae, ice)
                                  : sdm_parcel_launch_default_ice(ctx, call, ice);
    if (launched != SDM_OK) return launched;
  }
  return SDM_OK;
}

extern "C" int sdm_parcel_diagnose(sdm_ctx *ctx, int64_t n_parcel, int64_t n_sd,
                                   const int64_t *parcel_start, const double *water_mass,
                                   const int64_t *multiplicity, const double *vdry,
                                   const double *kappa, const double *f_org, const double *T,
                                   const double consts[34], const sdm_cond_formulae *formulae,
                                   const sdm_parcel_requests *requests,
                                   const sdm_parcel_diag *diag) {
  ARG_TRY(ctx && consts && requests && diag);
  ARG_TRY(n_parcel >= 0 && n_sd >= 0 && n_parcel <= 0x7fffffff);
  const int checked = check_requests(requests);
  if (checked != SDM_OK) return checked;
  if (n_parcel == 0) return SDM_OK;
  ARG_TRY(parcel_start && water_mass && multiplicity && vdry && kappa && T);
  const int uploaded = upload_requests(ctx, requests);
  if (uploaded != SDM_OK) return uploaded;
  const int starts_ok = check_starts(ctx, parcel_start, n_parcel, n_sd);  // (synchronises)
  if (starts_ok != SDM_OK) return starts_ok;
  ParcelDiagnoseCall call;
  call.n_parcel = n_parcel;
  call.n_sd = n_sd;
  call.parcel_start = parcel_start;
  call.multiplicity = multiplicity;
  call.water_mass = water_mass;
  call.vdry = vdry;
  call.kappa = kappa;
  call.f_org = f_org;
  call.T = T;
  call.consts = consts;
  call.requests = (const sdm_parcel_requests *)ctx->parcel_requests;
  call.diag = *diag;
  call.diag.dv = nullptr;
  call.failed_step = nullptr;
  return formulae ? sdm_parcel_diagnose_general(ctx, call, formulae)
                  : sdm_parcel_diagnose_default(ctx, call);
}

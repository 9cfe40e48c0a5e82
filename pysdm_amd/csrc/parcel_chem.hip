// parcel_chem.hip -- the adiabatic parcel with aqueous chemistry (include/sdm_parcel_chem.h, where
// the step is written out): the entry point and k_parcel_chem, the chemistry of one time step of
// every parcel.
//
// A step is two launches on the context's stream, three with a request table, and no host
// synchronisation between them:
//   1. a ONE-step launch of k_parcel / k_parcel_f (parcel_solver.h), as sdm_parcel_run makes it;
//   2. k_parcel_chem: points 2-5 of the header and the chemistry profile row;
//   3. k_parcel_diagnose(_f) on the columns k_parcel_chem left, at the temperature after the step.
// The chemistry is NOT inside parcel_steps<P>: k_parcel fills the register file (256 VGPRs, 992 B
// of scratch per lane), the chemistry row code is promised scratch-free, and a launch boundary
// costs microseconds against a parcel step of more than a hundred.
//
// k_parcel_chem: one workgroup of 256 lanes per parcel, the workgroups striding over the parcels
// (any grid size is correct; no grid barrier, no residency assumption; every loop is bounded by
// n_substep or the parcel's rows).  What one workgroup per parcel buys over sdm_chemistry_step,
// where a cell may span workgroups: the whole sub-step loop of a CLOSED system runs in one launch.
// The parcel's six mixing ratios and its 17 temperature-dependent constants (chem_cell_data, once
// per step) live in LDS; the `taken` sums are formed in the workgroup in the two shapes of
// sdm_chemistry.h, add for add as k_chem_sum forms them; barriers separate points 1-3, the sum
// and points 4-6.  A parcel of at most 256 rows keeps each row's seven amounts, pH, flag and volume
// in registers across all sub-steps; larger parcels stride their rows (q = t, t + 256, ...)
// through memory between the phases, every location written and read by the same lane.  The row
// arithmetic is chemistry_rows.h (chem_half, chem_cell_data, chem_delta_mr) with toms748.h, the
// functions k_chem_step calls: the two routes agree to the bit by construction.
//
// dv without touching the parcel kernels: `rhod_prev` holds every parcel's density before the
// step; the entry point fills it from rhod, the kernel saves rhod into it at its end, and
// (rhod + rhod_prev) / 2 has the two operands of the parcel step's (prhod + rhod) / 2.
//
// A parcel whose solver failed (failed_step >= 0, now or in an earlier step or call) is skipped
// whole.  The three event counts are integers: one atomic per wave.
#include "parcel_solver.h"
#include "chemistry_rows.h"
#include "../../include/sdm_parcel_chem.h"

#define PCH_CB 256  // lanes per workgroup == SDM_CHEM_SUM_BLOCK == the partials of the header's SUM

namespace {

struct ChemK { double v[SDM_CHEM_N_CONSTS]; };

struct ParcelChemArgs {
  int64_t n_parcel, n_sd;
  int64_t at0;  // the first entry of this step's profile rows: k * n_parcel
  const int64_t *parcel_start, *multiplicity, *failed_step;
  const double *water_mass, *ktdv, *T, *p, *rhod, *mass_of_dry_air;
  double *rhod_prev, *vdry, *kappa, *pH;
  uint8_t *flag;
  double *moles[SDM_CHEM_N_AQ];
  double *mr[SDM_CHEM_N_GAS];
  double *dq;     // closed system: [6][n_sd], the staging of parcels of more than PCH_CB rows
  uint8_t *took;  // closed system: [n_sd]
  int64_t *n_failed, *n_negative, *n_exceeded;  // per parcel, may be NULL
  sdm_parcel_chem_profile pr;
  double *diag_dv;  // sdm_parcel_diag's dv, may be NULL
  int n_sub, closed, blocked;
  double dt, H_min, H_max, threshold, rtol, rho_w, dry_factor;
  ChemK k;
};

__device__ __forceinline__ void count_add(int64_t *counter, int64_t v) {  // wave-collective
  const int64_t s = wave_sum_i64(v);
  if (counter && lane_id() == 0 && s != 0)
    atomicAdd((unsigned long long *)counter, (unsigned long long)s);
}

__global__ void __launch_bounds__(PCH_CB) k_parcel_chem(ParcelChemArgs a) {
  __shared__ chem_cell s_cell;
  __shared__ double s_mr[SDM_CHEM_N_GAS];
  // the sums' staging, a[g][0 .. 2 * PCH_CB) as in k_chem_sum; afterwards the 7 x PCH_CB partials of
  // aq_total
  __shared__ double s_a[SDM_CHEM_N_GAS * 2 * PCH_CB];
  __shared__ int s_wave_count[PCH_CB / SDM_WAVE];
  __shared__ unsigned long long s_flagged;
  const int tid = (int)threadIdx.x;
  const double *k = a.k.v;
  for (int64_t c = blockIdx.x; c < a.n_parcel; c += gridDim.x) {
    const int64_t row0 = a.parcel_start[c], n = a.parcel_start[c + 1] - row0;
    // (checked on the host too; a failed parcel is left alone for good.  Uniform over the workgroup)
    if (row0 < 0 || n <= 0 || row0 + n > a.n_sd || a.failed_step[c] >= 0) continue;
    __syncthreads();  // the previous parcel's reads of LDS are over
    const double T = a.T[c], p = a.p[c], rhod = a.rhod[c];
    const double dv = a.mass_of_dry_air[c] / ((rhod + a.rhod_prev[c]) / 2);
    if (tid == 0) {
      chem_cell_data(k, T, &s_cell);
      s_flagged = 0;
    }
    if (tid == SDM_WAVE) {
#pragma unroll
      for (int g = 0; g < SDM_CHEM_N_GAS; ++g) s_mr[g] = a.mr[g][c];
    }
    __syncthreads();

    const bool resident = n <= PCH_CB;  // the row of lane `tid` stays in registers
    chem_drop d;
    double mult = 0.0;
    if (resident && tid < n) {
      const int64_t row = row0 + tid;
#pragma unroll
      for (int q = 0; q < SDM_CHEM_N_AQ; ++q) d.m[q] = a.moles[q][row];
      d.pH = a.pH[row];
      d.flag = a.flag[row] != 0;
      d.volume = a.water_mass[row] / a.rho_w;
      mult = (double)a.multiplicity[row];
    }
    int64_t counts[2] = {0, 0};
    int64_t exceeded = 0;
#pragma unroll 1
    for (int half = 0; half < 2 * a.n_sub; ++half) {
      const int which = half & 1;
      double dq_reg[SDM_CHEM_N_GAS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      int took_reg = 0;
#pragma unroll 1
      for (int64_t q = tid; q < n; q += PCH_CB) {
        const int64_t row = row0 + q;
        if (!resident) {
#pragma unroll
          for (int s = 0; s < SDM_CHEM_N_AQ; ++s) d.m[s] = a.moles[s][row];
          d.pH = a.pH[row];
          d.flag = a.flag[row] != 0;
          d.volume = a.water_mass[row] / a.rho_w;
          mult = (double)a.multiplicity[row];
        }
        chem_half(k, &s_cell, s_mr, p, T, a.dt, a.H_min, a.H_max, a.threshold, a.rtol, mult, &d,
                  which, dq_reg, &took_reg, counts);
        if (!resident) {
          if (which == 0 && a.closed) {
            a.took[row] = (uint8_t)took_reg;
            if (took_reg) {
#pragma unroll
              for (int g = 0; g < SDM_CHEM_N_GAS; ++g) a.dq[(int64_t)g * a.n_sd + row] = dq_reg[g];
            }
          }
#pragma unroll
          for (int s = 0; s < SDM_CHEM_N_AQ; ++s) a.moles[s][row] = d.m[s];
          a.pH[row] = d.pH;
          a.flag[row] = (uint8_t)d.flag;
        }
      }
      if (which != 0 || !a.closed) continue;  // (uniform)
      // ---- the six `taken` sums and the decrements, as k_chem_sum (chemistry.hip) forms them ------
      double acc = 0.0;    // lanes 0..5: the gas tid
      int64_t n_took = 0;  // uniform over the workgroup
      int fill = 0;        // blocked: compacted entries waiting in s_a (uniform)
      auto reduce_block = [&](int len) {
        for (int h = PCH_CB / 2; h >= 1; h /= 2) {
          if (tid < h && tid + h < len) {
#pragma unroll
            for (int g = 0; g < SDM_CHEM_N_GAS; ++g)
              s_a[g * 2 * PCH_CB + tid] += s_a[g * 2 * PCH_CB + tid + h];
          }
          __syncthreads();
        }
        if (tid < SDM_CHEM_N_GAS) acc += s_a[tid * 2 * PCH_CB];
        __syncthreads();
      };
      for (int64_t base = 0; base < n; base += PCH_CB) {
        const int64_t q = base + tid;
        bool in = false;
        double v[SDM_CHEM_N_GAS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (q < n) {
          if (resident) {
            in = took_reg != 0;
#pragma unroll
            for (int g = 0; g < SDM_CHEM_N_GAS; ++g) v[g] = in ? dq_reg[g] : 0.0;
          } else {
            in = a.took[row0 + q] != 0;  // (this lane wrote it: program order)
            if (in) {
#pragma unroll
              for (int g = 0; g < SDM_CHEM_N_GAS; ++g) v[g] = a.dq[(int64_t)g * a.n_sd + row0 + q];
            }
          }
        }
        // position of this lane among the chunk's rows that took part
        const unsigned long long ballot = __ballot(in);
        const int wave = tid / SDM_WAVE;
        if (lane_id() == 0) s_wave_count[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, chunk_took = 0;
#pragma unroll
        for (int w = 0; w < PCH_CB / SDM_WAVE; ++w) {
          if (w < wave) before += s_wave_count[w];
          chunk_took += s_wave_count[w];
        }
        before += __popcll(ballot & ((1ull << lane_id()) - 1));
        n_took += chunk_took;
        if (!a.blocked) {
#pragma unroll
          for (int g = 0; g < SDM_CHEM_N_GAS; ++g) s_a[g * 2 * PCH_CB + tid] = v[g];
          __syncthreads();
          if (tid < SDM_CHEM_N_GAS) {
            const int stop = (int)(n - base < PCH_CB ? n - base : PCH_CB);
            for (int j = 0; j < stop; ++j) acc += s_a[tid * 2 * PCH_CB + j];
          }
          __syncthreads();
        } else {
          if (in) {
#pragma unroll
            for (int g = 0; g < SDM_CHEM_N_GAS; ++g) s_a[g * 2 * PCH_CB + fill + before] = v[g];
          }
          fill += chunk_took;
          __syncthreads();
          if (fill >= PCH_CB) {
            // the entries past the block are kept in registers over the destructive reduction
            double keep[SDM_CHEM_N_GAS];
            const int rest = fill - PCH_CB;
#pragma unroll
            for (int g = 0; g < SDM_CHEM_N_GAS; ++g)
              keep[g] = tid < rest ? s_a[g * 2 * PCH_CB + PCH_CB + tid] : 0.0;
            reduce_block(PCH_CB);
            if (tid < rest) {
#pragma unroll
              for (int g = 0; g < SDM_CHEM_N_GAS; ++g) s_a[g * 2 * PCH_CB + tid] = keep[g];
            }
            fill = rest;
            __syncthreads();
          }
        }
      }
      if (a.blocked && fill > 0) reduce_block(fill);
      if (tid < SDM_CHEM_N_GAS && n_took > 0) {
        const double delta = chem_delta_mr(k, tid, acc, dv, rhod);
        const double had = s_mr[tid];
        exceeded += !(delta <= had);
        s_mr[tid] = had - delta;
      }
      __syncthreads();  // the next sub-step reads the new mixing ratios
    }

    // ---- point 4, the amounts' write-back and the partial sums of aq_total ---------------------------
    double part[SDM_CHEM_N_AQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int64_t flagged = 0;
#pragma unroll 1
    for (int64_t q = tid; q < n; q += PCH_CB) {
      const int64_t row = row0 + q;
      if (resident) {
#pragma unroll
        for (int s = 0; s < SDM_CHEM_N_AQ; ++s) a.moles[s][row] = d.m[s];
        a.pH[row] = d.pH;
        a.flag[row] = (uint8_t)d.flag;
      } else {  // (this lane wrote them: program order)
#pragma unroll
        for (int s = 0; s < SDM_CHEM_N_AQ; ++s) d.m[s] = a.moles[s][row];
        d.flag = a.flag[row] != 0;
        mult = (double)a.multiplicity[row];
      }
      const double vd = d.m[SDM_CHEM_AQ_S_VI] * a.dry_factor;
      a.vdry[row] = vd;
      a.kappa[row] = a.ktdv[row] / vd;
#pragma unroll
      for (int s = 0; s < SDM_CHEM_N_AQ; ++s) part[s] += mult * d.m[s];
      flagged += d.flag ? 1 : 0;
    }
    // the SUM of include/sdm_parcel_diag.h: 256 partials, then the strides 128 .. 1
#pragma unroll
    for (int s = 0; s < SDM_CHEM_N_AQ; ++s) s_a[s * PCH_CB + tid] = part[s];
    if (flagged) atomicAdd(&s_flagged, (unsigned long long)flagged);
    __syncthreads();
    for (int stride = PCH_CB / 2; stride >= 1; stride /= 2) {
      if (tid < stride) {
#pragma unroll
        for (int s = 0; s < SDM_CHEM_N_AQ; ++s)
          s_a[s * PCH_CB + tid] += s_a[s * PCH_CB + tid + stride];
      }
      __syncthreads();
    }
    if (tid == 0) {
      const int64_t at = a.at0 + c;
#pragma unroll
      for (int g = 0; g < SDM_CHEM_N_GAS; ++g) {
        if (a.closed) a.mr[g][c] = s_mr[g];
        if (a.pr.mixing_ratio[g]) a.pr.mixing_ratio[g][at] = s_mr[g];
      }
#pragma unroll
      for (int s = 0; s < SDM_CHEM_N_AQ; ++s)
        if (a.pr.aq_total[s]) a.pr.aq_total[s][at] = s_a[s * PCH_CB];
      if (a.pr.n_flagged) a.pr.n_flagged[at] = (int64_t)s_flagged;
      if (a.pr.dv) a.pr.dv[at] = dv;
      if (a.diag_dv) a.diag_dv[at] = dv;
      a.rhod_prev[c] = rhod;  // (every lane read it before the barriers above)
    }
    count_add(a.n_failed ? a.n_failed + c : nullptr, counts[0]);
    count_add(a.n_negative ? a.n_negative + c : nullptr, counts[1]);
    if (tid < SDM_WAVE) count_add(a.n_exceeded ? a.n_exceeded + c : nullptr, exceeded);
  }
}

template <int N>
bool take(double *(&dst)[N], double *const *src) {
  if (!src) return false;
  for (int i = 0; i < N; ++i) {
    if (!src[i]) return false;
    dst[i] = src[i];
  }
  return true;
}

// rhod_prev (n_parcel doubles) and, for a closed system, dq (6 n_sd doubles) and took (n_sd bytes)
int reserve_chem(sdm_ctx *ctx, size_t bytes) {
  if (bytes <= ctx->parcel_chem_bytes) return SDM_OK;
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // earlier launches may still use the old one
  if (ctx->parcel_chem_buf) HIP_TRY(hipFree(ctx->parcel_chem_buf));
  ctx->parcel_chem_buf = nullptr;
  ctx->parcel_chem_bytes = 0;
  const size_t want = bytes + bytes / 4 + 4096;
  if (hipMalloc((void **)&ctx->parcel_chem_buf, want) != hipSuccess) {
    sdm_set_error("sdm_parcel_run_chem: hipMalloc(%zu) failed", want);
    return SDM_E_NOMEM;
  }
  ctx->parcel_chem_bytes = want;
  return SDM_OK;
}

}  // namespace

extern "C" int sdm_parcel_run_chem(
    sdm_ctx *ctx, const sdm_parcel_cfg *cfg, const sdm_chemistry_cfg *chem_cfg, int64_t n_steps,
    int64_t n_parcel, int64_t n_sd, const int64_t *parcel_start, double *water_mass,
    const int64_t *multiplicity, double *vdry, double *kappa, const double *f_org, double *v_cr,
    const sdm_parcel_state *state, const double *w_mid, const sdm_parcel_profile *profile,
    const double consts[34], const sdm_cond_formulae *formulae,
    const sdm_parcel_requests *requests, const sdm_parcel_diag *diag,
    const double *kappa_times_dry_volume, double *const moles[7], double *pH,
    uint8_t *do_chemistry_flag, double *const env_mixing_ratio[6], const double chem_consts[62],
    double dry_factor, int64_t *n_failed, int64_t *n_negative, int64_t *n_exceeded,
    const sdm_parcel_chem_profile *chem_profile) {
  ARG_TRY(ctx && chem_cfg && chem_consts);
  ARG_TRY(chem_cfg->n_substep >= 1);
  ARG_TRY(chem_cfg->system_type == SDM_CHEM_SYSTEM_OPEN ||
          chem_cfg->system_type == SDM_CHEM_SYSTEM_CLOSED);
  ARG_TRY(chem_cfg->sum == SDM_CHEM_SUM_ORDERED || chem_cfg->sum == SDM_CHEM_SUM_BLOCKED);
  // (the organic fraction would have to follow the dry volume)
  if (formulae)
    ARG_TRY(formulae->option[SDM_COND_OPT_SURFACE_TENSION] == SDM_COND_SGM_CONSTANT);
  ParcelCall call;
  bool with_diag, nothing_to_do;
  const int prepared = sdm_parcel_prepare(ctx, cfg, n_steps, n_parcel, n_sd, parcel_start,
                                          water_mass, multiplicity, vdry, kappa, f_org, v_cr, state,
                                          w_mid, profile, consts, formulae, requests, diag, &call,
                                          &with_diag, &nothing_to_do);
  if (prepared != SDM_OK || nothing_to_do) return prepared;

  ParcelChemArgs a;
  ARG_TRY(kappa_times_dry_volume && pH && do_chemistry_flag && take(a.moles, moles) &&
          take(a.mr, env_mixing_ratio));
  const bool closed = chem_cfg->system_type == SDM_CHEM_SYSTEM_CLOSED;
  const size_t prev_bytes = carve_size(sizeof(double) * (size_t)n_parcel);
  const size_t dq_bytes = closed ? carve_size(sizeof(double) * 6 * (size_t)n_sd) : 0;
  const size_t took_bytes = closed ? carve_size((size_t)n_sd) : 0;
  const int reserved = reserve_chem(ctx, prev_bytes + dq_bytes + took_bytes);
  if (reserved != SDM_OK) return reserved;
  Carver cv(ctx->parcel_chem_buf);
  a.rhod_prev = cv.take<double>((size_t)n_parcel);
  a.dq = closed ? cv.take<double>(6 * (size_t)n_sd) : nullptr;
  a.took = closed ? cv.take<uint8_t>((size_t)n_sd) : nullptr;
  HIP_TRY(hipMemcpyAsync(a.rhod_prev, state->rhod, sizeof(double) * (size_t)n_parcel,
                         hipMemcpyDeviceToDevice, ctx->stream));
  a.n_parcel = n_parcel;
  a.n_sd = n_sd;
  a.parcel_start = parcel_start;
  a.multiplicity = multiplicity;
  a.failed_step = state->failed_step;
  a.water_mass = water_mass;
  a.ktdv = kappa_times_dry_volume;
  a.T = state->T;
  a.p = state->p;
  a.rhod = state->rhod;
  a.mass_of_dry_air = state->mass_of_dry_air;
  a.vdry = vdry;
  a.kappa = kappa;
  a.pH = pH;
  a.flag = do_chemistry_flag;
  a.n_failed = n_failed;
  a.n_negative = n_negative;
  a.n_exceeded = n_exceeded;
  if (chem_profile) a.pr = *chem_profile;
  else memset(&a.pr, 0, sizeof(a.pr));
  a.diag_dv = with_diag ? diag->dv : nullptr;
  a.n_sub = chem_cfg->n_substep;
  a.closed = closed;
  a.blocked = chem_cfg->sum == SDM_CHEM_SUM_BLOCKED;
  a.dt = cfg->dt / chem_cfg->n_substep;
  a.H_min = chem_cfg->H_min;
  a.H_max = chem_cfg->H_max;
  a.threshold = chem_cfg->ionic_strength_threshold;
  a.rtol = chem_cfg->rtol;
  a.rho_w = consts[SDM_COND_K_RHO_W];
  a.dry_factor = dry_factor;
  memcpy(a.k.v, chem_consts, sizeof(a.k.v));

  // the parcel kernels without diagnostics; the table goes to the stage kernel after the chemistry
  ParcelDiagnoseCall dc;
  if (with_diag) {
    dc.n_parcel = n_parcel;
    dc.n_sd = n_sd;
    dc.parcel_start = parcel_start;
    dc.multiplicity = multiplicity;
    dc.water_mass = water_mass;
    dc.vdry = vdry;
    dc.kappa = kappa;
    dc.f_org = f_org;
    dc.T = state->T;
    dc.consts = consts;
    dc.requests = call.requests;
    dc.failed_step = state->failed_step;
  }
  call.requests = nullptr;
  memset(&call.diag, 0, sizeof(call.diag));
  const int64_t nm = requests ? requests->n_moments : 0, nb = requests ? requests->n_bins : 0;
  const unsigned grid =
      (unsigned)(n_parcel < SDM_PARCEL_CHEM_MAX_GRID ? n_parcel : SDM_PARCEL_CHEM_MAX_GRID);
  for (int64_t step = 0; step < n_steps; ++step) {
    call.k0 = step;
    call.k_count = 1;
    const int launched = formulae ? sdm_parcel_launch_general(ctx, call, formulae)
                                  : sdm_parcel_launch_default(ctx, call);
    if (launched != SDM_OK) return launched;
    a.at0 = step * n_parcel;
    hipLaunchKernelGGL(k_parcel_chem, dim3(grid), dim3(PCH_CB), 0, ctx->stream, a);
    LAUNCH_CHECK();
    if (with_diag) {
      const int64_t at = step * n_parcel;
      dc.diag.moment_0 = diag->moment_0 ? diag->moment_0 + at * nm : nullptr;
      dc.diag.moments = diag->moments ? diag->moments + at * nm : nullptr;
      dc.diag.spectrum = diag->spectrum ? diag->spectrum + at * nb : nullptr;
      dc.diag.dv = nullptr;
      const int diagnosed = formulae ? sdm_parcel_diagnose_general(ctx, dc, formulae)
                                     : sdm_parcel_diagnose_default(ctx, dc);
      if (diagnosed != SDM_OK) return diagnosed;
    }
  }
  return SDM_OK;
}

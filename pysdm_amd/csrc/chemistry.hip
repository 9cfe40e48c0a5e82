// chemistry.hip -- aqueous chemistry (include/sdm_chemistry.h): PySDM's `AqueousChemistry` dynamic
//
// The arithmetic of a cell and of a row is csrc/chemistry_rows.h (with csrc/toms748.h), which the
// CPU checker compiles too; this file is the kernels around it.
//   stage symbols   one launch each over columns in memory: k_chem_cells, k_chem_drops,
//                   k_chem_equilibrate, k_chem_dissolve (+ k_chem_sum, closed system), k_chem_oxidize
//   fused step      k_chem_step: one lane carries one super-droplet - 7 amounts, pH, flag, volume,
//                   the 17 constants of its cell, evaluated per row at the start - through the
//                   sub-steps; no barrier inside the loop, so a lane whose solve takes 32 iterations
//                   holds up its own wave only.  <true>: the records of up to 256 cells are
//                   filled into LDS once per workgroup (one barrier before the rows start).  Open system: one launch for all sub-steps.
//                   Closed system: one launch per sub-step, each followed by k_chem_sum, whose
//                   result the next launch reads
//   k_chem_sum      one workgroup per cell walks the cell's positions of idx in chunks of 256:
//                   ordered - lanes 0..5 each add one gas' staged values one by one (a row that
//                   did not take part is staged as +0.0, which leaves a sum that started at +0.0
//                   unchanged bit for bit); blocked - the rows that took part are compacted into
//                   LDS, every full 256 of them reduced in the fixed tree shape of the header
// No atomics on doubles anywhere; the three event counts are integers, one atomic per wave.
#include "common.h"
#include "chemistry_rows.h"

#define DF __device__ __forceinline__
#define CHEM_SB SDM_CHEM_SUM_BLOCK
// what SDM_CHEM_CONSTS_AUTO takes where both routes can run (profiles/chemistry_fused_vs_stages.jsonl)
#define SDM_CHEM_AUTO_PER_CELL 0

namespace {

struct ChemK { double v[SDM_CHEM_N_CONSTS]; };
struct Ptr7 { double *p[7]; };
struct Ptr6 { double *p[6]; };
struct Ptr5 { double *p[5]; };
struct Ptr4 { double *p[4]; };

template <typename P, typename T>
bool take(P &dst, T *const *src, int n) {
  if (!src) return false;
  for (int i = 0; i < n; ++i) {
    if (!src[i]) return false;
    dst.p[i] = (double *)src[i];
  }
  return true;
}

ChemK consts_of(const double *c) {
  ChemK k;
  memcpy(k.v, c, sizeof(k.v));
  return k;
}

DF void count_add(int64_t *counter, int64_t v) {  // wave-collective
  const int64_t s = wave_sum_i64(v);
  if (counter && lane_id() == 0 && s != 0)
    atomicAdd((unsigned long long *)counter, (unsigned long long)s);
}

// ---- stage kernels --------------------------------------------------------------------------------
__global__ void __launch_bounds__(SDM_BLOCK)
k_chem_cells(int64_t n_cell, const double *__restrict__ T, Ptr7 eq, Ptr4 kin, Ptr6 henry, ChemK k) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= n_cell) return;
  chem_cell cell;
  chem_cell_data(k.v, T[c], &cell);
#pragma unroll
  for (int e = 0; e < SDM_CHEM_N_EQ; ++e) eq.p[e][c] = cell.eq[e];
#pragma unroll
  for (int e = 0; e < SDM_CHEM_N_KIN; ++e) kin.p[e][c] = cell.kin[e];
#pragma unroll
  for (int g = 0; g < SDM_CHEM_N_GAS; ++g) henry.p[g][c] = cell.henry[g];
}

DF void load_eq(const Ptr7 &eq, int64_t c, double out[SDM_CHEM_N_EQ]) {
#pragma unroll
  for (int e = 0; e < SDM_CHEM_N_EQ; ++e) out[e] = eq.p[e][c];
}

__global__ void __launch_bounds__(SDM_BLOCK)
k_chem_drops(int64_t n_sd, const double *__restrict__ pH, const int64_t *__restrict__ cell_id,
             Ptr7 eq, Ptr6 df, ChemK k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n_sd) return;
  double e[SDM_CHEM_N_EQ], f[SDM_CHEM_N_GAS];
  load_eq(eq, cell_id[i], e);
  chem_drop_data(k.v, e, pH[i], f);
#pragma unroll
  for (int g = 0; g < SDM_CHEM_N_GAS; ++g) df.p[g][i] = f[g];
}

__global__ void __launch_bounds__(SDM_BLOCK)
k_chem_equilibrate(int64_t n_sd, const int64_t *__restrict__ cell_id, Ptr5 conc, Ptr7 eq,
                   double *__restrict__ pH, uint8_t *__restrict__ flag, int64_t *n_failed,
                   double H_min, double H_max, double threshold, double rtol, ChemK k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t failed = 0;
  if (i < n_sd) {
    double e[SDM_CHEM_N_EQ];
    load_eq(eq, cell_id[i], e);
    chem_acid q;
    chem_acid_of(k.v, e, &q);
    q.N_mIII = conc.p[SDM_CHEM_CONC_N_MIII][i];
    q.N_V = conc.p[SDM_CHEM_CONC_N_V][i];
    q.C_IV = conc.p[SDM_CHEM_CONC_C_IV][i];
    q.S_IV = conc.p[SDM_CHEM_CONC_S_IV][i];
    q.S_VI = conc.p[SDM_CHEM_CONC_S_VI][i];
    const double before = pH[i];
    double now = before;
    int f = 2;  // (2: the row was left alone)
    failed = chem_equilibrate_row(&q, H_min, H_max, threshold, rtol, &now, &f);
    if (f != 2) {
      pH[i] = now;
      flag[i] = (uint8_t)f;
    }
  }
  count_add(n_failed, failed);
}

// lane per position q of idx; the cell by bisection of cell_start
__global__ void __launch_bounds__(SDM_BLOCK)
k_chem_dissolve(int64_t n_sd, int64_t n_cell, const int64_t *__restrict__ idx,
                const int64_t *__restrict__ cell_start, const uint8_t *__restrict__ flag,
                Ptr6 moles, Ptr6 mr, const double *__restrict__ T, const double *__restrict__ p,
                Ptr6 henry, Ptr6 df, const double *__restrict__ volume,
                const int64_t *__restrict__ multiplicity, double dt, double *__restrict__ dq,
                int64_t *n_negative, ChemK k) {
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t negative = 0;
  if (q < n_sd && q >= cell_start[0] && q < cell_start[n_cell]) {
    const int64_t i = idx[q];
    if (i >= 0 && i < n_sd && flag[i]) {
      const int64_t c = find_cell(cell_start, n_cell, q);
      const double env_T = T[c], env_p = p[c], vol = volume[i];
      const double mult = (double)multiplicity[i];
#pragma unroll
      for (int g = 0; g < SDM_CHEM_N_GAS; ++g) {
        const double old = moles.p[g][i];
        const double now = chem_dissolution_row(k.v, g, mr.p[g][c], henry.p[g][c], env_p, env_T,
                                                dt, vol, old, df.p[g][i]);
        negative += !(now >= 0);
        if (dq) dq[(int64_t)g * n_sd + i] = mult * (now - old);
        moles.p[g][i] = now;
      }
    }
  }
  count_add(n_negative, negative);
}

__global__ void __launch_bounds__(SDM_BLOCK)
k_chem_oxidize(int64_t n_sd, const int64_t *__restrict__ cell_id,
               const uint8_t *__restrict__ flag, Ptr4 kin, Ptr7 eq, double dt,
               const double *__restrict__ volume, const double *__restrict__ pH,
               const double *__restrict__ df_SO2, double *__restrict__ m_O3,
               double *__restrict__ m_H2O2, double *__restrict__ m_S_IV,
               double *__restrict__ m_S_VI, ChemK k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n_sd || !flag[i]) return;
  const int64_t c = cell_id[i];
  double e[SDM_CHEM_N_EQ] = {0, 0, 0, 0, 0, 0, 0}, kn[SDM_CHEM_N_KIN];
  e[SDM_CHEM_EQ_SO2] = eq.p[SDM_CHEM_EQ_SO2][c];  // (the two the step reads: the header)
  e[SDM_CHEM_EQ_HSO3] = eq.p[SDM_CHEM_EQ_HSO3][c];
#pragma unroll
  for (int j = 0; j < SDM_CHEM_N_KIN; ++j) kn[j] = kin.p[j][c];
  double o3 = m_O3[i], h2o2 = m_H2O2[i], s4 = m_S_IV[i], s6 = m_S_VI[i];
  chem_oxidation_row(k.v, kn, e, dt, volume[i], pH[i], df_SO2[i], &o3, &h2o2, &s4, &s6);
  m_O3[i] = o3;
  m_H2O2[i] = h2o2;
  m_S_IV[i] = s4;
  m_S_VI[i] = s6;
}

// ---- the sums of a closed system ------------------------------------------------------------------
// one workgroup per cell; took[i] != 0: row i took part and dq[g * n_sd + i] is its contribution
template <bool BLOCKED>
__global__ void __launch_bounds__(CHEM_SB)
k_chem_sum(int64_t n_sd, const int64_t *__restrict__ idx, const int64_t *__restrict__ cell_start,
           const uint8_t *__restrict__ took, const double *__restrict__ dq, Ptr6 mr,
           const double *__restrict__ rhod, double dv, int64_t *n_exceeded, ChemK k) {
  __shared__ double a[SDM_CHEM_N_GAS][2 * CHEM_SB];
  __shared__ int wave_count[CHEM_SB / SDM_WAVE];
  const int64_t c = blockIdx.x;
  const int64_t begin = cell_start[c], end = cell_start[c + 1];
  const int tid = threadIdx.x;
  double acc = 0.0;      // lanes 0..5: the gas tid
  int64_t n_took = 0;    // uniform over the workgroup
  int fill = 0;          // BLOCKED: compacted entries waiting in `a` (uniform)
  // `a[g][0..256)` reduced to a[g][0] in the header's shape, added to the accumulators
  auto reduce_block = [&](int len) {
    for (int h = CHEM_SB / 2; h >= 1; h /= 2) {
      if (tid < h && tid + h < len) {
#pragma unroll
        for (int g = 0; g < SDM_CHEM_N_GAS; ++g) a[g][tid] += a[g][tid + h];
      }
      __syncthreads();
    }
    if (tid < SDM_CHEM_N_GAS) acc += a[tid][0];
    __syncthreads();
  };
  for (int64_t base = begin; base < end; base += CHEM_SB) {
    const int64_t q = base + tid;
    int64_t i = -1;
    bool in = false;
    if (q < end) {
      i = idx[q];
      in = i >= 0 && i < n_sd && took[i] != 0;
    }
    double v[SDM_CHEM_N_GAS];
#pragma unroll
    for (int g = 0; g < SDM_CHEM_N_GAS; ++g) v[g] = in ? dq[(int64_t)g * n_sd + i] : 0.0;
    // position of this lane among the chunk's rows that took part
    const unsigned long long ballot = __ballot(in);
    const int wave = tid / SDM_WAVE;
    if (lane_id() == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, chunk_took = 0;
#pragma unroll
    for (int w = 0; w < CHEM_SB / SDM_WAVE; ++w) {
      if (w < wave) before += wave_count[w];
      chunk_took += wave_count[w];
    }
    before += __popcll(ballot & ((1ull << lane_id()) - 1));
    n_took += chunk_took;
    if (!BLOCKED) {
#pragma unroll
      for (int g = 0; g < SDM_CHEM_N_GAS; ++g) a[g][tid] = v[g];
      __syncthreads();
      if (tid < SDM_CHEM_N_GAS) {
        const int stop = (int)(end - base < CHEM_SB ? end - base : CHEM_SB);
        for (int j = 0; j < stop; ++j) acc += a[tid][j];
      }
      __syncthreads();
    } else {
      if (in) {
#pragma unroll
        for (int g = 0; g < SDM_CHEM_N_GAS; ++g) a[g][fill + before] = v[g];
      }
      fill += chunk_took;
      __syncthreads();
      if (fill >= CHEM_SB) {
        // the entries past the block are kept in registers over the destructive reduction
        double keep[SDM_CHEM_N_GAS];
        const int rest = fill - CHEM_SB;
#pragma unroll
        for (int g = 0; g < SDM_CHEM_N_GAS; ++g) keep[g] = tid < rest ? a[g][CHEM_SB + tid] : 0.0;
        reduce_block(CHEM_SB);
        if (tid < rest) {
#pragma unroll
          for (int g = 0; g < SDM_CHEM_N_GAS; ++g) a[g][tid] = keep[g];
        }
        fill = rest;
        __syncthreads();
      }
    }
  }
  if (BLOCKED && fill > 0) reduce_block(fill);
  int64_t exceeded = 0;
  if (tid < SDM_CHEM_N_GAS && n_took > 0) {
    const double delta = chem_delta_mr(k.v, tid, acc, dv, rhod[c]);
    const double before = mr.p[tid][c];
    exceeded = !(delta <= before);
    mr.p[tid][c] = before - delta;
  }
  if (tid < SDM_WAVE) count_add(n_exceeded, exceeded);
}

// ---- the fused step -------------------------------------------------------------------------------
struct StepArgs {
  int64_t n_sd, n_cell;
  const int64_t *cell_id, *multiplicity;
  const double *volume, *T, *p;
  Ptr7 moles;
  Ptr6 mr;
  double *pH;
  uint8_t *flag;
  double *dq;       // closed system: [6][n_sd]
  uint8_t *took;    // closed system
  int64_t *counts;  // may be NULL
  int n_sub;
  double dt, H_min, H_max, threshold, rtol;
  ChemK k;
};

// what a row reads of its cell: the 17 constants, the six mixing ratios, T and p
struct CellRec {
  chem_cell c;
  double mr[SDM_CHEM_N_GAS], T, p;
};

DF void cell_rec(const StepArgs &s, int64_t c, CellRec *r) {
  r->T = s.T[c];
  r->p = s.p[c];
  chem_cell_data(s.k.v, r->T, &r->c);
#pragma unroll
  for (int g = 0; g < SDM_CHEM_N_GAS; ++g) r->mr[g] = s.mr.p[g][c];
}

// PER_CELL: the records of ALL cells (n_cell <= SDM_CHEM_LDS_CELLS) are evaluated once per
// workgroup into LDS, one cell per lane, before the rows start - one barrier, none inside the
// divergent loop - and a row reads its cell's values from there where it uses them instead of
// carrying 25 doubles in registers.  Otherwise every row evaluates its own record.  The same
// functions either way: the same bits.
template <bool PER_CELL>
__global__ void __launch_bounds__(SDM_BLOCK) k_chem_step(StepArgs s) {
  __shared__ CellRec table[PER_CELL ? SDM_CHEM_LDS_CELLS : 1];
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (PER_CELL) {
    for (int64_t c = threadIdx.x; c < s.n_cell; c += SDM_BLOCK) cell_rec(s, c, &table[c]);
    __syncthreads();
  }
  int64_t counts[2] = {0, 0};
  if (i < s.n_sd) {
    const int64_t c = s.cell_id[i];
    if (c >= 0 && c < s.n_cell) {
      CellRec own;
      if (!PER_CELL) cell_rec(s, c, &own);
      const CellRec *rec = PER_CELL ? &table[c] : &own;
      chem_drop d;
#pragma unroll
      for (int a = 0; a < SDM_CHEM_N_AQ; ++a) d.m[a] = s.moles.p[a][i];
      d.pH = s.pH[i];
      d.flag = s.flag[i] != 0;
      d.volume = s.volume[i];
      const double mult = (double)s.multiplicity[i];
#pragma unroll 1
      for (int half = 0; half < 2 * s.n_sub; ++half) {
        double dq[SDM_CHEM_N_GAS];
        int took = 0;
        chem_half(s.k.v, &rec->c, rec->mr, rec->p, rec->T, s.dt, s.H_min, s.H_max, s.threshold,
                  s.rtol, mult, &d, half & 1, dq, &took, counts);
        if (s.dq && (half & 1) == 0) {  // (closed system: n_sub is 1)
          s.took[i] = (uint8_t)took;
          if (took) {
#pragma unroll
            for (int g = 0; g < SDM_CHEM_N_GAS; ++g) s.dq[(int64_t)g * s.n_sd + i] = dq[g];
          }
        }
      }
#pragma unroll
      for (int a = 0; a < SDM_CHEM_N_AQ; ++a) s.moles.p[a][i] = d.m[a];
      s.pH[i] = d.pH;
      s.flag[i] = (uint8_t)d.flag;
    } else if (s.took) {
      s.took[i] = 0;  // (a row without a cell takes no part in the sums)
    }
  }
  count_add(s.counts ? s.counts + 0 : nullptr, counts[0]);
  count_add(s.counts ? s.counts + 1 : nullptr, counts[1]);
}

bool cfg_ok(const sdm_chemistry_cfg *cfg) {
  return cfg &&
         (cfg->system_type == SDM_CHEM_SYSTEM_OPEN || cfg->system_type == SDM_CHEM_SYSTEM_CLOSED) &&
         (cfg->sum == SDM_CHEM_SUM_ORDERED || cfg->sum == SDM_CHEM_SUM_BLOCKED) &&
         cfg->constants >= SDM_CHEM_CONSTS_AUTO && cfg->constants <= SDM_CHEM_CONSTS_PER_CELL;
}

int launch_sum(sdm_ctx *ctx, const sdm_chemistry_cfg *cfg, int64_t n_sd, int64_t n_cell,
               const int64_t *idx, const int64_t *cell_start, const uint8_t *took,
               const double *dq, const Ptr6 &mr, const double *rhod, int64_t *n_exceeded,
               const ChemK &k) {
  if (cfg->sum == SDM_CHEM_SUM_BLOCKED)
    hipLaunchKernelGGL(k_chem_sum<true>, dim3((unsigned)n_cell), dim3(CHEM_SB), 0, ctx->stream,
                       n_sd, idx, cell_start, took, dq, mr, rhod, cfg->cell_volume, n_exceeded, k);
  else
    hipLaunchKernelGGL(k_chem_sum<false>, dim3((unsigned)n_cell), dim3(CHEM_SB), 0, ctx->stream,
                       n_sd, idx, cell_start, took, dq, mr, rhod, cfg->cell_volume, n_exceeded, k);
  LAUNCH_CHECK();
  return SDM_OK;
}

}  // namespace

extern "C" int sdm_chem_recalculate_cell_data(sdm_ctx *ctx, int64_t n_cell, const double *T,
                                              double *const equilibrium[7],
                                              double *const kinetic[4], double *const henry[6],
                                              const double consts[62]) {
  ARG_TRY(ctx && consts && n_cell >= 0);
  if (n_cell == 0) return SDM_OK;
  Ptr7 eq;
  Ptr4 kin;
  Ptr6 hen;
  ARG_TRY(T && take(eq, equilibrium, 7) && take(kin, kinetic, 4) && take(hen, henry, 6));
  hipLaunchKernelGGL(k_chem_cells, dim3(grid_for(n_cell)), dim3(SDM_BLOCK), 0, ctx->stream, n_cell,
                     T, eq, kin, hen, consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_chem_recalculate_drop_data(sdm_ctx *ctx, int64_t n_sd, const double *pH,
                                              const int64_t *cell_id,
                                              const double *const equilibrium[7],
                                              double *const dissociation_factors[6],
                                              const double consts[62]) {
  ARG_TRY(ctx && consts && n_sd >= 0);
  if (n_sd == 0) return SDM_OK;
  Ptr7 eq;
  Ptr6 df;
  ARG_TRY(pH && cell_id && take(eq, equilibrium, 7) && take(df, dissociation_factors, 6));
  hipLaunchKernelGGL(k_chem_drops, dim3(grid_for(n_sd)), dim3(SDM_BLOCK), 0, ctx->stream, n_sd, pH,
                     cell_id, eq, df, consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_equilibrate_H(sdm_ctx *ctx, const sdm_chemistry_cfg *cfg, int64_t n_sd,
                                 const int64_t *cell_id, const double *const conc[5],
                                 const double *const equilibrium[7], double *pH,
                                 uint8_t *do_chemistry_flag, int64_t *n_failed,
                                 const double consts[62]) {
  ARG_TRY(ctx && cfg && consts && n_sd >= 0);
  if (n_failed) HIP_TRY(hipMemsetAsync(n_failed, 0, sizeof(int64_t), ctx->stream));
  if (n_sd == 0) return SDM_OK;
  Ptr5 cn;
  Ptr7 eq;
  ARG_TRY(cell_id && pH && do_chemistry_flag && take(cn, conc, 5) && take(eq, equilibrium, 7));
  hipLaunchKernelGGL(k_chem_equilibrate, dim3(grid_for(n_sd)), dim3(SDM_BLOCK), 0, ctx->stream,
                     n_sd, cell_id, cn, eq, pH, do_chemistry_flag, n_failed, cfg->H_min, cfg->H_max,
                     cfg->ionic_strength_threshold, cfg->rtol, consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_dissolution(sdm_ctx *ctx, const sdm_chemistry_cfg *cfg, int64_t n_sd,
                               int64_t n_cell, const int64_t *idx, const int64_t *cell_start,
                               const uint8_t *do_chemistry_flag, double *const moles[6],
                               double *const env_mixing_ratio[6], const double *T, const double *p,
                               const double *rhod, const double *const henry[6],
                               const double *const dissociation_factors[6], const double *volume,
                               const int64_t *multiplicity, int64_t *n_negative,
                               int64_t *n_exceeded, const double consts[62]) {
  ARG_TRY(ctx && consts && cfg_ok(cfg) && n_sd >= 0 && n_cell >= 1 && n_cell < 0x7fffffff);
  if (n_negative) HIP_TRY(hipMemsetAsync(n_negative, 0, sizeof(int64_t), ctx->stream));
  if (n_exceeded) HIP_TRY(hipMemsetAsync(n_exceeded, 0, sizeof(int64_t), ctx->stream));
  if (n_sd == 0) return SDM_OK;
  Ptr6 mo, mr, hen, df;
  ARG_TRY(idx && cell_start && do_chemistry_flag && T && p && rhod && volume && multiplicity &&
          take(mo, moles, 6) && take(mr, env_mixing_ratio, 6) && take(hen, henry, 6) &&
          take(df, dissociation_factors, 6));
  const bool closed = cfg->system_type == SDM_CHEM_SYSTEM_CLOSED;
  double *dq = nullptr;
  if (closed) {
    const int rc = sdm_reserve(ctx, carve_size(sizeof(double) * 6 * (size_t)n_sd));
    if (rc) return rc;
    dq = (double *)ctx->arena;
  }
  const ChemK k = consts_of(consts);
  hipLaunchKernelGGL(k_chem_dissolve, dim3(grid_for(n_sd)), dim3(SDM_BLOCK), 0, ctx->stream, n_sd,
                     n_cell, idx, cell_start, do_chemistry_flag, mo, mr, T, p, hen, df, volume,
                     multiplicity, cfg->timestep, dq, n_negative, k);
  LAUNCH_CHECK();
  if (!closed) return SDM_OK;
  return launch_sum(ctx, cfg, n_sd, n_cell, idx, cell_start, do_chemistry_flag, dq, mr, rhod,
                    n_exceeded, k);
}

extern "C" int sdm_oxidation(sdm_ctx *ctx, int64_t n_sd, const int64_t *cell_id,
                             const uint8_t *do_chemistry_flag, const double *const kinetic[4],
                             const double *const equilibrium[7], double timestep,
                             const double *volume, const double *pH,
                             const double *dissociation_factor_SO2, double *moles_O3,
                             double *moles_H2O2, double *moles_S_IV, double *moles_S_VI,
                             const double consts[62]) {
  ARG_TRY(ctx && consts && n_sd >= 0);
  if (n_sd == 0) return SDM_OK;
  Ptr4 kin;
  Ptr7 eq;
  ARG_TRY(cell_id && do_chemistry_flag && volume && pH && dissociation_factor_SO2 && moles_O3 &&
          moles_H2O2 && moles_S_IV && moles_S_VI && take(kin, kinetic, 4) &&
          take(eq, equilibrium, 7));
  hipLaunchKernelGGL(k_chem_oxidize, dim3(grid_for(n_sd)), dim3(SDM_BLOCK), 0, ctx->stream, n_sd,
                     cell_id, do_chemistry_flag, kin, eq, timestep, volume, pH,
                     dissociation_factor_SO2, moles_O3, moles_H2O2, moles_S_IV, moles_S_VI,
                     consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_chemistry_step(sdm_ctx *ctx, const sdm_chemistry_cfg *cfg, int64_t n_sd,
                                  int64_t n_cell, const int64_t *idx, const int64_t *cell_start,
                                  const int64_t *cell_id, const int64_t *multiplicity,
                                  const double *volume, double *const moles[7], double *pH,
                                  uint8_t *do_chemistry_flag, const double *T, const double *p,
                                  const double *rhod, double *const env_mixing_ratio[6],
                                  int64_t *counts, const double consts[62]) {
  ARG_TRY(ctx && consts && cfg_ok(cfg) && n_sd >= 0 && n_cell >= 1 && n_cell < 0x7fffffff);
  ARG_TRY(cfg->n_substep >= 1);
  if (counts) HIP_TRY(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), ctx->stream));
  if (n_sd == 0) return SDM_OK;
  StepArgs s;
  ARG_TRY(idx && cell_start && cell_id && multiplicity && volume && pH && do_chemistry_flag && T &&
          p && rhod && take(s.moles, moles, 7) && take(s.mr, env_mixing_ratio, 6));
  const bool closed = cfg->system_type == SDM_CHEM_SYSTEM_CLOSED;
  s.dq = nullptr;
  s.took = nullptr;
  if (closed) {
    const size_t dq_bytes = carve_size(sizeof(double) * 6 * (size_t)n_sd);
    const int rc = sdm_reserve(ctx, dq_bytes + carve_size((size_t)n_sd));
    if (rc) return rc;
    Carver cv(ctx->arena);
    s.dq = cv.take<double>(6 * (size_t)n_sd);
    s.took = cv.take<uint8_t>((size_t)n_sd);
  }
  s.n_sd = n_sd;
  s.n_cell = n_cell;
  s.cell_id = cell_id;
  s.multiplicity = multiplicity;
  s.volume = volume;
  s.T = T;
  s.p = p;
  s.pH = pH;
  s.flag = do_chemistry_flag;
  s.counts = counts;
  s.dt = cfg->timestep / cfg->n_substep;
  s.H_min = cfg->H_min;
  s.H_max = cfg->H_max;
  s.threshold = cfg->ionic_strength_threshold;
  s.rtol = cfg->rtol;
  s.k = consts_of(consts);
  s.n_sub = closed ? 1 : cfg->n_substep;
  const int launches = closed ? cfg->n_substep : 1;
  ARG_TRY(cfg->constants != SDM_CHEM_CONSTS_PER_CELL || n_cell <= SDM_CHEM_LDS_CELLS);
  // SDM_CHEM_CONSTS_AUTO: see the header
  const bool per_cell = cfg->constants == SDM_CHEM_CONSTS_PER_CELL ||
                        (cfg->constants == SDM_CHEM_CONSTS_AUTO && SDM_CHEM_AUTO_PER_CELL &&
                         n_cell <= SDM_CHEM_LDS_CELLS);
  for (int l = 0; l < launches; ++l) {
    if (per_cell)
      hipLaunchKernelGGL(k_chem_step<true>, dim3(grid_for(n_sd)), dim3(SDM_BLOCK), 0, ctx->stream,
                         s);
    else
      hipLaunchKernelGGL(k_chem_step<false>, dim3(grid_for(n_sd)), dim3(SDM_BLOCK), 0,
                         ctx->stream, s);
    LAUNCH_CHECK();
    if (closed) {
      const int rc = launch_sum(ctx, cfg, n_sd, n_cell, idx, cell_start, s.took, s.dq, s.mr, rhod,
                                counts ? counts + 2 : nullptr, s.k);
      if (rc) return rc;
    }
  }
  return SDM_OK;
}

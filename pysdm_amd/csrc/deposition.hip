// deposition.hip -- vapour deposition on ice (include/sdm_deposition.h): PySDM's
// `VapourDepositionOnIce` dynamic
//
// Reference: PySDM/backends/impl_numba/methods/deposition_methods.py ("dm.py" below), with the
// formulae it calls: physics/particle_shape_and_density/mixed_phase_spheres.py (mass_to_radius),
// diffusion_ice_capacity/, diffusion_ice_kinetics/, diffusion_thermics/neglect.py,
// latent_heat_sublimation/murphy_koop_2005.py, saturation_vapour_pressure/flatau_walko_cotton.py
// (pvs_ice), drop_growth/{fick,howell_1949,mason_1971}.py, diffusion_coordinate/ and
// state_variable_triplet/libcloudphplusplus.py (dthd_dt).  Python evaluates left to right; every
// expression keeps that order, nothing is contracted (-ffp-contract=off), and pow / exp / log are
// csrc/sdm_math.h, which the CPU checker compiles too.
//
// The reference is one serial loop over the rows that adds each ice particle's contribution to
// two per-cell sums.  Here:
//   k_dep_cells   one thread per cell: what depends on the cell only (S_ice, pvs_ice, ls, the
//                 lambdas, every cell-only prefix of the row's left-to-right expressions) into a
//                 128-byte record of the arena - for any number of cells
//   k_dep_rows    streaming, a thread owns 4 consecutive rows: new mass, the row's two
//                 contributions, the sort key (its cell if it contributes, else the extra key
//                 n_cell) and the identity permutation
//   the project's stable counting sort (index.hip) over the identity permutation by that key:
//                 per cell the CONTRIBUTING rows in ascending row order, nothing else - so the sums
//                 never see a row to skip, and a block of the blocked sum is 256 consecutive
//                 entries.  (Also with one cell: the sort then drops the rows that do not
//                 contribute, which the blocked shape is defined over.)
//   k_dep_walk    one workgroup per cell: acc = predicted[c], the lanes stage 1024 contributions at
//                 a time in LDS (the next chunk's loads are in flight during the walk), lane 0
//                 adds them serially, two independent chains - the reference's bits
//   blocked sum:  k_dep_blocks reduces one block per workgroup in the fixed tree shape of the
//                 header, k_dep_walk then adds the block values in block order
// No atomics on doubles anywhere; n_exceeded is an integer count, one atomic per wave.
#include "common.h"
#include "index.h"
#include "deposition_rows.h"

#define DEP_ELEMS 4   // consecutive rows per thread of k_dep_rows
#define DEP_CH 1024   // contributions staged per chunk of the serial walk
#define DEP_CR (DEP_CH / SDM_BLOCK)

namespace {

// ---- per cell ------------------------------------------------------------------------------------
// (the record and the row code: deposition_rows.h, which the mixed-phase parcel compiles too)
__global__ void __launch_bounds__(SDM_BLOCK) k_dep_cells(DepArgs g) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c == 0) g.p_len[0] = g.n_sd;
  if (c <= g.n_cell) g.cidx[c] = c;  // the sort's cell_idx: identity over n_cell + 1 keys
  if (c >= g.n_cell) return;
  dep_cell_record(g, g.dv, g.T[c], g.p[c], g.RH[c], g.a_w_ice[c], g.qv[c], g.rhod[c], g.thd[c],
                  g.cv + c * DEP_CV);
}

// DEP_ELEMS consecutive values of a column, 16-byte loads where the thread's run is whole and
// aligned (as freezing.hip: load_run)
template <typename T2, typename T1>
DF void load_run(const T1 *__restrict__ p, int64_t first, int64_t n, T1 out[DEP_ELEMS]) {
  static_assert(DEP_ELEMS == 4 && sizeof(T2) == 2 * sizeof(T1), "two 16-byte loads per run");
  if (first + DEP_ELEMS <= n && (((uintptr_t)(p + first)) & 15) == 0) {
    const T2 a = ((const T2 *)(p + first))[0], b = ((const T2 *)(p + first))[1];
    out[0] = a.x; out[1] = a.y; out[2] = b.x; out[3] = b.y;
  } else {
#pragma unroll
    for (int e = 0; e < DEP_ELEMS; ++e) out[e] = first + e < n ? p[first + e] : (T1)0;
  }
}

// (the arena pieces are 256-byte aligned and `first` is a multiple of DEP_ELEMS)
DF void store_run(int64_t *__restrict__ p, int64_t first, int64_t n,
                  const int64_t v[DEP_ELEMS]) {
  if (first + DEP_ELEMS <= n) {
    ((longlong2 *)(p + first))[0] = make_longlong2(v[0], v[1]);
    ((longlong2 *)(p + first))[1] = make_longlong2(v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < DEP_ELEMS; ++e)
      if (first + e < n) p[first + e] = v[e];
  }
}

__global__ void __launch_bounds__(SDM_BLOCK) k_dep_rows(DepArgs g) {
  const int64_t first =
      ((int64_t)blockIdx.x * SDM_BLOCK + (int64_t)threadIdx.x) * DEP_ELEMS;
  int64_t n_exceeded = 0;
  if (first < g.n_sd) {
    double m[DEP_ELEMS];
    int64_t cell[DEP_ELEMS], mult[DEP_ELEMS], key[DEP_ELEMS], ident[DEP_ELEMS];
    load_run<double2>(g.m, first, g.n_sd, m);
    load_run<longlong2>((const long long *)g.cell, first, g.n_sd, (long long *)cell);
    load_run<longlong2>((const long long *)g.multiplicity, first, g.n_sd, (long long *)mult);
#pragma unroll
    for (int e = 0; e < DEP_ELEMS; ++e) {
      const int64_t i = first + e;
      ident[e] = i;
      key[e] = g.n_cell;
      // dm.py:42 `not unfrozen`: m > 0 is liquid
      if (i >= g.n_sd || m[e] > 0 || cell[e] < 0 || cell[e] >= g.n_cell) continue;
      const double *cv = g.cv + cell[e] * DEP_CV;
      if (cv[CV_S] == 1) continue;  // dm.py:79-80
      double m_new, dq, dth;
      n_exceeded += dep_row(g, cv, m[e], mult[e], &m_new, &dq, &dth) ? 1 : 0;
      key[e] = cell[e];
      g.m[i] = m_new;
      g.dq[i] = dq;
      g.dth[i] = dth;
    }
    store_run(g.key, first, g.n_sd, key);
    store_run(g.ident, first, g.n_sd, ident);
  }
  if (g.n_exceeded) {  // (uniform: every lane of the wave gets here)
    const int64_t s = wave_sum_i64(n_exceeded);
    if (lane_id() == 0 && s != 0)
      atomicAdd((unsigned long long *)g.n_exceeded, (unsigned long long)s);
  }
}

// ---- the sums ------------------------------------------------------------------------------------
// one workgroup per segment c of `start` (a cell's sorted rows, or a cell's blocks): acc =
// predicted[c], then the segment's values one by one.  GATHER: value of position q is v[rows[q]]
template <bool GATHER>
__global__ void __launch_bounds__(SDM_BLOCK)
k_dep_walk(const int64_t *__restrict__ start, const int64_t *__restrict__ rows,
           const double *__restrict__ vq, const double *__restrict__ vt,
           double *__restrict__ predicted_qv, double *__restrict__ predicted_thd) {
  __shared__ double sq[DEP_CH], st[DEP_CH];
  const int64_t c = blockIdx.x;
  const int64_t begin = start[c], end = start[c + 1];
  if (end <= begin) return;  // nothing contributes: the predicted values keep their bits
  const int tid = threadIdx.x;
  double accq = 0, acct = 0;
  if (tid == 0) {
    accq = predicted_qv[c];
    acct = predicted_thd[c];
  }
  double rq[DEP_CR], rt[DEP_CR];
  auto fetch = [&](int64_t base) {
#pragma unroll
    for (int s = 0; s < DEP_CR; ++s) {
      const int64_t q = base + tid + s * SDM_BLOCK;
      rq[s] = rt[s] = 0.0;
      if (q < end) {
        const int64_t at = GATHER ? rows[q] : q;
        rq[s] = vq[at];
        rt[s] = vt[at];
      }
    }
  };
  fetch(begin);
  for (int64_t base = begin; base < end; base += DEP_CH) {
#pragma unroll
    for (int s = 0; s < DEP_CR; ++s) {
      sq[tid + s * SDM_BLOCK] = rq[s];
      st[tid + s * SDM_BLOCK] = rt[s];
    }
    __syncthreads();
    if (base + DEP_CH < end) fetch(base + DEP_CH);  // in flight during the walk
    if (tid == 0) {
      const int stop = (int)(end - base < DEP_CH ? end - base : DEP_CH);
      int q = 0;
      for (; q + 16 <= stop; q += 16) {  // loads issued ahead of the adds (as condensation.hip)
        double a[16], b[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          a[j] = sq[q + j];
          b[j] = st[q + j];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          accq += a[j];
          acct += b[j];
        }
      }
      for (; q < stop; ++q) {
        accq += sq[q];
        acct += st[q];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    predicted_qv[c] = accq;
    predicted_thd[c] = acct;
  }
}

__global__ void __launch_bounds__(SDM_BLOCK)
k_dep_block_counts(const int64_t *__restrict__ cell_start, int64_t *__restrict__ count,
                   int64_t n_cell) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c < n_cell)
    count[c] = (cell_start[c + 1] - cell_start[c] + SDM_DEP_SUM_BLOCK - 1) / SDM_DEP_SUM_BLOCK;
}

// workgroup g reduces block g (block_start: first block of every cell) in the header's shape
__global__ void __launch_bounds__(SDM_DEP_SUM_BLOCK)
k_dep_blocks(const int64_t *__restrict__ cell_start, const int64_t *__restrict__ block_start,
             int64_t n_cell, const int64_t *__restrict__ rows, const double *__restrict__ dq,
             const double *__restrict__ dth, double *__restrict__ bq, double *__restrict__ bt) {
  __shared__ double aq[SDM_DEP_SUM_BLOCK], at[SDM_DEP_SUM_BLOCK];
  const int64_t blk = blockIdx.x;
  if (blk >= block_start[n_cell]) return;
  const int64_t c = find_cell(block_start, n_cell, blk);
  const int64_t pos = cell_start[c] + (blk - block_start[c]) * SDM_DEP_SUM_BLOCK;
  const int64_t left = cell_start[c + 1] - pos;
  const int len = (int)(left < SDM_DEP_SUM_BLOCK ? left : SDM_DEP_SUM_BLOCK);
  const int j = threadIdx.x;
  if (j < len) {
    const int64_t row = rows[pos + j];
    aq[j] = dq[row];
    at[j] = dth[row];
  }
  __syncthreads();
  for (int h = SDM_DEP_SUM_BLOCK / 2; h >= 1; h /= 2) {
    if (j < h && j + h < len) {
      aq[j] += aq[j + h];
      at[j] += at[j + h];
    }
    __syncthreads();
  }
  if (j == 0) {
    bq[blk] = aq[0];
    bt[blk] = at[0];
  }
}

}  // namespace

extern "C" int sdm_deposition(sdm_ctx *ctx, const sdm_deposition_cfg *cfg, int64_t n_sd,
                              int64_t n_cell, const int64_t *multiplicity,
                              double *signed_water_mass, const int64_t *cell_id, const double *T,
                              const double *p, const double *RH, const double *a_w_ice,
                              const double *qv, const double *rhod, const double *thd,
                              double *predicted_qv, double *predicted_thd, int64_t *n_exceeded,
                              const double consts[39]) {
  ARG_TRY(ctx && cfg && consts && n_sd >= 0 && n_cell >= 1 && n_cell < 0x7fffffff);
  ARG_TRY(cfg->coordinate == SDM_DEP_COORD_WATER_MASS_LOGARITHM ||
          cfg->coordinate == SDM_DEP_COORD_WATER_MASS);
  ARG_TRY(cfg->capacity == SDM_DEP_CAPACITY_SPHERICAL ||
          cfg->capacity == SDM_DEP_CAPACITY_COLUMNAR);
  ARG_TRY(cfg->kinetics == SDM_DEP_KINETICS_STANDARD ||
          cfg->kinetics == SDM_DEP_KINETICS_NEGLECT);
  ARG_TRY(cfg->sum == SDM_DEP_SUM_ORDERED || cfg->sum == SDM_DEP_SUM_BLOCKED);
  // (the reference's loop over aliased arrays reads values earlier rows changed: not reproduced)
  ARG_TRY(!predicted_qv || (const double *)predicted_qv != qv);
  ARG_TRY(!predicted_thd || (const double *)predicted_thd != thd);
  if (n_sd == 0) return SDM_OK;
  ARG_TRY(multiplicity && signed_water_mass && cell_id && T && p && RH && a_w_ice && qv && rhod &&
          thd && predicted_qv && predicted_thd);
  const int64_t n_key = n_cell + 1;  // key n_cell: the rows that contribute nothing
  const int64_t max_blocks = n_sd / SDM_DEP_SUM_BLOCK + (n_cell < n_sd ? n_cell : n_sd) + 1;
  ARG_TRY(max_blocks < 0x7fffffff);
  const bool blocked = cfg->sum == SDM_DEP_SUM_BLOCKED;
  const size_t sort_bytes = carve_size(sdm_sort_scratch(n_sd, n_key));
  size_t bytes = carve_size(sizeof(double) * DEP_CV * n_cell) + carve_size(8 * n_key) + 256 +
                 5 * carve_size(8 * (size_t)n_sd) + carve_size(8 * (n_key + 1)) + sort_bytes;
  if (blocked)
    bytes += carve_size(8 * n_cell) + carve_size(8 * (n_cell + 1)) + 2 * carve_size(8 * max_blocks);
  int rc = sdm_reserve(ctx, bytes);
  if (rc) return rc;
  Carver cv(ctx->arena);
  DepArgs g;
  g.cv = cv.take<double>((size_t)DEP_CV * n_cell);
  g.cidx = cv.take<int64_t>(n_key);
  g.p_len = cv.take<int64_t>(1);
  g.key = cv.take<int64_t>(n_sd);
  g.ident = cv.take<int64_t>(n_sd);
  int64_t *sorted = cv.take<int64_t>(n_sd);
  g.dq = cv.take<double>(n_sd);
  g.dth = cv.take<double>(n_sd);
  int64_t *cell_start = cv.take<int64_t>(n_key + 1);
  char *sort_scratch = cv.take<char>(sort_bytes);
  g.n_sd = n_sd;
  g.n_cell = n_cell;
  g.multiplicity = multiplicity;
  g.m = signed_water_mass;
  g.cell = cell_id;
  g.T = T; g.p = p; g.RH = RH; g.a_w_ice = a_w_ice; g.qv = qv; g.rhod = rhod; g.thd = thd;
  g.coordinate = cfg->coordinate;
  g.capacity = cfg->capacity;
  g.kinetics = cfg->kinetics;
  g.dt = cfg->time_step;
  g.dv = cfg->cell_volume;
  g.n_exceeded = n_exceeded;
  g.k = dep_consts_of(consts);
  if (n_exceeded) HIP_TRY(hipMemsetAsync(n_exceeded, 0, sizeof(int64_t), ctx->stream));
  hipLaunchKernelGGL(k_dep_cells, dim3(grid_for(n_key)), dim3(SDM_BLOCK), 0, ctx->stream, g);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_dep_rows, dim3(grid_for(n_sd, SDM_BLOCK * DEP_ELEMS)), dim3(SDM_BLOCK), 0,
                     ctx->stream, g);
  LAUNCH_CHECK();
  rc = sdm_counting_sort_async(ctx, sort_scratch, sorted, g.ident, g.key, g.cidx, g.p_len, n_sd,
                               cell_start, n_key);
  if (rc) return rc;
  if (!blocked) {
    hipLaunchKernelGGL(k_dep_walk<true>, dim3((unsigned)n_cell), dim3(SDM_BLOCK), 0, ctx->stream,
                       cell_start, sorted, g.dq, g.dth, predicted_qv, predicted_thd);
    LAUNCH_CHECK();
    return SDM_OK;
  }
  int64_t *block_count = cv.take<int64_t>(n_cell);
  int64_t *block_start = cv.take<int64_t>(n_cell + 1);
  double *bq = cv.take<double>(max_blocks), *bt = cv.take<double>(max_blocks);
  hipLaunchKernelGGL(k_dep_block_counts, dim3(grid_for(n_cell)), dim3(SDM_BLOCK), 0, ctx->stream,
                     cell_start, block_count, n_cell);
  LAUNCH_CHECK();
  rc = sdm_cell_start_from_counts_async(ctx, block_count, block_start, n_cell, g.p_len);
  if (rc) return rc;
  hipLaunchKernelGGL(k_dep_blocks, dim3((unsigned)max_blocks), dim3(SDM_DEP_SUM_BLOCK), 0,
                     ctx->stream, cell_start, block_start, n_cell, sorted, g.dq, g.dth, bq, bt);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_dep_walk<false>, dim3((unsigned)n_cell), dim3(SDM_BLOCK), 0, ctx->stream,
                     block_start, (const int64_t *)nullptr, bq, bt, predicted_qv, predicted_thd);
  LAUNCH_CHECK();
  return SDM_OK;
}

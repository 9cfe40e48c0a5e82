// freezing.hip -- the freezing path (include/sdm_freezing.h): PySDM's `Freezing` dynamic
//
// Reference: PySDM/backends/impl_numba/methods/freezing_methods.py ("fm.py" below),
// impl_numba/methods/physics_methods.py:78-105 ("pm.py"), physics/trivia.py:79-92,158-163,
// physics/{heterogeneous,homogeneous}_ice_nucleation_rate/, physics/saturation_vapour_pressure/
// flatau_walko_cotton.py (pvs_ice), physics/particle_shape_and_density/mixed_phase_spheres.py.
// Python evaluates left to right; every expression keeps that order, nothing is contracted
// (-ffp-contract=off), and pow / exp are csrc/sdm_math.h, which the CPU checker compiles too.
//
// The work is pure streaming: a super-droplet is read, carried through the enabled passes in
// registers and written back only if it changed.  What a pass needs beyond the droplet's own
// columns depends on its cell only: the thaw condition, the saturation conditions and the
// nucleation rate j_het(a_w_ice[c]) / j_hom(T[c], d_a_w_ice[c]).  A cell that cannot freeze has the
// rate NaN: 1 - exp(NaN) is NaN and `rand < NaN` is false, which is what the reference's skipped
// branch does.  k_freezing_step either evaluates the rate for every eligible droplet or, with up
// to 1024 cells, once per cell and workgroup into LDS (same expression, same bits; measured faster
// over that whole range).  The uniform numbers are the NumPy-PCG64 stream evaluated in place
// with k_pcg_fill's construction (ctx.hip): one jump per workgroup, one per thread (through the
// context's ready jumps, common.h), PCG_ELEMS consecutive draws.
#include "common.h"
#include "index.h"
#include "freezing_rows.h"

#define GRID1D(n) dim3(grid_for(n)), dim3(SDM_BLOCK), 0, ctx->stream

namespace {

// ---- stage kernels ---------------------------------------------------------------------------------
__global__ void k_freeze_singular(double *m_, const double *t_fz, const double *T,
                                  const double *RH, const int64_t *cell, int64_t n, int thaw,
                                  double T0) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double tfz = t_fz[i];
  if (tfz == 0) return;  // fm.py:52-53
  double m = m_[i];
  const int64_t c = cell[i];
  if (freeze_singular_row(m, tfz, T[c], RH[c], thaw, T0)) m_[i] = m;
}

__global__ void k_freeze_time_dependent(const double *rand, double *m_, const double *area_,
                                        double dt, const int64_t *cell, const double *a_w_ice,
                                        const double *T, const double *RH, int64_t n, int thaw,
                                        int code, Kf k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double area = area_[i];
  if (area == 0) return;  // fm.py:92-93
  double m = m_[i];
  const int64_t c = cell[i];
  const double rate = m > 0 ? het_rate_of_cell(k, code, RH, a_w_ice, c) : 0.0;  // (as read)
  if (freeze_time_dependent_row(m, area, T[c], rate, dt, rand[i], thaw, k.T0)) m_[i] = m;
}

__global__ void k_freeze_time_dependent_homogeneous(const double *rand, double *m_,
                                                    const double *volume, double dt,
                                                    const int64_t *cell, const double *a_w_ice,
                                                    const double *T, const double *RH_ice,
                                                    int64_t n, int thaw, int code, Kf k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  double m = m_[i];
  const int64_t c = cell[i];
  const double rate = m > 0 ? hom_rate_of_cell(k, code, T, RH_ice, a_w_ice, c) : 0.0;  // (as read)
  if (freeze_homogeneous_row(m, volume[i], T[c], rate, dt, rand[i], thaw, k.T0)) m_[i] = m;
}

__global__ void k_record_freezing_temperatures(double *data, const int64_t *cell_id,
                                               const double *T, const double *m_, int64_t n) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  double d = data[i];
  if (record_one(d, m_[i], T[cell_id[i]])) data[i] = d;
}

__global__ void k_a_w_ice(const double *T, const double *p, const double *RH, const double *qv,
                          double *a_w_ice, double *RH_ice, int64_t n, Kf k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  a_w_ice_of(k, T[i], p[i], RH[i], qv[i], a_w_ice[i], RH_ice[i]);
}

// Python's max(0, x) / min(0, x) and numpy's maximum / minimum agree for every finite x and give
// NaN for NaN in the numpy form; the scalar form max(ZERO_MASS, nan) is 0 - masses are finite
__global__ void k_volume_of_signed_mass(double *volume, const double *mass, int64_t n,
                                        double rho_w, double rho_i) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double m = mass[i];
  volume[i] = (m > 0.0 ? m : 0.0) / rho_w + (m < 0.0 ? m : 0.0) / rho_i;
}

__global__ void k_signed_mass_of_volume(double *mass, const double *volume, int64_t n,
                                        double rho_w, double rho_i) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = volume[i];
  mass[i] = (v > 0.0 ? v : 0.0) * rho_w + (v < 0.0 ? v : 0.0) * rho_i;
}

// ---- the fused step ----------------------------------------------------------------------------------
struct FrzArgs {
  int64_t n_sd, n_cell;
  double *m;
  const double *t_fz, *area, *volume;
  const int64_t *cell;
  double *t_last;
  const double *T, *RH, *a_w_ice, *RH_ice;
  int imm_singular, imm_time_dependent, hom, thaw, j_het, j_hom;
  double dt;
  u128 s_imm, s_hom, inc;  // generator states at the first uniform of each stochastic pass
  const u128 *tab, *aff;
  Kf k;
};

// PCG_ELEMS consecutive values of a column, 16-byte loads where the thread's run is whole and
// aligned (the rows of a thread are 32 contiguous bytes: a wave reads 2 KiB in one piece)
template <typename T2, typename T1>
__device__ __forceinline__ void load_run(const T1 *__restrict__ p, int64_t first, int64_t n,
                                         T1 out[PCG_ELEMS]) {
  static_assert(PCG_ELEMS == 4 && sizeof(T2) == 2 * sizeof(T1), "two 16-byte loads per run");
  if (first + PCG_ELEMS <= n && (((uintptr_t)(p + first)) & 15) == 0) {
    const T2 a = ((const T2 *)(p + first))[0], b = ((const T2 *)(p + first))[1];
    out[0] = a.x; out[1] = a.y; out[2] = b.x; out[3] = b.y;
  } else {
#pragma unroll
    for (int e = 0; e < PCG_ELEMS; ++e) out[e] = first + e < n ? p[first + e] : (T1)0;
  }
}

__device__ __forceinline__ void draw_run(u128 s_blk, const FrzArgs &g, double u[PCG_ELEMS]) {
  static_assert(SDM_BLOCK * PCG_ELEMS <= PCG_AFF_SMALL, "a ready jump for every thread");
  u128 state = pcg_apply(s_blk, g.aff, (int64_t)threadIdx.x * PCG_ELEMS);
  const u128 mult = pcg_mult();
#pragma unroll
  for (int e = 0; e < PCG_ELEMS; ++e) {
    state = state * mult + g.inc;
    u[e] = pcg_output(state);
  }
}

// TABLE: the rates of all cells in LDS (dynamic: 2 * n_cell doubles), else per eligible droplet
template <bool TABLE>
__global__ void __launch_bounds__(SDM_BLOCK) k_freezing_step(FrzArgs g) {
  extern __shared__ double s_rate[];  // [0, n_cell): immersion, [n_cell, 2 n_cell): homogeneous
  __shared__ u128 s_blk[2];
  const int64_t blk_first = (int64_t)blockIdx.x * (SDM_BLOCK * PCG_ELEMS);
  if (g.imm_time_dependent && threadIdx.x == 0)
    s_blk[0] = pcg_jump_fast(g.s_imm, g.tab, g.aff, (uint64_t)blk_first);
  if (g.hom && threadIdx.x == SDM_WAVE)
    s_blk[1] = pcg_jump_fast(g.s_hom, g.tab, g.aff, (uint64_t)blk_first);
  if (TABLE) {
    for (int64_t c = threadIdx.x; c < g.n_cell; c += SDM_BLOCK) {
      if (g.imm_time_dependent) s_rate[c] = het_rate_of_cell(g.k, g.j_het, g.RH, g.a_w_ice, c);
      if (g.hom)
        s_rate[g.n_cell + c] = hom_rate_of_cell(g.k, g.j_hom, g.T, g.RH_ice, g.a_w_ice, c);
    }
  }
  __syncthreads();
  const int64_t first = blk_first + (int64_t)threadIdx.x * PCG_ELEMS;
  if (first >= g.n_sd) return;

  double m[PCG_ELEMS], x[PCG_ELEMS], u[PCG_ELEMS];
  int64_t cell[PCG_ELEMS];
  bool changed[PCG_ELEMS];
  load_run<double2>(g.m, first, g.n_sd, m);
  load_run<longlong2>((const long long *)g.cell, first, g.n_sd, (long long *)cell);
#pragma unroll
  for (int e = 0; e < PCG_ELEMS; ++e) changed[e] = false;

  if (g.imm_singular) {  // fm.py:40-66
    load_run<double2>(g.t_fz, first, g.n_sd, x);
#pragma unroll
    for (int e = 0; e < PCG_ELEMS; ++e) {
      if (first + e >= g.n_sd || x[e] == 0) continue;
      const int64_t c = cell[e];
      if (g.thaw && m[e] < 0 && g.T[c] > g.k.T0) {
        m[e] = -m[e];
        changed[e] = !changed[e];
      } else if (m[e] > 0 && g.RH[c] > 1 && g.T[c] <= x[e]) {
        m[e] = -m[e];
        changed[e] = !changed[e];
      }
    }
  }
  if (g.imm_time_dependent) {  // fm.py:68-111
    load_run<double2>(g.area, first, g.n_sd, x);
    draw_run(s_blk[0], g, u);
#pragma unroll
    for (int e = 0; e < PCG_ELEMS; ++e) {
      if (first + e >= g.n_sd || x[e] == 0) continue;
      const int64_t c = cell[e];
      if (g.thaw && m[e] < 0 && g.T[c] > g.k.T0) {
        m[e] = -m[e];
        changed[e] = !changed[e];
      } else if (m[e] > 0) {
        const double rate =
            TABLE ? s_rate[c] : het_rate_of_cell(g.k, g.j_het, g.RH, g.a_w_ice, c);
        if (nucleates(rate, x[e], g.dt, u[e])) {
          m[e] = -m[e];
          changed[e] = !changed[e];
        }
      }
    }
  }
  if (g.hom) {  // fm.py:113-168
    if (g.volume) load_run<double2>(g.volume, first, g.n_sd, x);
    draw_run(s_blk[1], g, u);
#pragma unroll
    for (int e = 0; e < PCG_ELEMS; ++e) {
      if (first + e >= g.n_sd) continue;
      const int64_t c = cell[e];
      if (g.thaw && m[e] < 0 && g.T[c] > g.k.T0) {
        m[e] = -m[e];
        changed[e] = !changed[e];
      } else if (m[e] > 0) {
        const double rate = TABLE ? s_rate[g.n_cell + c]
                                  : hom_rate_of_cell(g.k, g.j_hom, g.T, g.RH_ice, g.a_w_ice, c);
        // (no column: mixed_phase_spheres.py mass_to_volume of this mass, which is > 0)
        const double v = g.volume ? x[e] : liquid_volume_of(g.k, m[e]);
        if (nucleates(rate, v, g.dt, u[e])) {
          m[e] = -m[e];
          changed[e] = !changed[e];
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < PCG_ELEMS; ++e)
    if (changed[e] && first + e < g.n_sd) g.m[first + e] = m[e];
  if (g.t_last) {  // fm.py:236-260
    load_run<double2>(g.t_last, first, g.n_sd, x);
#pragma unroll
    for (int e = 0; e < PCG_ELEMS; ++e) {
      if (first + e >= g.n_sd) continue;
      if (record_one(x[e], m[e], g.T[cell[e]])) g.t_last[first + e] = x[e];
    }
  }
}

bool known_j_het(int code) { return code == SDM_FRZ_JHET_CONSTANT || code == SDM_FRZ_JHET_ABIFM; }
bool known_j_hom(int code) { return code >= SDM_FRZ_JHOM_CONSTANT && code <= SDM_FRZ_JHOM_KOOPMURRAY2016; }

}  // namespace

extern "C" int sdm_freeze_singular(sdm_ctx *ctx, double *signed_water_mass,
                                   const double *freezing_temperature, const double *temperature,
                                   const double *relative_humidity, const int64_t *cell,
                                   int64_t n_sd, int thaw, const double consts[33]) {
  ARG_TRY(ctx && n_sd >= 0 && consts);
  if (n_sd == 0) return SDM_OK;
  ARG_TRY(signed_water_mass && freezing_temperature && temperature && relative_humidity && cell);
  hipLaunchKernelGGL(k_freeze_singular, GRID1D(n_sd), signed_water_mass, freezing_temperature,
                     temperature, relative_humidity, cell, n_sd, thaw, consts[SDM_FRZ_K_T0]);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_freeze_time_dependent(sdm_ctx *ctx, const double *rand,
                                         double *signed_water_mass,
                                         const double *immersed_surface_area, double timestep,
                                         const int64_t *cell, const double *a_w_ice,
                                         const double *temperature,
                                         const double *relative_humidity, int64_t n_sd, int thaw,
                                         int j_het, const double consts[33]) {
  ARG_TRY(ctx && n_sd >= 0 && consts && known_j_het(j_het));
  if (n_sd == 0) return SDM_OK;
  ARG_TRY(rand && signed_water_mass && immersed_surface_area && cell && temperature &&
          relative_humidity);
  ARG_TRY(a_w_ice || j_het == SDM_FRZ_JHET_CONSTANT);
  hipLaunchKernelGGL(k_freeze_time_dependent, GRID1D(n_sd), rand, signed_water_mass,
                     immersed_surface_area, timestep, cell, a_w_ice, temperature,
                     relative_humidity, n_sd, thaw, j_het, frz_consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_freeze_time_dependent_homogeneous(
    sdm_ctx *ctx, const double *rand, double *signed_water_mass, const double *volume,
    double timestep, const int64_t *cell, const double *a_w_ice, const double *temperature,
    const double *relative_humidity_ice, int64_t n_sd, int thaw, int j_hom,
    const double consts[33]) {
  ARG_TRY(ctx && n_sd >= 0 && consts && known_j_hom(j_hom));
  if (n_sd == 0) return SDM_OK;
  ARG_TRY(rand && signed_water_mass && volume && cell && temperature && relative_humidity_ice);
  ARG_TRY(a_w_ice || j_hom == SDM_FRZ_JHOM_CONSTANT);
  hipLaunchKernelGGL(k_freeze_time_dependent_homogeneous, GRID1D(n_sd), rand, signed_water_mass,
                     volume, timestep, cell, a_w_ice, temperature, relative_humidity_ice, n_sd,
                     thaw, j_hom, frz_consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_record_freezing_temperatures(sdm_ctx *ctx, double *data,
                                                const int64_t *cell_id,
                                                const double *temperature,
                                                const double *signed_water_mass, int64_t n_sd) {
  ARG_TRY(ctx && n_sd >= 0);
  if (n_sd == 0) return SDM_OK;
  ARG_TRY(data && cell_id && temperature && signed_water_mass);
  hipLaunchKernelGGL(k_record_freezing_temperatures, GRID1D(n_sd), data, cell_id, temperature,
                     signed_water_mass, n_sd);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_a_w_ice(sdm_ctx *ctx, const double *T, const double *p, const double *RH,
                           const double *water_vapour_mixing_ratio, double *a_w_ice,
                           double *RH_ice, int64_t n, const double consts[33]) {
  ARG_TRY(ctx && n >= 0 && consts);
  if (n == 0) return SDM_OK;
  ARG_TRY(T && p && RH && water_vapour_mixing_ratio && a_w_ice && RH_ice);
  hipLaunchKernelGGL(k_a_w_ice, GRID1D(n), T, p, RH, water_vapour_mixing_ratio, a_w_ice, RH_ice,
                     n, frz_consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_volume_of_signed_water_mass(sdm_ctx *ctx, double *volume, const double *mass,
                                               int64_t n, const double consts[33]) {
  ARG_TRY(ctx && n >= 0 && consts);
  if (n == 0) return SDM_OK;
  ARG_TRY(volume && mass);
  hipLaunchKernelGGL(k_volume_of_signed_mass, GRID1D(n), volume, mass, n,
                     consts[SDM_FRZ_K_RHO_W], consts[SDM_FRZ_K_RHO_I]);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_signed_water_mass_of_volume(sdm_ctx *ctx, double *mass, const double *volume,
                                               int64_t n, const double consts[33]) {
  ARG_TRY(ctx && n >= 0 && consts);
  if (n == 0) return SDM_OK;
  ARG_TRY(volume && mass);
  hipLaunchKernelGGL(k_signed_mass_of_volume, GRID1D(n), mass, volume, n,
                     consts[SDM_FRZ_K_RHO_W], consts[SDM_FRZ_K_RHO_I]);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_freezing_step(sdm_ctx *ctx, const sdm_freezing_cfg *cfg, uint64_t rng_offset,
                                 int64_t n_sd, int64_t n_cell, double *signed_water_mass,
                                 const double *freezing_temperature,
                                 const double *immersed_surface_area, const double *volume,
                                 const int64_t *cell_id, double *temperature_of_last_freezing,
                                 const double *T, const double *RH, const double *a_w_ice,
                                 const double *RH_ice, const double consts[33]) {
  ARG_TRY(ctx && cfg && consts && n_sd >= 0 && n_cell >= 1);
  FrzArgs g;
  g.imm_singular = cfg->immersion_freezing && cfg->singular;
  g.imm_time_dependent = cfg->immersion_freezing && !cfg->singular;
  g.hom = cfg->homogeneous_freezing != 0;
  g.thaw = cfg->thaw != 0;
  g.j_het = cfg->j_het;
  g.j_hom = cfg->j_hom;
  ARG_TRY(!g.imm_time_dependent || known_j_het(g.j_het));
  ARG_TRY(!g.hom || known_j_hom(g.j_hom));
  ARG_TRY(cfg->rates >= SDM_FRZ_RATES_AUTO && cfg->rates <= SDM_FRZ_RATES_PER_CELL);
  ARG_TRY(cfg->rates != SDM_FRZ_RATES_PER_CELL || n_cell <= SDM_FRZ_RATES_MAX_CELLS);
  const bool any_pass = g.imm_singular || g.imm_time_dependent || g.hom;
  if (n_sd == 0 || (!any_pass && !temperature_of_last_freezing)) return SDM_OK;
  ARG_TRY(signed_water_mass && cell_id && T);
  ARG_TRY(!g.imm_singular || (freezing_temperature && RH));
  ARG_TRY(!g.imm_time_dependent ||
          (immersed_surface_area && RH && (a_w_ice || g.j_het == SDM_FRZ_JHET_CONSTANT)));
  ARG_TRY(!g.hom || (RH_ice && (a_w_ice || g.j_hom == SDM_FRZ_JHOM_CONSTANT)));
  g.n_sd = n_sd;
  g.n_cell = n_cell;
  g.m = signed_water_mass;
  g.t_fz = freezing_temperature;
  g.area = immersed_surface_area;
  g.volume = volume;
  g.cell = cell_id;
  g.t_last = temperature_of_last_freezing;
  g.T = T;
  g.RH = RH;
  g.a_w_ice = a_w_ice;
  g.RH_ice = RH_ice;
  g.dt = cfg->timestep;
  g.k = frz_consts_of(consts);
  g.s_imm = g.s_hom = g.inc = 0;
  g.tab = ctx->pcg_tab;
  g.aff = ctx->pcg_aff;
  const bool stochastic = g.imm_time_dependent || g.hom;
  if (stochastic) {
    int rc = sdm_pcg_prepare(ctx, cfg->rng_state_inc);
    if (rc) return rc;
    const u128 st = (((u128)cfg->rng_state_inc[0]) << 64) | cfg->rng_state_inc[1];
    g.inc = (((u128)cfg->rng_state_inc[2]) << 64) | cfg->rng_state_inc[3];
    g.s_imm = sdm_pcg_advance_host(st, g.inc, rng_offset);
    g.s_hom = g.imm_time_dependent
                  ? sdm_pcg_advance_host(st, g.inc, rng_offset + (uint64_t)n_sd)
                  : g.s_imm;
  }
  const bool table = stochastic && (cfg->rates == SDM_FRZ_RATES_PER_CELL ||
                                    (cfg->rates == SDM_FRZ_RATES_AUTO &&
                                     n_cell <= SDM_FRZ_RATES_MAX_CELLS));
  const dim3 grid(grid_for(n_sd, SDM_BLOCK * PCG_ELEMS)), block(SDM_BLOCK);
  if (table)
    hipLaunchKernelGGL(k_freezing_step<true>, grid, block, 2 * (size_t)n_cell * sizeof(double),
                       ctx->stream, g);
  else
    hipLaunchKernelGGL(k_freezing_step<false>, grid, block, 0, ctx->stream, g);
  LAUNCH_CHECK();
  return SDM_OK;
}

// relaxed_velocity.hip -- the relaxed-fall-velocity path (include/sdm_relaxed_velocity.h): PySDM's
// `RelaxedVelocity` dynamic
//
// Reference: PySDM/dynamics/relaxed_velocity.py (a dozen one-operation Storage launches per call),
// PySDM/attributes/physics/{radius,terminal_velocity,relative_fall_velocity}.py.
//
// One streaming kernel: a read of the mass and the momentum, a write of the momentum and (if asked
// for) of the velocity - 32 bytes a slot.  A thread takes two neighbouring slots, 16 bytes per
// access where the column is 16-byte aligned (row k of an [n_attr, n_sd] block with odd n_sd is
// not: the flags below are uniform over the launch, the pair of 8-byte accesses is the same
// arithmetic); the grid is capped and strides.  The arithmetic of a slot is physics.h's, operation
// by operation as the header lists it.
//
// The Gunn-Kinzer table ends at gk_top and the refusal of a radius beyond it has to come before
// the first store, so with that law k_rv_count goes over the mass column first (a comparison per
// slot; the cube root only for a mass within 1e-9 of the one at the top) and k_rv_step starts with
// one look at the count.
#include "common.h"
#include "physics.h"
#include "../../include/sdm_relaxed_velocity.h"

#define RV_PER_THREAD 2
#define RV_GRID_CAP 2048  // workgroups: 2^20 slots a grid pass

namespace {

struct RvArgs {
  const double *mass;
  double *momentum, *velocity;
  const double *gk_a, *gk_b;
  const int64_t *gate;  // NULL: no verdict to wait for
  int mass_wide, momentum_wide, velocity_wide;
};

__device__ __forceinline__ double rv_radius(const sdm_relaxed_velocity_cfg &cfg, double m) {
  const double inv = 1 / (3.14159265358979323846 * 4 / 3);
  return radius_of_volume(volume_of_mass(m, cfg.rho_w), inv);
}

// gk_interpolate with the index kept inside the table on both sides (a NaN radius converts to
// anything; its result is NaN whichever entry is read)
__device__ __forceinline__ double rv_table(const sdm_relaxed_velocity_cfg &cfg, const RvArgs &A,
                                           double r) {
  if (r < 0) return 0.0;
  const double x = cfg.gk_factor * r;
  int64_t r_id = (int64_t)x;
  r_id = r_id > cfg.gk_table_len - 1 ? cfg.gk_table_len - 1 : r_id;
  r_id = r_id < 0 ? 0 : r_id;
  const double r_rest = fmod(x, 1.0) / cfg.gk_factor;
  return A.gk_a[r_id] + r_rest * A.gk_b[r_id];
}

__device__ __forceinline__ double rv_slot(const sdm_relaxed_velocity_cfg &cfg, const RvArgs &A,
                                          double signed_mass, double p, double &velocity) {
  const double m = fabs(signed_mass);
  const double r = rv_radius(cfg, m);
  double u_t;
  if (cfg.law == SDM_RV_LAW_GUNN_KINZER) {
    u_t = rv_table(cfg, A, r);
  } else {
    u_t = rogers_yau_velocity(r, cfg.rogers_yau);
  }
  const double tau = cfg.constant ? cfg.c : cfg.c * signed_pow(r, 0.5);
  const double scale = sdm_exp(-cfg.dt / tau) * -1.0 + 1.0;
  const double diff = (u_t * m - p) * scale;
  const double p_new = p + diff;
  velocity = p_new / m;
  return p_new;
}

// A mass of at most m_below has a radius below the top and one of at least m_above a radius above
// it, whatever the last places of the cube root do (the band between them is 2e-9 of the mass
// wide, the derivation is good to a few 1e-16); only a mass inside the band has its radius
// derived, exactly as k_rv_step derives it.  So the pass is a read of the column.
__global__ void __launch_bounds__(SDM_BLOCK)
k_rv_count(sdm_relaxed_velocity_cfg cfg, const double *__restrict__ mass, double m_below,
           double m_above, int64_t *status) {
  __shared__ int s_wave[SDM_BLOCK / SDM_WAVE];
  int above = 0;
  const int64_t stride = (int64_t)gridDim.x * SDM_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * SDM_BLOCK + threadIdx.x; i < cfg.n_sd; i += stride) {
    const double m = fabs(mass[i]);
    if (m >= m_above)
      above += 1;
    else if (m > m_below)
      above += rv_radius(cfg, m) > cfg.gk_top ? 1 : 0;
  }
  above = wave_sum_i32(above);
  if (lane_id() == 0) s_wave[threadIdx.x / SDM_WAVE] = above;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < SDM_BLOCK / SDM_WAVE; ++w) total += s_wave[w];
    if (total)
      atomicAdd((unsigned long long *)&status[SDM_RV_STATUS_ABOVE_TOP], (unsigned long long)total);
  }
}

__global__ void __launch_bounds__(SDM_BLOCK) k_rv_step(sdm_relaxed_velocity_cfg cfg, RvArgs A) {
  if (A.gate && A.gate[SDM_RV_STATUS_ABOVE_TOP] != 0) return;  // (uniform over the launch)
  const int64_t n_pairs = cfg.n_sd / RV_PER_THREAD;
  const int64_t stride = (int64_t)gridDim.x * SDM_BLOCK;
  for (int64_t t = (int64_t)blockIdx.x * SDM_BLOCK + threadIdx.x; t < n_pairs; t += stride) {
    const int64_t i = t * RV_PER_THREAD;  // i + 1 < n_sd
    const double2 m = A.mass_wide ? *(const double2 *)(A.mass + i)
                                  : make_double2(A.mass[i], A.mass[i + 1]);
    const double2 p = A.momentum_wide ? *(const double2 *)(A.momentum + i)
                                      : make_double2(A.momentum[i], A.momentum[i + 1]);
    double2 q, v;
    q.x = rv_slot(cfg, A, m.x, p.x, v.x);
    q.y = rv_slot(cfg, A, m.y, p.y, v.y);
    if (A.momentum_wide) {
      *(double2 *)(A.momentum + i) = q;
    } else {
      A.momentum[i] = q.x;
      A.momentum[i + 1] = q.y;
    }
    if (A.velocity) {
      if (A.velocity_wide) {
        *(double2 *)(A.velocity + i) = v;
      } else {
        A.velocity[i] = v.x;
        A.velocity[i + 1] = v.y;
      }
    }
  }
  // the last slot of an odd column
  if ((cfg.n_sd & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t i = cfg.n_sd - 1;
    double v;
    A.momentum[i] = rv_slot(cfg, A, A.mass[i], A.momentum[i], v);
    if (A.velocity) A.velocity[i] = v;
  }
}

inline int wide(const void *p) { return ((uintptr_t)p & 15) == 0 ? 1 : 0; }

}  // namespace

extern "C" int sdm_relaxed_velocity_step(sdm_ctx *ctx, const sdm_relaxed_velocity_cfg *cfg,
                                         const double *signed_water_mass, double *momentum,
                                         double *velocity_out, const double *gk_a,
                                         const double *gk_b, int64_t *status) {
  ARG_TRY(ctx && cfg && cfg->n_sd >= 0 && cfg->n_sd < INT32_MAX);
  ARG_TRY(cfg->law == SDM_RV_LAW_GUNN_KINZER || cfg->law == SDM_RV_LAW_ROGERS_YAU);
  if (cfg->n_sd == 0) return SDM_OK;
  ARG_TRY(signed_water_mass && momentum);
  ARG_TRY(((uintptr_t)signed_water_mass & 7) == 0 && ((uintptr_t)momentum & 7) == 0 &&
          ((uintptr_t)velocity_out & 7) == 0);
  const bool table = cfg->law == SDM_RV_LAW_GUNN_KINZER;
  ARG_TRY(!table || (gk_a && gk_b && cfg->gk_table_len >= 1 && cfg->gk_factor > 0));
  if (!status) {
    int rc = sdm_reserve(ctx, 256);
    if (rc) return rc;
    status = (int64_t *)ctx->arena;
  }
  HIP_TRY(hipMemsetAsync(status, 0, sizeof(int64_t) * SDM_RV_STATUS_WORDS, ctx->stream));
  RvArgs A;
  A.mass = signed_water_mass;
  A.momentum = momentum;
  A.velocity = velocity_out;
  A.gk_a = gk_a;
  A.gk_b = gk_b;
  A.gate = table ? status : nullptr;
  A.mass_wide = wide(signed_water_mass);
  A.momentum_wide = wide(momentum);
  A.velocity_wide = wide(velocity_out);
  if (table) {
    unsigned grid = grid_for(cfg->n_sd);
    if (grid > RV_GRID_CAP) grid = RV_GRID_CAP;
    // (a top that is not positive and finite: an empty band at 0, every radius is derived)
    const double m_top = cfg->rho_w * (3.14159265358979323846 * 4 / 3) * cfg->gk_top *
                         cfg->gk_top * cfg->gk_top;
    const bool banded = m_top > 0 && m_top < 1e300;
    hipLaunchKernelGGL(k_rv_count, dim3(grid), dim3(SDM_BLOCK), 0, ctx->stream, *cfg,
                       signed_water_mass, banded ? m_top * (1 - 1e-9) : -1.0,
                       banded ? m_top * (1 + 1e-9) : 1.0 / 0.0, status);
    LAUNCH_CHECK();
  }
  unsigned grid = grid_for(cfg->n_sd, SDM_BLOCK * RV_PER_THREAD);
  if (grid > RV_GRID_CAP) grid = RV_GRID_CAP;
  hipLaunchKernelGGL(k_rv_step, dim3(grid), dim3(SDM_BLOCK), 0, ctx->stream, *cfg, A);
  LAUNCH_CHECK();
  return SDM_OK;
}

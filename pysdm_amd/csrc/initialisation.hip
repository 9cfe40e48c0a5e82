// initialisation.hip -- the initialisation path (include/sdm_initialisation.h): Koehler-equilibrium
// wet radii of a dry aerosol, one TOMS748 root search per super-droplet
//
// Reference: PySDM/initialisation/equilibrate_wet_radii.py:43-122 ("ewr.py" below), whose search is
// PySDM/backends/impl_numba/toms748.py (csrc/toms748.h, line for line) and whose formulae are the
// option switches of csrc/condensation_formulae.h (surface_tension, hygroscopicity, trivia).
//
// One super-droplet per lane, 256 threads per workgroup, a grid-stride loop over a grid capped at
// WR_GRID_CAP workgroups, no LDS.  A row reads 16 to 32 bytes (T and RH gathered through cell_id)
// and writes 16; what it costs is the search: a few to a few dozen evaluations of minfun, each a
// handful of sdm_pow / sdm_exp (and, with CompressedFilmRuehl, a nested search of its own), and
// the lanes of a wave leave the search at different times.  Rows are taken in the caller's order.
// The status words are summed per wave and added with one atomic per wave and word.
//
// Two instantiations of one kernel: the general one, every option a kernel-uniform switch on the
// descriptor, and one with the surface tension fixed to Constant (PySDM's default; both
// hygroscopicities), which carries neither the film formulae nor CompressedFilmRuehl's nested
// search.  profiles/wet_radii_kernel_resources.tsv has the registers of both.
//
// The CPU checker of this file is tests/initialisation_checker/.
#include "common.h"
#include "sdm_math.h"
#include "../../include/sdm_initialisation.h"

#define CF_FN __device__ __forceinline__ static
#include "condensation_formulae.h"

// workgroups: 2^18 rows a grid pass (four workgroups a CU)
#define WR_GRID_CAP (SDM_INIT_ROWS_PER_PASS / SDM_BLOCK)
static_assert(WR_GRID_CAP * SDM_BLOCK == SDM_INIT_ROWS_PER_PASS && WR_GRID_CAP == 1024, "grid cap");

// ewr.py:48-50
typedef struct wr_args {
  const cf_k *k;
  double T, RH, kp, rd3, f_org;
  int *fail;
} wr_args;
CF_FN double wr_minfun(double r, const wr_args *a) {
  const cf_k *k = a->k;
  const double sgm = cf_sigma(k, a->T, cf_volume(k, r), CF_C(PI_4_3) * a->rd3, a->f_org, a->fail);
  return a->RH - cf_RH_eq(k, r, a->T, a->kp, a->rd3, sgm);
}
#undef TOMS748_ARGS
#undef TOMS748_EVAL
#define TOMS748_ARGS wr_args
#define TOMS748_EVAL(x, args) wr_minfun((x), (args))
#define TOMS748_NAME(name) name##_wet
#include "toms748.h"

namespace {

struct WrArgs {
  const double *r_dry, *ktdv, *f_org, *T, *RH;
  const int64_t *cell_id;
  double *r_wet;
  int64_t *iters, *status;
  int64_t n, n_cell;
  double rtol;
  int max_iters;
};

// one row, ewr.py:64-102; returns r_wet, *iters as the reference leaves it, *fail as cf_sigma
__device__ __forceinline__ double wr_row(const cf_k *k, double r_dry, double ktdv, double f_org,
                                         double T, double RH_cell, double rtol, int max_iters,
                                         int *iters, int *fail) {
  const double kappa = ktdv / cf_volume(k, r_dry);  // ewr.py:43
  const double rd3 = sdm_pow(r_dry, 3.0);
  const double a = r_dry;
  const double b = cf_r_cr(k, kappa, rd3, T, CF_C(SGM_W));
  *iters = 0;
  if (!(a < b)) return r_dry;
  wr_args args;
  args.k = k;
  args.T = T;
  args.RH = cf_np_max(0.0, cf_np_min(1.0, RH_cell));
  args.kp = kappa;
  args.rd3 = rd3;
  args.f_org = f_org;
  args.fail = fail;
  const double fa = wr_minfun(a, &args);
  if (fa < 0) return r_dry;
  const double fb = wr_minfun(b, &args);
  return toms748_solve_wet(&args, a, b, fa, fb, rtol, max_iters, iters);
}

// CONSTANT_SGM: the surface tension is Constant whatever the descriptor says (the launcher checks)
template <bool CONSTANT_SGM>
__global__ __launch_bounds__(SDM_BLOCK) void k_wet_radii(WrArgs A, cf_k kk) {
  if (CONSTANT_SGM) kk.o[SDM_COND_OPT_SURFACE_TENSION] = SDM_COND_SGM_CONSTANT;
  const cf_k *k = &kk;
  int n_failed = 0, n_max = 0, n_sigma = 0;
  long long first = A.n;
  const int64_t stride = (int64_t)gridDim.x * SDM_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * SDM_BLOCK + threadIdx.x; i < A.n; i += stride) {
    const int64_t cell = A.cell_id ? A.cell_id[i] : 0;
    const double r_dry = A.r_dry[i];
    double r_wet;
    int iters, fail = 0;
    if (cell < 0 || cell >= A.n_cell) {
      r_wet = sdm_nan();
      iters = -1;
    } else {
      const double f_org = (!CONSTANT_SGM && A.f_org) ? A.f_org[i] : 0.0;
      r_wet = wr_row(k, r_dry, A.ktdv[i], f_org, A.T[cell], A.RH[cell], A.rtol, A.max_iters,
                     &iters, &fail);
    }
    A.r_wet[i] = r_wet;
    A.iters[i] = iters;
    n_failed += iters == -1;
    n_max += iters == A.max_iters;
    n_sigma += fail;
    if ((iters == -1 || iters == A.max_iters) && i < first) first = i;
  }
  // per wave, then one atomic per wave and word (nothing to add on most waves)
  n_failed = wave_sum_i32(n_failed);
  n_max = wave_sum_i32(n_max);
  n_sigma = wave_sum_i32(n_sigma);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long t = __shfl_xor(first, o, 64);
    first = t < first ? t : first;
  }
  if (lane_id() == 0) {
    unsigned long long *s = (unsigned long long *)A.status;
    if (n_failed) atomicAdd(&s[SDM_INIT_STATUS_FAILED], (unsigned long long)n_failed);
    if (n_max) atomicAdd(&s[SDM_INIT_STATUS_MAX_ITERS], (unsigned long long)n_max);
    if (n_sigma) atomicAdd(&s[SDM_INIT_STATUS_SIGMA_FAILED], (unsigned long long)n_sigma);
    if (first < A.n) atomicMin((long long *)&A.status[SDM_INIT_STATUS_FIRST], first);
  }
}

__global__ void k_wet_radii_status(int64_t *status, int64_t n) {
  if (threadIdx.x < SDM_INIT_STATUS_WORDS)
    status[threadIdx.x] = threadIdx.x == SDM_INIT_STATUS_FIRST ? n : 0;
}

// the descriptor and the default path's constants as the kernel's argument; refuses codes the
// header does not define (NULL: PySDM's defaults)
int wr_formulae_of(const double *consts, const sdm_cond_formulae *formulae, cf_k *out) {
  static const int n_choices[SDM_COND_N_OPTS] = CF_N_CHOICES;
  for (int i = 0; i < SDM_COND_N_CONSTS; ++i) out->c[i] = consts[i];
  for (int i = 0; i < SDM_COND_F_N_CONSTS; ++i) out->f[i] = formulae ? formulae->consts[i] : 0.0;
  for (int i = 0; i < 10; ++i) out->o[i] = 0;
  if (!formulae) return 1;
  for (int i = 0; i < SDM_COND_N_OPTS; ++i) {
    if (formulae->option[i] < 0 || formulae->option[i] >= n_choices[i]) return 0;
    out->o[i] = formulae->option[i];
  }
  return 1;
}

}  // namespace

extern "C" int sdm_equilibrate_wet_radii(sdm_ctx *ctx, int64_t n, const double *r_dry,
                                         const double *kappa_times_dry_volume,
                                         const double *f_org, const int64_t *cell_id,
                                         const double *T, const double *RH, int64_t n_cell,
                                         double rtol, int max_iters, const double consts[34],
                                         const sdm_cond_formulae *formulae, double *r_wet,
                                         int64_t *iters, int64_t *status) {
  ARG_TRY(ctx && n >= 0 && n_cell >= 1 && max_iters >= 1 && consts);
  cf_k k;
  ARG_TRY(wr_formulae_of(consts, formulae, &k));
  const bool film = k.o[SDM_COND_OPT_SURFACE_TENSION] != SDM_COND_SGM_CONSTANT;
  if (n == 0) return SDM_OK;
  ARG_TRY(r_dry && kappa_times_dry_volume && T && RH && r_wet && iters && status);
  ARG_TRY(!film || f_org);
  WrArgs A;
  A.r_dry = r_dry;
  A.ktdv = kappa_times_dry_volume;
  A.f_org = f_org;
  A.T = T;
  A.RH = RH;
  A.cell_id = cell_id;
  A.r_wet = r_wet;
  A.iters = iters;
  A.status = status;
  A.n = n;
  A.n_cell = n_cell;
  A.rtol = rtol;
  A.max_iters = max_iters;
  hipLaunchKernelGGL(k_wet_radii_status, dim3(1), dim3(SDM_WAVE), 0, ctx->stream, status, n);
  LAUNCH_CHECK();
  unsigned grid = grid_for(n);
  if (grid > WR_GRID_CAP) grid = WR_GRID_CAP;
  if (film)
    hipLaunchKernelGGL(k_wet_radii<false>, dim3(grid), dim3(SDM_BLOCK), 0, ctx->stream, A, k);
  else
    hipLaunchKernelGGL(k_wet_radii<true>, dim3(grid), dim3(SDM_BLOCK), 0, ctx->stream, A, k);
  LAUNCH_CHECK();
  return SDM_OK;
}

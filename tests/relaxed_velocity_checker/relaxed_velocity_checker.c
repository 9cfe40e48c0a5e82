/*
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_relaxed_velocity.h.
 *
 * A plain serial restatement of the one symbol, written from the contract in the header: one loop
 * over the slots, the operations in the header's order, each rounded once (-ffp-contract=off), exp
 * and pow from sdm_math.h as everywhere in the oracle.  The radii above the table top are counted
 * before anything is stored.  Host pointers; the context is ignored.  Built by
 * __graft_entry__.build() next to this file (git-ignored); nothing in pysdm_amd/ loads it.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/sdm_relaxed_velocity.h"
#include "../../pysdm_amd/csrc/sdm_math.h"

#define API __attribute__((visibility("default")))

static __thread char g_err[256] = "";
#define FAIL(code, msg)                        \
  do {                                         \
    snprintf(g_err, sizeof(g_err), "%s", msg); \
    return (code);                             \
  } while (0)

API const char *sdm_last_error(void) { return g_err; }
API int64_t sdm_relaxed_velocity_cfg_size(void) { return sizeof(sdm_relaxed_velocity_cfg); }

/* np.sign(x) * np.power(np.abs(x), p) */
static double signed_pow(double x, double p) {
  if (x != x) return x;
  return (double)((x > 0) - (x < 0)) * sdm_pow(fabs(x), p);
}

static double radius_of_mass(const sdm_relaxed_velocity_cfg *cfg, double m) {
  const double inv = 1 / (3.14159265358979323846 * 4 / 3);
  return signed_pow(m / cfg->rho_w * inv, 1.0 / 3.0);
}

static double table(const sdm_relaxed_velocity_cfg *cfg, const double *a, const double *b,
                    double r) {
  if (r < 0) return 0.0;
  if (r != r) return r; /* (no index from a NaN) */
  const double x = cfg->gk_factor * r;
  int64_t k = x >= 9e18 ? cfg->gk_table_len - 1 : (int64_t)x;
  if (k > cfg->gk_table_len - 1) k = cfg->gk_table_len - 1;
  const double rest = fmod(x, 1.0) / cfg->gk_factor;
  return a[k] + rest * b[k];
}

API int sdm_relaxed_velocity_step(sdm_ctx *ctx, const sdm_relaxed_velocity_cfg *cfg,
                                  const double *signed_water_mass, double *momentum,
                                  double *velocity_out, const double *gk_a, const double *gk_b,
                                  int64_t *status) {
  (void)ctx;
  if (!cfg || cfg->n_sd < 0) FAIL(SDM_E_ARG, "bad argument: cfg");
  if (cfg->law != SDM_RV_LAW_GUNN_KINZER && cfg->law != SDM_RV_LAW_ROGERS_YAU)
    FAIL(SDM_E_ARG, "bad argument: law");
  if (cfg->n_sd == 0) return SDM_OK;
  if (!signed_water_mass || !momentum) FAIL(SDM_E_ARG, "bad argument: a null pointer");
  const int use_table = cfg->law == SDM_RV_LAW_GUNN_KINZER;
  if (use_table && (!gk_a || !gk_b || cfg->gk_table_len < 1 || !(cfg->gk_factor > 0)))
    FAIL(SDM_E_ARG, "bad argument: the table");
  int64_t above = 0;
  if (use_table)
    for (int64_t i = 0; i < cfg->n_sd; ++i)
      above += radius_of_mass(cfg, fabs(signed_water_mass[i])) > cfg->gk_top;
  if (status) {
    status[SDM_RV_STATUS_ABOVE_TOP] = above;
    status[1] = 0;
  }
  if (above) return SDM_OK;
  for (int64_t i = 0; i < cfg->n_sd; ++i) {
    const double m = fabs(signed_water_mass[i]);
    const double r = radius_of_mass(cfg, m);
    double u_t;
    if (use_table) {
      u_t = table(cfg, gk_a, gk_b, r);
    } else {
      const double *K = cfg->rogers_yau;
      u_t = r < K[3] ? K[0] * (r * r) : (r < K[4] ? K[1] * r : K[2] * sdm_pow(r, 0.5));
    }
    const double tau = cfg->constant ? cfg->c : cfg->c * signed_pow(r, 0.5);
    const double scale = sdm_exp(-cfg->dt / tau) * -1.0 + 1.0;
    const double p = momentum[i];
    const double diff = (u_t * m - p) * scale;
    momentum[i] = p + diff;
    if (velocity_out) velocity_out[i] = momentum[i] / m;
  }
  return SDM_OK;
}

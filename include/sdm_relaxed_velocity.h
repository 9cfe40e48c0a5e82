/*
 * sdm_relaxed_velocity.h -- C ABI of the relaxed-fall-velocity path of libsdm_hip.so: PySDM's
 * `RelaxedVelocity` dynamic (PySDM/dynamics/relaxed_velocity.py), which relaxes the extensive
 * attribute "relative fall momentum" towards terminal velocity x water mass, and the derived
 * attribute "relative fall velocity" = momentum / water mass that goes with it
 * (PySDM/attributes/physics/relative_fall_velocity.py).
 *
 * Same conventions as sdm_hip.h (whose context, error codes and sdm_last_error() it uses): a
 * context first, DEVICE pointers owned by the caller (double), 0 = ok, negative = SDM_E_*; work is
 * enqueued on the context's stream.  A separate header so that implementations of sdm_hip.h (the
 * CPU oracle) need not implement this path.
 *
 * The contract.  For EVERY slot i in [0, n_sd) - the reference works on whole columns, dead and
 * unused slots included - in this order, every operation rounded once (no contraction), exp and
 * pow being those of sdm_math.h:
 *     m     = |signed_water_mass[i]|
 *     r     = sign(x) * pow(|x|, 1/3)  with  x = (m / rho_w) * (1 / (pi * 4 / 3))
 *     u_t   = law(r)
 *               SDM_RV_LAW_GUNN_KINZER: k = (int64)(gk_factor * r), clamped to the table;
 *                                       gk_a[k] + (fmod(gk_factor * r, 1) / gk_factor) * gk_b[k]
 *               SDM_RV_LAW_ROGERS_YAU:  r < K[3] ? K[0] * (r * r)
 *                                                : r < K[4] ? K[1] * r : K[2] * pow(r, 0.5)
 *     tau   = constant ? c : c * pow(r, 0.5)
 *     scale = exp(-dt / tau) * -1 + 1
 *     p     = momentum[i];   momentum[i] = p + (u_t * m - p) * scale
 *     velocity_out[i] = momentum[i] / m              (only if velocity_out is not NULL)
 * This is the sequence of Storage operations of RelaxedVelocity.__call__ over the attributes
 * "water mass", "radius", "square root of radius" and "terminal velocity".
 *
 * With the Gunn-Kinzer table, radii above `gk_top` cannot be interpolated (the reference raises a
 * ValueError).  They are counted BEFORE anything is stored: status[SDM_RV_STATUS_ABOVE_TOP]
 * receives the count, and if it is not 0 neither momentum nor velocity_out is written.  The count
 * costs a pass over the mass column of its own (the verdict is global, the stores are not: a
 * comparison per slot, the radius derived only for a mass within 1e-9 of the one at the top); with
 * Rogers-Yau the call is a single launch.
 */
#ifndef SDM_RELAXED_VELOCITY_H
#define SDM_RELAXED_VELOCITY_H
#include "sdm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDM_RV_LAW_GUNN_KINZER 0
#define SDM_RV_LAW_ROGERS_YAU 1

/* words of `status` */
#define SDM_RV_STATUS_ABOVE_TOP 0 /* radii above gk_top; not 0: nothing was stored */
#define SDM_RV_STATUS_WORDS 2     /* (word 1: reserved, written as 0) */

typedef struct sdm_relaxed_velocity_cfg {
  int64_t n_sd;
  int64_t gk_table_len;  /* entries of gk_a and of gk_b (Gunn-Kinzer) */
  double dt;
  double c;              /* tau = c (constant != 0) or c * sqrt(radius) */
  double rho_w;
  double gk_factor;      /* table points per metre */
  double gk_top;         /* largest radius the table serves */
  double rogers_yau[5];  /* small k, medium k, large k, small-r limit, medium-r limit */
  int32_t constant;
  int32_t law;           /* SDM_RV_LAW_* */
} sdm_relaxed_velocity_cfg;

/* One `RelaxedVelocity.__call__`.  Enqueues only.  `signed_water_mass`, `momentum`: n_sd doubles
 * each, 8-byte aligned (rows of an [n_attr, n_sd] block with odd n_sd are served).  `velocity_out`
 * (n_sd doubles) may be NULL.  gk_a, gk_b: the table (may be NULL with Rogers-Yau).  `status`:
 * int64[SDM_RV_STATUS_WORDS] on the device, written by the call (may be NULL); the caller reads it
 * when it next synchronises.  n_sd == 0 returns before any launch (status is not written).       */
int sdm_relaxed_velocity_step(sdm_ctx *ctx, const sdm_relaxed_velocity_cfg *cfg,
                              const double *signed_water_mass, double *momentum,
                              double *velocity_out, const double *gk_a, const double *gk_b,
                              int64_t *status);

#ifdef __cplusplus
}
#endif
#endif

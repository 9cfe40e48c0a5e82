/*
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE: the CPU checker of include/sdm_freezing.h.
 *
 * A serial, strict-IEEE restatement of the reference's freezing methods
 * (PySDM/backends/impl_numba/methods/freezing_methods.py, "fm.py" below), of `a_w_ice`
 * (impl_numba/methods/physics_methods.py:78-105, "pm.py") and of the MixedPhaseSpheres
 * conversions, loop for loop, with the formulae inlined where they are used (physics/trivia.py,
 * physics/{heterogeneous,homogeneous}_ice_nucleation_rate/, saturation_vapour_pressure/
 * flatau_walko_cotton.py).  Python evaluates left to right; every expression below keeps that
 * order.  pow / exp are the project's csrc/sdm_math.h, which the product compiles too, so both
 * sides get the same bits.  The fused step is literally the stage sequence over a uniform array
 * filled from NumPy's PCG64 (restated below: 128-bit LCG, XSL-RR output, 53 bits per double).
 * Host pointers; the context is ignored.  Built by __graft_entry__.build() next to this file
 * (git-ignored); nothing in pysdm_amd/ loads it.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/sdm_freezing.h"
#include "../../pysdm_amd/csrc/sdm_math.h"

#define API __attribute__((visibility("default")))

static __thread char g_err[256] = "";
#define FAIL(code, msg)                        \
  do {                                         \
    snprintf(g_err, sizeof(g_err), "%s", msg); \
    return (code);                             \
  } while (0)

API const char *sdm_last_error(void) { return g_err; }

#define K(name) consts[SDM_FRZ_K_##name]

/* ---- formulae ------------------------------------------------------------------------------ */
/* trivia.py:79-92 */
static int unfrozen(double m) { return m > 0; }
static int unfrozen_and_saturated(double m, double rh) { return m > 0 && rh > 1; }
static int frozen_and_above_freezing_point(const double *consts, double m, double T) {
  return m < 0 && T > K(T0);
}
/* trivia.py:158-163 */
static double poissonian_avoidance_function(double r, double dt) { return sdm_exp(-r * dt); }

/* heterogeneous_ice_nucleation_rate/constant.py, abifm.py */
static int j_het(const double *consts, int code, const double *a_w_ice, int64_t c, double *out) {
  if (code == SDM_FRZ_JHET_CONSTANT) {
    *out = K(J_HET);
    return 0;
  }
  if (code == SDM_FRZ_JHET_ABIFM) {
    *out = sdm_pow(10.0, K(ABIFM_M) * (1 - a_w_ice[c]) + K(ABIFM_C)) * K(ABIFM_UNIT);
    return 0;
  }
  return -1;
}

/* homogeneous_ice_nucleation_rate/constant.py, koop.py, koop_corr.py, koop_murray.py */
static int d_a_w_ice_within_range(const double *consts, int code, double d) {
  return code == SDM_FRZ_JHOM_CONSTANT ? 1 : d >= K(KOOP_MIN_DA_W_ICE);
}
static double d_a_w_ice_maximum(const double *consts, int code, double d) {
  if (code == SDM_FRZ_JHOM_CONSTANT) return d;
  return d > K(KOOP_MAX_DA_W_ICE) ? K(KOOP_MAX_DA_W_ICE) : d;
}
static double j_hom(const double *consts, int code, double T, double d) {
  const double *c2000 = &K(KOOP_2000_C1), *murray = &K(KOOP_MURRAY_C0);
  switch (code) {
    case SDM_FRZ_JHOM_CONSTANT:
      return K(J_HOM);
    case SDM_FRZ_JHOM_KOOP2000:
      return sdm_pow(10.0, c2000[0] + c2000[1] * d + c2000[2] * sdm_pow(d, 2.0) +
                               c2000[3] * sdm_pow(d, 3.0)) *
             K(KOOP_UNIT);
    case SDM_FRZ_JHOM_KOOP_CORRECTION:
      return sdm_pow(10.0, c2000[0] + c2000[1] * d + c2000[2] * sdm_pow(d, 2.0) +
                               c2000[3] * sdm_pow(d, 3.0) + K(KOOP_CORR)) *
             K(KOOP_UNIT);
    default: /* SDM_FRZ_JHOM_KOOPMURRAY2016 */
      return sdm_pow(10.0, murray[0] + murray[1] * (T - K(T0)) +
                               murray[2] * sdm_pow(T - K(T0), 2.0) +
                               murray[3] * sdm_pow(T - K(T0), 3.0) +
                               murray[4] * sdm_pow(T - K(T0), 4.0) +
                               murray[5] * sdm_pow(T - K(T0), 5.0) +
                               murray[6] * sdm_pow(T - K(T0), 6.0)) *
             K(KOOP_UNIT);
  }
}

/* flatau_walko_cotton.py: pvs_ice */
static double pvs_ice(const double *consts, double T) {
  const double *I = &K(FWC_I0);
  const double t = T - K(T0);
  return I[0] + t * (I[1] + t * (I[2] + t * (I[3] + t * (I[4] + t * (I[5] + t * (I[6] + t * (I[7] + t * I[8])))))));
}

/* ---- fm.py:40-66 ----------------------------------------------------------------------------- */
API int sdm_freeze_singular(sdm_ctx *ctx, double *signed_water_mass,
                            const double *freezing_temperature, const double *temperature,
                            const double *relative_humidity, const int64_t *cell, int64_t n_sd,
                            int thaw, const double consts[33]) {
  (void)ctx;
  for (int64_t i = 0; i < n_sd; ++i) {
    if (freezing_temperature[i] == 0) continue;
    if (thaw && frozen_and_above_freezing_point(consts, signed_water_mass[i], temperature[cell[i]]))
      signed_water_mass[i] = -1 * signed_water_mass[i];
    else if (unfrozen_and_saturated(signed_water_mass[i], relative_humidity[cell[i]]) &&
             temperature[cell[i]] <= freezing_temperature[i])
      signed_water_mass[i] = -1 * signed_water_mass[i];
  }
  return SDM_OK;
}

/* ---- fm.py:68-111 ---------------------------------------------------------------------------- */
API int sdm_freeze_time_dependent(sdm_ctx *ctx, const double *rand, double *signed_water_mass,
                                  const double *immersed_surface_area, double timestep,
                                  const int64_t *cell, const double *a_w_ice,
                                  const double *temperature, const double *relative_humidity,
                                  int64_t n_sd, int thaw, int j_het_code,
                                  const double consts[33]) {
  (void)ctx;
  for (int64_t i = 0; i < n_sd; ++i) {
    if (immersed_surface_area[i] == 0) continue;
    const int64_t cell_id = cell[i];
    if (thaw &&
        frozen_and_above_freezing_point(consts, signed_water_mass[i], temperature[cell_id])) {
      signed_water_mass[i] = -1 * signed_water_mass[i];
    } else if (unfrozen_and_saturated(signed_water_mass[i], relative_humidity[cell_id])) {
      double j;
      if (j_het(consts, j_het_code, a_w_ice, cell_id, &j)) FAIL(SDM_E_ARG, "unknown j_het code");
      const double rate = j * immersed_surface_area[i];
      const double prob = 1 - poissonian_avoidance_function(rate, timestep);
      if (rand[i] < prob) signed_water_mass[i] = -1 * signed_water_mass[i];
    }
  }
  return SDM_OK;
}

/* ---- fm.py:113-168 --------------------------------------------------------------------------- */
API int sdm_freeze_time_dependent_homogeneous(sdm_ctx *ctx, const double *rand,
                                              double *signed_water_mass, const double *volume,
                                              double timestep, const int64_t *cell,
                                              const double *a_w_ice, const double *temperature,
                                              const double *relative_humidity_ice, int64_t n_sd,
                                              int thaw, int j_hom_code,
                                              const double consts[33]) {
  (void)ctx;
  if (j_hom_code < SDM_FRZ_JHOM_CONSTANT || j_hom_code > SDM_FRZ_JHOM_KOOPMURRAY2016)
    FAIL(SDM_E_ARG, "unknown j_hom code");
  for (int64_t i = 0; i < n_sd; ++i) {
    const int64_t cell_id = cell[i];
    if (thaw &&
        frozen_and_above_freezing_point(consts, signed_water_mass[i], temperature[cell_id])) {
      signed_water_mass[i] = -1 * signed_water_mass[i];
    } else if (unfrozen_and_saturated(signed_water_mass[i], relative_humidity_ice[cell_id])) {
      /* (constant.py never looks at d_a_w_ice: a_w_ice may be absent then) */
      double d_a_w_ice = j_hom_code == SDM_FRZ_JHOM_CONSTANT
                             ? 0.0
                             : (relative_humidity_ice[cell_id] - 1.0) * a_w_ice[cell_id];
      if (d_a_w_ice_within_range(consts, j_hom_code, d_a_w_ice)) {
        d_a_w_ice = d_a_w_ice_maximum(consts, j_hom_code, d_a_w_ice);
        const double rate = j_hom(consts, j_hom_code, temperature[cell_id], d_a_w_ice) * volume[i];
        const double prob = 1 - poissonian_avoidance_function(rate, timestep);
        if (rand[i] < prob) signed_water_mass[i] = -1 * signed_water_mass[i];
      }
    }
  }
  return SDM_OK;
}

/* ---- fm.py:236-260 --------------------------------------------------------------------------- */
API int sdm_record_freezing_temperatures(sdm_ctx *ctx, double *data, const int64_t *cell_id,
                                         const double *temperature,
                                         const double *signed_water_mass, int64_t n_sd) {
  (void)ctx;
  for (int64_t drop_id = 0; drop_id < n_sd; ++drop_id) {
    if (unfrozen(signed_water_mass[drop_id])) {
      if (data[drop_id] > 0) data[drop_id] = sdm_nan();
    } else {
      if (data[drop_id] != data[drop_id]) data[drop_id] = temperature[cell_id[drop_id]];
    }
  }
  return SDM_OK;
}

/* ---- pm.py:78-105 ---------------------------------------------------------------------------- */
API int sdm_a_w_ice(sdm_ctx *ctx, const double *T, const double *p, const double *RH,
                    const double *water_vapour_mixing_ratio, double *a_w_ice, double *RH_ice,
                    int64_t n, const double consts[33]) {
  (void)ctx;
  for (int64_t i = 0; i < n; ++i) {
    const double pvi = pvs_ice(consts, T[i]);
    const double qv = water_vapour_mixing_ratio[i];
    const double pv = p[i] * qv / (qv + K(EPS)); /* state_variable_triplet/libcloudphplusplus.py */
    const double pvs = pv / RH[i];
    a_w_ice[i] = pvi / pvs;
    RH_ice[i] = pv / pvi;
  }
  return SDM_OK;
}

/* ---- particle_shape_and_density/mixed_phase_spheres.py --------------------------------------- */
static double max0(double x) { return x > 0.0 ? x : 0.0; }
static double min0(double x) { return x < 0.0 ? x : 0.0; }

API int sdm_volume_of_signed_water_mass(sdm_ctx *ctx, double *volume, const double *mass,
                                        int64_t n, const double consts[33]) {
  (void)ctx;
  for (int64_t i = 0; i < n; ++i) volume[i] = max0(mass[i]) / K(RHO_W) + min0(mass[i]) / K(RHO_I);
  return SDM_OK;
}

API int sdm_signed_water_mass_of_volume(sdm_ctx *ctx, double *mass, const double *volume,
                                        int64_t n, const double consts[33]) {
  (void)ctx;
  for (int64_t i = 0; i < n; ++i) mass[i] = max0(volume[i]) * K(RHO_W) + min0(volume[i]) * K(RHO_I);
  return SDM_OK;
}

/* ---- NumPy's PCG64 (numpy/random/src/pcg64: pcg_setseq_128, XSL-RR 128/64) -------------------- */
typedef unsigned __int128 u128;
static const u128 PCG_MULT = (((u128)0x2360ED051FC65DA4ULL) << 64) | 0x4385DF649FCCF645ULL;

static u128 pcg_advance(u128 state, u128 inc, uint64_t delta) {
  u128 acc_mult = 1, acc_plus = 0, cur_mult = PCG_MULT, cur_plus = inc;
  while (delta > 0) {
    if (delta & 1) {
      acc_mult *= cur_mult;
      acc_plus = acc_plus * cur_mult + cur_plus;
    }
    cur_plus = (cur_mult + 1) * cur_plus;
    cur_mult *= cur_mult;
    delta >>= 1;
  }
  return acc_mult * state + acc_plus;
}

/* out[i] = uniform number `offset + i` of the stream */
static void pcg_uniform(const uint64_t state_inc[4], uint64_t offset, double *out, int64_t n) {
  const u128 inc = (((u128)state_inc[2]) << 64) | state_inc[3];
  u128 state = pcg_advance((((u128)state_inc[0]) << 64) | state_inc[1], inc, offset);
  for (int64_t i = 0; i < n; ++i) {
    state = state * PCG_MULT + inc;
    const uint64_t hi = (uint64_t)(state >> 64), lo = (uint64_t)state;
    const uint64_t x = hi ^ lo;
    const unsigned rot = (unsigned)(hi >> 58);
    const uint64_t v = (x >> rot) | (x << ((64 - rot) & 63));
    out[i] = (double)(v >> 11) * (1.0 / 9007199254740992.0);
  }
}

/* ---- the fused step = the stage sequence (dynamics/freezing.py:62-87) ------------------------- */
API int sdm_freezing_step(sdm_ctx *ctx, const sdm_freezing_cfg *cfg, uint64_t rng_offset,
                          int64_t n_sd, int64_t n_cell, double *signed_water_mass,
                          const double *freezing_temperature,
                          const double *immersed_surface_area, const double *volume,
                          const int64_t *cell_id, double *temperature_of_last_freezing,
                          const double *T, const double *RH, const double *a_w_ice,
                          const double *RH_ice, const double consts[33]) {
  if (!cfg || !consts || n_sd < 0 || n_cell < 1) FAIL(SDM_E_ARG, "bad argument");
  if (cfg->rates == SDM_FRZ_RATES_PER_CELL && n_cell > SDM_FRZ_RATES_MAX_CELLS)
    FAIL(SDM_E_ARG, "too many cells for SDM_FRZ_RATES_PER_CELL");
  double *rand = NULL;
  int rc = SDM_OK;
  if (n_sd > 0 && (cfg->homogeneous_freezing || (cfg->immersion_freezing && !cfg->singular))) {
    rand = (double *)malloc(sizeof(double) * (size_t)n_sd);
    if (!rand) FAIL(SDM_E_ARG, "out of memory");
  }
  if (cfg->immersion_freezing) {
    if (cfg->singular) {
      rc = sdm_freeze_singular(ctx, signed_water_mass, freezing_temperature, T, RH, cell_id, n_sd,
                               cfg->thaw, consts);
    } else {
      pcg_uniform(cfg->rng_state_inc, rng_offset, rand, n_sd);
      rng_offset += (uint64_t)n_sd;
      rc = sdm_freeze_time_dependent(ctx, rand, signed_water_mass, immersed_surface_area,
                                     cfg->timestep, cell_id, a_w_ice, T, RH, n_sd, cfg->thaw,
                                     cfg->j_het, consts);
    }
  }
  if (rc == SDM_OK && cfg->homogeneous_freezing) {
    double *own_volume = NULL;
    if (!volume && n_sd > 0) { /* PySDM's `volume` attribute: it follows the signed water mass */
      own_volume = (double *)malloc(sizeof(double) * (size_t)n_sd);
      if (!own_volume) {
        free(rand);
        FAIL(SDM_E_ARG, "out of memory");
      }
      sdm_volume_of_signed_water_mass(ctx, own_volume, signed_water_mass, n_sd, consts);
      volume = own_volume;
    }
    pcg_uniform(cfg->rng_state_inc, rng_offset, rand, n_sd);
    rc = sdm_freeze_time_dependent_homogeneous(ctx, rand, signed_water_mass, volume,
                                               cfg->timestep, cell_id, a_w_ice, T, RH_ice, n_sd,
                                               cfg->thaw, cfg->j_hom, consts);
    free(own_volume);
  }
  free(rand);
  if (rc == SDM_OK && temperature_of_last_freezing)
    rc = sdm_record_freezing_temperatures(ctx, temperature_of_last_freezing, cell_id, T,
                                          signed_water_mass, n_sd);
  return rc;
}

/* sizeof(sdm_freezing_cfg) as C lays it out, for the binding's layout check */
API int freezing_checker_cfg_size(void) { return (int)sizeof(sdm_freezing_cfg); }

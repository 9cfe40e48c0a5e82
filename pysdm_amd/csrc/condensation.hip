// condensation.hip -- PySDM's condensation solver (include/sdm_condensation.h) for gfx950.
//
// Reference: PySDM/backends/impl_numba/methods/condensation_methods.py ("cm.py"), toms748.py and
// physics_methods.py ("pm.py"), with PySDM's default formulae inlined (physics/...).
//
// One workgroup per cell (the cells are independent: cm.py:102-176 gives each cell its own
// solver call).  The whole adaptive loop runs in the kernel: fake steps (adapt_substeps), then
// the real sub-steps; the cell's scalars (T, p, pv, lv, pvs, lambdaK, lambdaD, RH, ...) are
// computed by every lane from the same values (uniform); each droplet's bracket search and
// TOMS748 run in registers of its lane.  The cell's super-droplets are strided over the 256
// lanes: position q of the cell (idx[cell_start + q]) belongs to lane q % 256; the first
// COND_CH = 1024 positions keep their per-call constants (drop id, multiplicity, rd3, kappa,
// x_insane, mass at v_cr) and their water mass in registers for the whole call, later positions
// (chunks of COND_CH) are read from HBM on each pass.
//
// Bit parity with the reference's serial loop: the sums of n * m (calculate_ml_old / _new) are
// formed in the order of the cell's permutation - every lane writes its n * m into an LDS column
// and lane 0 adds the column up serially, chunk after chunk.  A failed droplet (no bracket within
// max_iters, or TOMS748 failing) ends the reference's droplet loop (cm.py:496,515): lane 0's walk
// stops at the first failed position (an atomicMin over the lanes that failed), droplets at and after it keep their mass and add nothing,
// and success goes to 0 - nothing traps.  All arithmetic is IEEE double without contraction
// (-ffp-contract=off) and exp / log / pow come from sdm_math.h, so the CPU checker
// (tests/checker/condensation_checker.c) gets the same bits.
#include "common.h"
#include "../../include/sdm_condensation.h"

#define GRID1D(n) dim3(grid_for(n)), dim3(SDM_BLOCK), 0, ctx->stream
#define COND_CB 256                // lanes per workgroup
#define COND_CR 4                  // register-cached positions per lane
#define COND_CH (COND_CB * COND_CR)  // positions per chunk

namespace {

struct Kc {
  double rho_w, Rv, Rd, c_pd, c_pv, c_pw, l_tri, T_tri, T0, p1000, eps, sgm_w, D0, K0, MAC, HAC,
      PI, PI_4_3, Rd_over_c_pd, ONE_THIRD, THREE, FWC[9], Z3, Z2, Z1, Z0;
};

Kc consts_of(const double *c) {
  Kc k;
  k.rho_w = c[SDM_COND_K_RHO_W]; k.Rv = c[SDM_COND_K_RV]; k.Rd = c[SDM_COND_K_RD];
  k.c_pd = c[SDM_COND_K_C_PD]; k.c_pv = c[SDM_COND_K_C_PV]; k.c_pw = c[SDM_COND_K_C_PW];
  k.l_tri = c[SDM_COND_K_L_TRI]; k.T_tri = c[SDM_COND_K_T_TRI]; k.T0 = c[SDM_COND_K_T0];
  k.p1000 = c[SDM_COND_K_P1000]; k.eps = c[SDM_COND_K_EPS]; k.sgm_w = c[SDM_COND_K_SGM_W];
  k.D0 = c[SDM_COND_K_D0]; k.K0 = c[SDM_COND_K_K0]; k.MAC = c[SDM_COND_K_MAC];
  k.HAC = c[SDM_COND_K_HAC]; k.PI = c[SDM_COND_K_PI]; k.PI_4_3 = c[SDM_COND_K_PI_4_3];
  k.Rd_over_c_pd = c[SDM_COND_K_RD_OVER_C_PD]; k.ONE_THIRD = c[SDM_COND_K_ONE_THIRD];
  k.THREE = c[SDM_COND_K_THREE];
  for (int i = 0; i < 9; ++i) k.FWC[i] = c[SDM_COND_K_FWC_C0 + i];
  k.Z3 = c[SDM_COND_K_ZOGRAFOS_T3]; k.Z2 = c[SDM_COND_K_ZOGRAFOS_T2];
  k.Z1 = c[SDM_COND_K_ZOGRAFOS_T1]; k.Z0 = c[SDM_COND_K_ZOGRAFOS_T0];
  return k;
}

// ---- default formulae (Python's left-to-right order kept in every expression) ------------------
#define DF __device__ __forceinline__
DF double py_max(double x, double y) { return y > x ? y : x; }  // Python's max / min
DF double py_min(double x, double y) { return y < x ? y : x; }
// state_variable_triplet/libcloudphplusplus.py
DF double svt_T(const Kc &k, double rhod, double thd) {
  return thd * sdm_pow(rhod * thd / k.p1000 * k.Rd, k.Rd_over_c_pd / (1 - k.Rd_over_c_pd));
}
DF double svt_p(const Kc &k, double rhod, double T, double qv) {
  return rhod * (1 + qv) * (k.Rv / (1 / qv + 1) + k.Rd / (1 + qv)) * T;
}
DF double svt_pv(const Kc &k, double p, double qv) { return p * qv / (qv + k.eps); }
DF double lv_of(const Kc &k, double T) { return k.l_tri + (k.c_pv - k.c_pw) * (T - k.T_tri); }
DF double pvs_water(const Kc &k, double T) {  // flatau_walko_cotton.py
  const double d = T - k.T0;
  const double *C = k.FWC;
  return C[0] + d * (C[1] + d * (C[2] + d * (C[3] + d * (C[4] + d * (C[5] + d * (C[6] +
         d * (C[7] + d * C[8])))))));
}
DF double radius_of(const Kc &k, double v) { return sdm_pow(v / k.PI_4_3, k.ONE_THIRD); }
DF double RH_eq_of(const Kc &k, double r, double T, double kp, double rd3, double sgm) {
  return 1 + (2 * sgm / k.Rv / T / k.rho_w) / r - kp * rd3 / sdm_pow(r, k.THREE);
}
DF int within_tolerance(double e, double value, double rtol) { return e < rtol * sdm_abs(value); }

struct MinArgs {
  double x_old, timestep, kappa, rd3, T, RH, Fk, Fd;
};

// minfun, cm.py:366-397
DF double minfun(const Kc &k, double x_new, const MinArgs &a) {
  if (x_new > 0.0) return a.x_old - x_new;  // x_max = ZERO (water_mass_logarithm.py)
  const double mass_new = sdm_exp(x_new);
  const double volume_new = mass_new / k.rho_w;
  const double r_new = radius_of(k, volume_new);
  const double RH_eq = RH_eq_of(k, r_new, a.T, a.kappa, a.rd3, k.sgm_w);
  const double r_dr_dt = (a.RH - RH_eq) / (a.Fk + a.Fd);
  const double dm_dt = 4 * k.PI * k.rho_w * r_new * r_dr_dt;
  return a.x_old - x_new + a.timestep * (dm_dt / mass_new);
}

// ---- TOMS748 (toms748.py) ------------------------------------------------------------------------
#define T_EPS 2.220446049250313e-16
#define T_MAX 1.7976931348623157e308
#define T_MIN 2.2250738585072014e-308

DF void bracket(const Kc &k, const MinArgs &args, double &a, double &b, double c, double &fa,
                double &fb, double &d, double &fd) {  // :24-47
  const double tol = T_EPS * 2;
  if ((b - a) < 2 * tol * a) c = a + (b - a) / 2;
  else if (c <= a + sdm_abs(a) * tol) c = a + sdm_abs(a) * tol;
  else if (c >= b - sdm_abs(b) * tol) c = b - sdm_abs(a) * tol;
  const double fc = minfun(k, c, args);
  if (fc == 0) {
    a = c; fa = 0; d = 0; fd = 0;
  } else if (fa * fc < 0) {
    d = b; fd = fb; b = c; fb = fc;
  } else {
    d = a; fd = fa; a = c; fa = fc;
  }
}
DF double safe_div(double num, double denom, double r) {  // :50-55
  if (sdm_abs(denom) < 1)
    if (sdm_abs(denom * T_MAX) <= sdm_abs(num)) return r;
  return num / denom;
}
DF double secant_interpolate(double a, double b, double fa, double fb) {  // :58-64
  const double tol = T_EPS * 5;
  const double c = a - (fa / (fb - fa)) * (b - a);
  if (c <= a + sdm_abs(a) * tol || c >= b - sdm_abs(b) * tol) return (a + b) / 2;
  return c;
}
DF double quadratic_interpolate(double a, double b, double d, double fa, double fb, double fd,
                                int count) {  // :67-87
  const double B = safe_div(fb - fa, b - a, T_MAX);
  double A = safe_div(fd - fb, d - b, T_MAX);
  A = safe_div(A - B, d - a, 0.0);
  if (A == 0) return secant_interpolate(a, b, fa, fb);
  double c = (A * fa > 0) ? a : b;
  for (int i = 1; i < count + 1; ++i)
    c -= safe_div(fa + (B + A * (c - b)) * (c - a), B + A * (2.0 * c - a - b), 1.0 + c - a);
  if ((c <= a) || (c >= b)) c = secant_interpolate(a, b, fa, fb);
  return c;
}
DF double cubic_interpolate(double a, double b, double d, double e, double fa, double fb,
                            double fd, double fe) {  // :90-106
  const double q11 = (d - e) * fd / (fe - fd);
  const double q21 = (b - d) * fb / (fd - fb);
  const double q31 = (a - b) * fa / (fb - fa);
  const double d21 = (b - d) * fd / (fd - fb);
  const double d31 = (a - b) * fb / (fb - fa);
  const double q22 = (d21 - q11) * fb / (fe - fb);
  const double q32 = (d31 - q21) * fa / (fd - fa);
  const double d32 = (d31 - q21) * fd / (fd - fa);
  const double q33 = (d32 - q22) * fa / (fe - fa);
  double c = q31 + q32 + q33 + a;
  if ((c <= a) || (c >= b)) c = quadratic_interpolate(a, b, d, fa, fb, fd, 3);
  return c;
}
DF int tol_check(double a, double b, double rtol) {
  return within_tolerance(sdm_abs(a - b), py_min(sdm_abs(a), sdm_abs(b)), rtol);
}
DF int prof_of(double fa, double fb, double fd, double fe) {
  const double m = T_MIN * 32;
  return sdm_abs(fa - fb) < m || sdm_abs(fa - fd) < m || sdm_abs(fa - fe) < m ||
         sdm_abs(fb - fd) < m || sdm_abs(fb - fe) < m || sdm_abs(fd - fe) < m;
}
// :114-223; *iters = iterations taken, -1: not a bracket
DF double toms748_solve(const Kc &k, const MinArgs &args, double ax, double bx,
                                double fax, double fbx, double rtol, int max_iter, int *iters) {
  int count = max_iter;
  const double mu = 0.5;
  double a = ax, b = bx, fa = fax, fb = fbx;
  if (!(a < b)) { *iters = -1; return sdm_nan(); }
  if (tol_check(a, b, rtol) || fa == 0 || fb == 0) {
    if (fa == 0) b = a;
    else if (fb == 0) a = b;
    *iters = 0;
    return (a + b) / 2;
  }
  if (!(fa * fb < 0)) { *iters = -1; return sdm_nan(); }
  double fe = 1e5, e = 1e5, fd = 1e5, d = 0, c;
  if (fa != 0) {
    c = secant_interpolate(a, b, fa, fb);
    bracket(k, args, a, b, c, fa, fb, d, fd);
    count -= 1;
    if (count > 0 && fa != 0 && !tol_check(a, b, rtol)) {
      c = quadratic_interpolate(a, b, d, fa, fb, fd, 2);
      e = d;
      fe = fd;
      bracket(k, args, a, b, c, fa, fb, d, fd);
      count -= 1;
    }
  }
  while (count > 0 && fa != 0 && !tol_check(a, b, rtol)) {
    const double a0 = a, b0 = b;
    if (prof_of(fa, fb, fd, fe)) c = quadratic_interpolate(a, b, d, fa, fb, fd, 2);
    else c = cubic_interpolate(a, b, d, e, fa, fb, fd, fe);
    e = d;
    fe = fd;
    bracket(k, args, a, b, c, fa, fb, d, fd);
    if (count == 1 || fa == 0 || tol_check(a, b, rtol)) { count -= 1; break; }
    if (prof_of(fa, fb, fd, fe)) c = quadratic_interpolate(a, b, d, fa, fb, fd, 3);
    else c = cubic_interpolate(a, b, d, e, fa, fb, fd, fe);
    bracket(k, args, a, b, c, fa, fb, d, fd);
    if (count == 1 || fa == 0 || tol_check(a, b, rtol)) { count -= 1; break; }
    double u, fu;
    if (sdm_abs(fa) < sdm_abs(fb)) { u = a; fu = fa; } else { u = b; fu = fb; }
    c = u - 2 * (fu / (fb - fa)) * (b - a);
    if (sdm_abs(c - u) > (b - a) / 2) c = a + (b - a) / 2;
    e = d;
    fe = fd;
    bracket(k, args, a, b, c, fa, fb, d, fd);
    if (count == 1 || fa == 0 || tol_check(a, b, rtol)) { count -= 1; break; }
    if ((b - a) < mu * (b0 - a0)) continue;
    e = d;
    fe = fd;
    bracket(k, args, a, b, a + (b - a) / 2, fa, fb, d, fd);
    count -= 1;
  }
  *iters = max_iter - count;
  if (fa == 0) b = a;
  else if (fb == 0) a = b;
  return (a + b) / 2;
}

// the per-droplet body of calculate_ml_new (cm.py:429-556) for a droplet with water mass m > 0;
// returns the new mass, *ok = 0 where the reference sets success = False and breaks
struct Cellwide {  // the sub-step's cell scalars (uniform)
  double T, RH, lv, pvs, DTp, KTp, lambdaK, lambdaD, timestep, rtol_x, RH_rtol;
  int max_iters;
};

__device__ __attribute__((noinline)) double drop_new_mass(const Kc &k, const Cellwide &w, double m, double rd3,
                                double kappa, double x_insane, int *ok) {
  const double v_drop = m / k.rho_w;
  const double x_old = sdm_log(m);
  const double r_old = radius_of(k, v_drop);
  const double RH_eq = RH_eq_of(k, r_old, w.T, kappa, rd3, k.sgm_w);
  double dx_old = 0.0;
  MinArgs args = {x_old, w.timestep, kappa, rd3, w.T, w.RH, 0, 0};
  if (!within_tolerance(sdm_abs(w.RH - RH_eq), w.RH, w.RH_rtol)) {
    const double lD = w.lambdaD, lK = w.lambdaK;  // fuchs_sutugin.py:20-44
    const double Dr = w.DTp * (1 + lD / r_old) /
                      (1 + (4.0 / 3 / k.MAC + 0.377) * lD / r_old +
                       (4.0 / 3 / k.MAC) * lD / r_old * lD / r_old);
    const double Kr = w.KTp * (1 + lK / r_old) /
                      (1 + (4.0 / 3 / k.HAC + 0.377) * lK / r_old +
                       (4.0 / 3 / k.HAC) * lK / r_old * lK / r_old);
    // ventilation Neglect: factor 1; mason_1971.py (Fk), fick.py (Fd)
    args.Fk = k.rho_w * w.lv / w.T / (Kr * 1.0) * (w.lv / w.T / k.Rv - 1);
    args.Fd = k.rho_w * k.Rv * w.T / (Dr * 1.0) / w.pvs;
    const double r_dr_dt_old = (w.RH - RH_eq) / (args.Fk + args.Fd);
    const double mass_old = sdm_exp(x_old);
    const double dm_dt_old = 4 * k.PI * k.rho_w * r_old * r_dr_dt_old;
    dx_old = w.timestep * (dm_dt_old / mass_old);
  }
  double x_new = x_old;
  if (dx_old != 0) {
    double a = x_old;
    double b = py_max(x_insane, a + dx_old);
    double fa = minfun(k, a, args);
    double fb = minfun(k, b, args);
    int counter = 0;
    while (!(fa * fb < 0)) {
      counter += 1;
      if (counter > w.max_iters) {
        *ok = 0;
        return m;
      }
      b = py_max(x_insane, a + dx_old * sdm_pow2i(counter));  // math.ldexp
      fb = minfun(k, b, args);
    }
    if (a != b) {
      if (a > b) {
        double t = a; a = b; b = t;
        t = fa; fa = fb; fb = t;
      }
      int iters;
      x_new = toms748_solve(k, args, a, b, fa, fb, w.rtol_x, w.max_iters, &iters);
      if (iters == -1 || iters == w.max_iters) {
        *ok = 0;
        return m;
      }
    }
  }
  *ok = 1;
  return sdm_exp(x_new);
}

struct CondArgs {
  int64_t n_sd, n_cell;
  const int64_t *cell_start, *idx, *multiplicity, *cell_order;
  double *water_mass;
  const double *v_cr, *vdry, *kappa, *rhod, *thd, *qv, *prhod;
  double *pthd, *pqv, *RH_max;
  int64_t *n_substeps, *n_activating, *n_deactivating, *n_ripening;
  uint8_t *success;
  double dv, rtol_x, rtol_thd, timestep, RH_rtol;
  int64_t n_min, n_max;
  int adaptive, fuse, multiplier, max_iters;
  Kc k;
};

struct StepOut {
  double qv, thd, RH_max;
  int64_t n_activating, n_deactivating, n_ripening;
  int success;
};

// one workgroup = one cell; see the head of this file
struct CellSolver {
  const CondArgs &g;
  const int64_t *cidx;  // idx + cell_start
  int64_t n;            // super-droplets in the cell
  int tid;
  // registers: positions tid + s * COND_CB, s < COND_CR
  int64_t c_drop[COND_CR], c_mult[COND_CR];
  double c_m[COND_CR], c_rd3[COND_CR], c_kappa[COND_CR], c_xins[COND_CR], c_mcr[COND_CR];
  // LDS
  double *col;
  int *s_badq;
  double *s_sum, *s_probe;
  int64_t *s_fail;
  unsigned long long *s_cnt;

  DF void load(int64_t drop, int64_t &mult, double &m, double &rd3, double &kappa,
                       double &xins, double &mcr) const {
    const Kc &k = g.k;
    mult = g.multiplicity[drop];
    m = g.water_mass[drop];
    const double vdry = g.vdry[drop];
    rd3 = vdry / k.PI_4_3;
    kappa = g.kappa[drop];
    xins = sdm_log(k.rho_w * (vdry / 100));  // cm.py:436-440
    mcr = k.rho_w * g.v_cr[drop];            // cm.py:531-533
  }

  DF void init() {
#pragma unroll
    for (int s = 0; s < COND_CR; ++s) {
      const int64_t q = tid + s * COND_CB;
      c_drop[s] = -1;
      c_mult[s] = 0;
      c_m[s] = c_rd3[s] = c_kappa[s] = c_xins[s] = c_mcr[s] = 0;
      if (q < n) {
        const int64_t drop = cidx[q];
        if (drop >= 0 && drop < g.n_sd) {
          c_drop[s] = drop;
          load(drop, c_mult[s], c_m[s], c_rd3[s], c_kappa[s], c_xins[s], c_mcr[s]);
        }
      }
    }
  }

  // lane 0 adds col[0 .. len) to *s_sum in order, stopping at the first failed position of the
  // chunk (*s_badq, an atomicMin of the lanes that failed; reset here for the next chunk) and
  // setting *s_fail to its cell position.  The loads run ahead in batches of 16 so that the walk
  // waits on the add chain, not on LDS latency; the order of the additions is the reference's.
  DF double walk(double sum, int stop) const {
    int q = 0;
    for (; q + 16 <= stop; q += 16) {
      double v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = col[q + j];
#pragma unroll
      for (int j = 0; j < 16; ++j) sum += v[j];
    }
    for (; q < stop; ++q) sum += col[q];
    return sum;
  }

  DF void serial_sum(int64_t base, int len, bool flags) {
    __syncthreads();
    if (tid == 0) {
      int stop = len;
      if (flags) {
        const int first_bad = *s_badq;
        if (first_bad < len) {
          stop = first_bad;
          *s_fail = base + first_bad;
        }
        *s_badq = COND_CH;
      }
      *s_sum = walk(*s_sum, stop);
#ifdef SDM_COND_SERIAL_TWICE
      // measurement variant (scripts/condensation_timing.py): the same walk once more, its sum
      // stored (volatile: the compiler may not drop the walk) where nothing reads it - the time
      // difference is the cost of one serial chain
      *(volatile double *)s_probe = walk(0.0, stop);
#endif
    }
    __syncthreads();
  }

  // calculate_ml_old, cm.py:359-368
  DF double ml_old() {
    if (tid == 0) *s_sum = 0.0;
    for (int64_t base = 0; base < n; base += COND_CH) {
      const int len = (int)(n - base < COND_CH ? n - base : COND_CH);
#pragma unroll
      for (int s = 0; s < COND_CR; ++s) {
        const int64_t q = base + tid + s * COND_CB;
        if (q >= n) continue;
        int64_t mult = 0;
        double m = 0;
        if (base == 0) {
          mult = c_mult[s];
          m = c_m[s];
        } else {
          const int64_t drop = cidx[q];
          if (drop >= 0 && drop < g.n_sd) {
            mult = g.multiplicity[drop];
            m = g.water_mass[drop];
          }
        }
        col[tid + s * COND_CB] = m > 0 ? (double)mult * m : 0.0;
      }
      serial_sum(base, len, false);
    }
    const double r = *s_sum;
    __syncthreads();
    return r;
  }

  // calculate_ml_new, cm.py:399-557 (fake: no counters, no writes)
  DF double ml_new(const Cellwide &w, bool fake, int *success, int64_t *n_act,
                           int64_t *n_deact, int64_t *n_rip) {
    const Kc &k = g.k;
    if (tid == 0) {
      *s_sum = 0.0;
      *s_fail = n;
      *s_badq = COND_CH;
      s_cnt[0] = s_cnt[1] = s_cnt[2] = 0;
    }
    __syncthreads();
    unsigned long long act = 0, deact = 0, grow = 0;
    for (int64_t base = 0; base < n; base += COND_CH) {
      const int len = (int)(n - base < COND_CH ? n - base : COND_CH);
      double m_new[COND_CR];
#pragma unroll
      for (int s = 0; s < COND_CR; ++s) {
        const int64_t q = base + tid + s * COND_CB;
        m_new[s] = 0;
        if (q >= n) continue;
        int64_t drop = -1, mult = 0;
        double m = 0, rd3 = 0, kappa = 0, xins = 0, mcr = 0;
        if (base == 0) {
          drop = c_drop[s]; mult = c_mult[s]; m = c_m[s]; rd3 = c_rd3[s];
          kappa = c_kappa[s]; xins = c_xins[s];
        } else {
          drop = cidx[q];
          if (drop >= 0 && drop < g.n_sd) load(drop, mult, m, rd3, kappa, xins, mcr);
          else drop = -1;
        }
        int ok = 1;
        double contribution = 0.0;
        if (drop >= 0 && m > 0) {
          m_new[s] = drop_new_mass(k, w, m, rd3, kappa, xins, &ok);
          contribution = (double)mult * m_new[s];
        }
        col[tid + s * COND_CB] = contribution;
        if (!ok) atomicMin(s_badq, (int)(tid + s * COND_CB));
      }
      serial_sum(base, len, true);
      const int64_t fail = *s_fail;
      if (!fake) {
#pragma unroll
        for (int s = 0; s < COND_CR; ++s) {
          const int64_t q = base + tid + s * COND_CB;
          if (q >= n || q >= fail) continue;
          int64_t drop, mult;
          double m, mcr;
          if (base == 0) {
            drop = c_drop[s]; mult = c_mult[s]; m = c_m[s]; mcr = c_mcr[s];
          } else {
            drop = cidx[q];
            if (drop < 0 || drop >= g.n_sd) continue;
            mult = g.multiplicity[drop];
            m = g.water_mass[drop];
            mcr = k.rho_w * g.v_cr[drop];
          }
          if (drop < 0 || !(m > 0)) continue;
          const double mn = m_new[s];
          if (mn > mcr && mn > m) grow += (unsigned long long)mult;
          if (mn > mcr && mcr > m) act += (unsigned long long)mult;
          if (mn < mcr && mcr < m) deact += (unsigned long long)mult;
          if (base == 0) c_m[s] = mn;
          else g.water_mass[drop] = mn;
        }
      }
      if (fail < n) break;  // uniform: read from LDS after the barrier
    }
    double result = *s_sum;
    *success = *s_fail >= n;
    if (!fake) {
      if (act) atomicAdd(&s_cnt[0], act);
      if (deact) atomicAdd(&s_cnt[1], deact);
      if (grow) atomicAdd(&s_cnt[2], grow);
      __syncthreads();
      *n_act = (int64_t)s_cnt[0];
      *n_deact = (int64_t)s_cnt[1];
      *n_rip = *n_deact > 0 ? (int64_t)s_cnt[2] : 0;
    }
    __syncthreads();
    return result;
  }

  // step_impl, cm.py:249-357
  DF StepOut step_impl(double thd, double qv, double rhod, double dthd_dt,
                               double dqv_dt, double drhod_dt, double m_d, double timestep,
                               int64_t n_substeps, bool fake) {
    const Kc &k = g.k;
    timestep /= (double)n_substeps;
    double ml_o = ml_old();
    StepOut o = {0, 0, 0, 0, 0, 0, 1};
    for (int64_t it = 0; it < n_substeps; ++it) {
      thd += timestep * dthd_dt / 2;
      qv += timestep * dqv_dt / 2;
      rhod += timestep * drhod_dt / 2;
      Cellwide w;
      w.T = svt_T(k, rhod, thd);
      const double p = svt_p(k, rhod, w.T, qv);
      const double pv = svt_pv(k, p, qv);
      w.lv = lv_of(k, w.T);
      w.pvs = pvs_water(k, w.T);
      w.DTp = k.D0;  // diffusion_thermics/neglect.py
      w.KTp = k.K0;
      w.RH = pv / w.pvs;
      // fuchs_sutugin.py:14-18
      w.lambdaK = (4.0 / 5) * k.K0 * w.T / p / SDM_MATH_SQRT(2 * k.Rd * w.T);
      w.lambdaD = w.DTp / SDM_MATH_SQRT(2 * k.Rv * w.T);
      w.timestep = timestep;
      w.rtol_x = g.rtol_x;
      w.RH_rtol = g.RH_rtol;
      w.max_iters = g.max_iters;
      int ok = 1;
      int64_t na = 0, nd = 0, nr = 0;
      const double ml_n = ml_new(w, fake, &ok, &na, &nd, &nr);
      const double dml_dt = (ml_n - ml_o) / timestep;
      const double dqv_corr = -dml_dt / m_d;
      const double dthd_dt_corr = -w.lv * dqv_corr / k.c_pd / w.T * thd * rhod;
      thd += timestep * (dthd_dt / 2 + dthd_dt_corr);
      qv += timestep * (dqv_dt / 2 + dqv_corr);
      rhod += timestep * drhod_dt / 2;
      ml_o = ml_n;
      o.n_activating += na;
      o.n_deactivating += nd;
      o.n_ripening += nr;
      o.RH_max = py_max(o.RH_max, w.RH);
      o.success = o.success && ok;
    }
    o.qv = qv;
    o.thd = thd;
    return o;
  }

  DF void write_back() {
#pragma unroll
    for (int s = 0; s < COND_CR; ++s)
      if (c_drop[s] >= 0) g.water_mass[c_drop[s]] = c_m[s];
  }
};

DF int64_t floordiv(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

__global__ __launch_bounds__(COND_CB) void k_condensation(CondArgs g) {
  __shared__ double col[COND_CH];
  __shared__ int s_badq;
  __shared__ double s_sum, s_probe;
  __shared__ int64_t s_fail;
  __shared__ unsigned long long s_cnt[3];
  // _condensation, cm.py:126-176
  const int64_t cell = g.cell_order[blockIdx.x];
  if (cell < 0 || cell >= g.n_cell) return;
  const int64_t start = g.cell_start[cell], end = g.cell_start[cell + 1];
  if (start < 0 || end > g.n_sd || end <= start) return;  // empty cells are skipped
  CellSolver cs{g, g.idx + start, end - start, (int)threadIdx.x};
  cs.col = col;
  cs.s_badq = &s_badq;
  cs.s_sum = &s_sum;
  cs.s_probe = &s_probe;
  cs.s_fail = &s_fail;
  cs.s_cnt = s_cnt;
  cs.init();

  const double thd = g.thd[cell], qv = g.qv[cell], rhod = g.rhod[cell];
  const double dthd_dt = (g.pthd[cell] - thd) / g.timestep;
  const double dqv_dt = (g.pqv[cell] - qv) / g.timestep;
  const double drhod_dt = (g.prhod[cell] - rhod) / g.timestep;
  const double m_d = (g.prhod[cell] + rhod) / 2 * g.dv;
  __syncthreads();  // every lane has read pthd / pqv before lane 0 writes them

  // solve, cm.py:636-698 (adapt_substeps :190-227, step_fake :231-238)
  int ok = 1;
  int64_t n = g.n_substeps[cell];
  if (g.adaptive) {
    const int64_t mult = g.multiplier;
    const int64_t fd = floordiv(n, mult);
    n = fd > g.n_min ? fd : g.n_min;
    double thd_long = 0;
    ok = 0;
    bool done = false;
    for (int burnout = 0; burnout < g.fuse + 1 && !done; ++burnout) {
      if (burnout == g.fuse) { ok = 0; n = 0; done = true; break; }
      const StepOut f = cs.step_impl(thd, qv, rhod, dthd_dt, dqv_dt, drhod_dt, m_d,
                                     g.timestep / (double)n, 1, true);
      thd_long = f.thd;
      ok = f.success;
      if (ok) break;
      n *= mult;
    }
    for (int burnout = 0; burnout < g.fuse + 1 && !done; ++burnout) {
      if (burnout == g.fuse) { ok = 0; n = 0; break; }
      const StepOut f = cs.step_impl(thd, qv, rhod, dthd_dt, dqv_dt, drhod_dt, m_d,
                                     g.timestep / (double)(n * mult), 1, true);
      ok = f.success;
      if (!ok) { n = 0; break; }
      const double dthd_long = thd_long - thd;
      const double dthd_short = f.thd - thd;
      const double error_estimate = sdm_abs(dthd_long - (double)mult * dthd_short);
      thd_long = f.thd;
      if (within_tolerance(error_estimate, thd, g.rtol_thd)) break;
      n *= mult;
      if (n > g.n_max) break;
    }
    if (ok) n = g.n_max < n ? g.n_max : n;
  }
  StepOut o;
  if (ok) {
    o = cs.step_impl(thd, qv, rhod, dthd_dt, dqv_dt, drhod_dt, m_d, g.timestep, n, false);
    cs.write_back();
  } else {
    o = StepOut{qv, thd, -1, -1, -1, -1, 0};
  }
  if (threadIdx.x == 0) {
    g.success[cell] = (uint8_t)(o.success != 0);
    g.pqv[cell] = o.qv;
    g.pthd[cell] = o.thd;
    g.n_substeps[cell] = n;
    g.n_activating[cell] = o.n_activating;
    g.n_deactivating[cell] = o.n_deactivating;
    g.n_ripening[cell] = o.n_ripening;
    g.RH_max[cell] = o.RH_max;
  }
}

// ---- ambient methods (pm.py) ---------------------------------------------------------------------
__global__ void k_temperature_pressure_rh(const double *rhod, const double *thd, const double *qv,
                                          double *T, double *p, double *RH, int64_t n, Kc k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double t = svt_T(k, rhod[i], thd[i]);  // pm.py:53-61
  const double pp = svt_p(k, rhod[i], t, qv[i]);
  T[i] = t;
  p[i] = pp;
  RH[i] = svt_pv(k, pp, qv[i]) / pvs_water(k, t);
}

__global__ void k_air_density(double *out, const double *rhod, const double *qv, int64_t n) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) out[i] = rhod[i] * (1 + qv[i]);  // libcloudphplusplus.py:58
}

__global__ void k_air_dynamic_viscosity(double *out, const double *temperature, int64_t n, Kc k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double t = temperature[i];  // zografos_et_al_1987.py:17-23
  out[i] = k.Z3 * sdm_pow(t, 3.0) + k.Z2 * sdm_pow(t, 2.0) + k.Z1 * t + k.Z0;
}

__global__ void k_critical_volume(double *v_cr, const double *kappa, const double *v_dry,
                                  const double *T, const int64_t *cell, int64_t n, Kc k) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  // pm.py:22-33; kappa_koehler_leading_terms.py:23-25 (r_cr), trivia.py:27-28 (volume)
  const double sgm = k.sgm_w;
  const double t = T[cell[i]];
  const double r_cr = SDM_MATH_SQRT(3 * kappa[i] * (v_dry[i] / k.PI_4_3) /
                                    (2 * sgm / k.Rv / t / k.rho_w));
  v_cr[i] = k.PI_4_3 * sdm_pow(r_cr, k.THREE);
}

__global__ void k_reynolds_number(double *out, const int64_t *cell_id, const double *eta,
                                  const double *rho, const double *radius, const double *u,
                                  int64_t n) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t c = cell_id[i];  // liquid_spheres.py:29-31
  out[i] = 2 * radius[i] * u[i] * rho[c] / eta[c];
}

__global__ void k_explicit_euler(double *y, int64_t n, double dt, double dy_dt) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) y[i] = y[i] + dt * dy_dt;  // trivia.py:35-36
}

}  // namespace

extern "C" int sdm_condensation(
    sdm_ctx *ctx, int64_t n_sd, int64_t n_cell, const int64_t *cell_start_arg, double *water_mass,
    const double *v_cr, const int64_t *multiplicity, const double *vdry, const int64_t *idx,
    const double *rhod, const double *thd, const double *water_vapour_mixing_ratio, double dv,
    const double *prhod, double *pthd, double *predicted_water_vapour_mixing_ratio,
    const double *kappa, const double *f_org, double rtol_x, double rtol_thd, double timestep,
    int64_t *n_substeps, int64_t *n_activating, int64_t *n_deactivating, int64_t *n_ripening,
    const int64_t *cell_order, double *RH_max, uint8_t *success, const double *reynolds_number,
    const double *air_density, const double *air_dynamic_viscosity, double dt_min, double dt_max,
    int adaptive, int fuse, int multiplier, double RH_rtol, int max_iters,
    const double consts[34]) {
  (void)f_org;  // surface_tension Constant
  (void)reynolds_number;  // ventilation Neglect
  (void)air_density;
  (void)air_dynamic_viscosity;
  ARG_TRY(ctx && n_sd >= 0 && n_cell >= 0 && consts);
  ARG_TRY(multiplier >= 1 && fuse >= 0 && max_iters >= 0 && timestep > 0);
  ARG_TRY(n_cell <= 0x7fffffff);
  if (dt_max > timestep) dt_max = timestep;  // make_adapt_substeps, cm.py:181-188
  ARG_TRY(dt_min != 0);
  if (n_cell == 0) return SDM_OK;
  ARG_TRY(cell_start_arg && cell_order && rhod && thd && water_vapour_mixing_ratio && prhod &&
          pthd && predicted_water_vapour_mixing_ratio && n_substeps && n_activating &&
          n_deactivating && n_ripening && RH_max && success);
  ARG_TRY(n_sd == 0 || (water_mass && v_cr && multiplicity && vdry && idx && kappa));
  CondArgs g;
  g.n_sd = n_sd;
  g.n_cell = n_cell;
  g.cell_start = cell_start_arg;
  g.idx = idx;
  g.multiplicity = multiplicity;
  g.cell_order = cell_order;
  g.water_mass = water_mass;
  g.v_cr = v_cr;
  g.vdry = vdry;
  g.kappa = kappa;
  g.rhod = rhod;
  g.thd = thd;
  g.qv = water_vapour_mixing_ratio;
  g.prhod = prhod;
  g.pthd = pthd;
  g.pqv = predicted_water_vapour_mixing_ratio;
  g.RH_max = RH_max;
  g.n_substeps = n_substeps;
  g.n_activating = n_activating;
  g.n_deactivating = n_deactivating;
  g.n_ripening = n_ripening;
  g.success = success;
  g.dv = dv;
  g.rtol_x = rtol_x;
  g.rtol_thd = rtol_thd;
  g.timestep = timestep;
  g.RH_rtol = RH_rtol;
  g.n_min = (int64_t)ceil(timestep / dt_max);
  g.n_max = (int64_t)floor(timestep / dt_min);
  g.adaptive = adaptive;
  g.fuse = fuse;
  g.multiplier = multiplier;
  g.max_iters = max_iters;
  g.k = consts_of(consts);
  hipLaunchKernelGGL(k_condensation, dim3((unsigned)n_cell), dim3(COND_CB), 0, ctx->stream, g);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_temperature_pressure_rh(sdm_ctx *ctx, const double *rhod, const double *thd,
                                           const double *water_vapour_mixing_ratio, double *T,
                                           double *p, double *RH, int64_t n,
                                           const double consts[34]) {
  ARG_TRY(ctx && n >= 0 && consts);
  if (n == 0) return SDM_OK;
  ARG_TRY(rhod && thd && water_vapour_mixing_ratio && T && p && RH);
  hipLaunchKernelGGL(k_temperature_pressure_rh, GRID1D(n), rhod, thd, water_vapour_mixing_ratio,
                     T, p, RH, n, consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_air_density(sdm_ctx *ctx, double *output, const double *rhod,
                               const double *water_vapour_mixing_ratio, int64_t n) {
  ARG_TRY(ctx && n >= 0);
  if (n == 0) return SDM_OK;
  ARG_TRY(output && rhod && water_vapour_mixing_ratio);
  hipLaunchKernelGGL(k_air_density, GRID1D(n), output, rhod, water_vapour_mixing_ratio, n);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_air_dynamic_viscosity(sdm_ctx *ctx, double *output, const double *temperature,
                                         int64_t n, const double consts[34]) {
  ARG_TRY(ctx && n >= 0 && consts);
  if (n == 0) return SDM_OK;
  ARG_TRY(output && temperature);
  hipLaunchKernelGGL(k_air_dynamic_viscosity, GRID1D(n), output, temperature, n,
                     consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_critical_volume(sdm_ctx *ctx, double *v_cr, const double *kappa,
                                   const double *f_org, const double *v_dry, const double *v_wet,
                                   const double *T, const int64_t *cell, int64_t n,
                                   const double consts[34]) {
  (void)f_org;  // surface_tension Constant: sigma ignores the volumes and f_org
  (void)v_wet;
  ARG_TRY(ctx && n >= 0 && consts);
  if (n == 0) return SDM_OK;
  ARG_TRY(v_cr && kappa && v_dry && T && cell);
  hipLaunchKernelGGL(k_critical_volume, GRID1D(n), v_cr, kappa, v_dry, T, cell, n,
                     consts_of(consts));
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_reynolds_number(sdm_ctx *ctx, double *output, const int64_t *cell_id,
                                   const double *dynamic_viscosity, const double *density,
                                   const double *radius, const double *velocity_wrt_air,
                                   int64_t n) {
  ARG_TRY(ctx && n >= 0);
  if (n == 0) return SDM_OK;
  ARG_TRY(output && cell_id && dynamic_viscosity && density && radius && velocity_wrt_air);
  hipLaunchKernelGGL(k_reynolds_number, GRID1D(n), output, cell_id, dynamic_viscosity, density,
                     radius, velocity_wrt_air, n);
  LAUNCH_CHECK();
  return SDM_OK;
}

extern "C" int sdm_explicit_euler(sdm_ctx *ctx, double *y, int64_t n, double dt, double dy_dt) {
  ARG_TRY(ctx && n >= 0);
  if (n == 0) return SDM_OK;
  ARG_TRY(y);
  hipLaunchKernelGGL(k_explicit_euler, GRID1D(n), y, n, dt, dy_dt);
  LAUNCH_CHECK();
  return SDM_OK;
}

// condensation_solver.h -- PySDM's condensation solver for gfx950 as a template over a formulae
// policy.  Two instantiations: condensation.hip (PySDM's default formulae inlined, the kernel of
// sdm_condensation) and condensation_formulae.hip (every choice of include/
// sdm_condensation_formulae.h behind kernel-uniform switches, the kernel of sdm_condensation_f).
//
// Reference: PySDM/backends/impl_numba/methods/condensation_methods.py ("cm.py") and toms748.py.
//
// One workgroup per cell (the cells are independent: cm.py:102-176 gives each cell its own
// solver call).  The whole adaptive loop runs in the kernel: fake steps (adapt_substeps), then
// the real sub-steps; the cell's scalars (T, p, pv, lv, pvs, lambdaK, lambdaD, RH, ...) are
// computed by every lane from the same values (uniform); each droplet's bracket search and
// TOMS748 run in registers of its lane.  The cell's super-droplets are strided over the 256
// lanes: position q of the cell (idx[cell_start + q]) belongs to lane q % 256; the first
// COND_CH = 1024 positions keep their per-call constants (drop id, multiplicity, rd3, kappa,
// x_insane, mass at v_cr) and their water mass in registers for the whole call, later positions
// (chunks of COND_CH) are read from HBM on each pass.  What a policy reads per droplet beyond
// these (f_org and the Reynolds number) has no registers left: the first COND_CH positions keep
// it in LDS (P::STAGE doubles), later ones read it from HBM on each pass like the other columns.
//
// Bit parity with the reference's serial loop: the sums of n * m (calculate_ml_old / _new) are
// formed in the order of the cell's permutation - every lane writes its n * m into an LDS column
// and lane 0 adds the column up serially, chunk after chunk.  A failed droplet (no bracket within
// max_iters, or TOMS748 failing) ends the reference's droplet loop (cm.py:496,515): lane 0's walk
// stops at the first failed position (an atomicMin over the lanes that failed), droplets at and
// after it keep their mass and add nothing, and success goes to 0 - nothing traps.  All arithmetic
// is IEEE double without contraction (-ffp-contract=off) and exp / log / pow come from sdm_math.h,
// so the CPU checkers get the same bits.
//
// A policy P provides
//   K                      the constants (and whatever else the formulae read), part of CondArgs
//   Extra                  per-droplet inputs beyond the cached ones; STAGE, stage_put / stage_get
//                          and extra_of: their LDS staging and their HBM read
//   Cellwide               the sub-step's cell scalars; cellwide() fills T, RH, lv and its own
//   MinArgs, minfun        cm.py:366-397
//   x_of, mass_of          the diffusion coordinate
//   start                  the head of the per-droplet body of calculate_ml_new: x_old, the
//                          minfun arguments and dx_old (0: the droplet keeps its mass)
//   failed                 whether an evaluation failed inside the formulae
//   rho_w, c_pd            the two constants the shared code reads itself
#ifndef SDM_CONDENSATION_SOLVER_H
#define SDM_CONDENSATION_SOLVER_H
#include "common.h"

#define COND_CB 256                // lanes per workgroup
#define COND_CR 4                  // register-cached positions per lane
#define COND_CH (COND_CB * COND_CR)  // positions per chunk

namespace {

#define DF __device__ __forceinline__
DF double py_max(double x, double y) { return y > x ? y : x; }  // Python's max / min
DF double py_min(double x, double y) { return y < x ? y : x; }
DF int within_tolerance(double e, double value, double rtol) { return e < rtol * sdm_abs(value); }

// ---- TOMS748 (toms748.py) ------------------------------------------------------------------------
#define T_EPS 2.220446049250313e-16
#define T_MAX 1.7976931348623157e308
#define T_MIN 2.2250738585072014e-308

template <class P>
DF void bracket(const typename P::K &k, typename P::MinArgs &args, double &a, double &b, double c,
                double &fa, double &fb, double &d, double &fd) {  // :24-47
  const double tol = T_EPS * 2;
  if ((b - a) < 2 * tol * a) c = a + (b - a) / 2;
  else if (c <= a + sdm_abs(a) * tol) c = a + sdm_abs(a) * tol;
  else if (c >= b - sdm_abs(b) * tol) c = b - sdm_abs(a) * tol;
  const double fc = P::minfun(k, c, args);
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
template <class P>
DF double toms748_solve(const typename P::K &k, typename P::MinArgs &args, double ax, double bx,
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
    bracket<P>(k, args, a, b, c, fa, fb, d, fd);
    count -= 1;
    if (count > 0 && fa != 0 && !tol_check(a, b, rtol)) {
      c = quadratic_interpolate(a, b, d, fa, fb, fd, 2);
      e = d;
      fe = fd;
      bracket<P>(k, args, a, b, c, fa, fb, d, fd);
      count -= 1;
    }
  }
  while (count > 0 && fa != 0 && !tol_check(a, b, rtol)) {
    const double a0 = a, b0 = b;
    if (prof_of(fa, fb, fd, fe)) c = quadratic_interpolate(a, b, d, fa, fb, fd, 2);
    else c = cubic_interpolate(a, b, d, e, fa, fb, fd, fe);
    e = d;
    fe = fd;
    bracket<P>(k, args, a, b, c, fa, fb, d, fd);
    if (count == 1 || fa == 0 || tol_check(a, b, rtol)) { count -= 1; break; }
    if (prof_of(fa, fb, fd, fe)) c = quadratic_interpolate(a, b, d, fa, fb, fd, 3);
    else c = cubic_interpolate(a, b, d, e, fa, fb, fd, fe);
    bracket<P>(k, args, a, b, c, fa, fb, d, fd);
    if (count == 1 || fa == 0 || tol_check(a, b, rtol)) { count -= 1; break; }
    double u, fu;
    if (sdm_abs(fa) < sdm_abs(fb)) { u = a; fu = fa; } else { u = b; fu = fb; }
    c = u - 2 * (fu / (fb - fa)) * (b - a);
    if (sdm_abs(c - u) > (b - a) / 2) c = a + (b - a) / 2;
    e = d;
    fe = fd;
    bracket<P>(k, args, a, b, c, fa, fb, d, fd);
    if (count == 1 || fa == 0 || tol_check(a, b, rtol)) { count -= 1; break; }
    if ((b - a) < mu * (b0 - a0)) continue;
    e = d;
    fe = fd;
    bracket<P>(k, args, a, b, a + (b - a) / 2, fa, fb, d, fd);
    count -= 1;
  }
  *iters = max_iter - count;
  if (fa == 0) b = a;
  else if (fb == 0) a = b;
  return (a + b) / 2;
}

// the per-droplet body of calculate_ml_new (cm.py:429-556) for a droplet with water mass m > 0;
// returns the new mass, *ok = 0 where the reference sets success = False and breaks
template <class P>
__device__ __attribute__((noinline)) double drop_new_mass(
    const typename P::K &k, const typename P::Cellwide &w, double m, double rd3, double kappa,
    double x_insane, typename P::Extra extra, int *ok) {
  typename P::MinArgs args;
  double x_old, dx_old;
  P::start(k, w, m, rd3, kappa, extra, args, x_old, dx_old);
  double x_new = x_old;
  if (dx_old != 0) {
    double a = x_old;
    double b = py_max(x_insane, a + dx_old);
    double fa = P::minfun(k, a, args);
    double fb = P::minfun(k, b, args);
    int counter = 0;
    while (!(fa * fb < 0)) {
      counter += 1;
      if (counter > w.max_iters) {
        *ok = 0;
        return m;
      }
      b = py_max(x_insane, a + dx_old * sdm_pow2i(counter));  // math.ldexp
      fb = P::minfun(k, b, args);
    }
    if (a != b) {
      if (a > b) {
        double t = a; a = b; b = t;
        t = fa; fa = fb; fb = t;
      }
      int iters;
      x_new = toms748_solve<P>(k, args, a, b, fa, fb, w.rtol_x, w.max_iters, &iters);
      if (iters == -1 || iters == w.max_iters) {
        *ok = 0;
        return m;
      }
    }
  }
  if (P::failed(args)) {
    *ok = 0;
    return m;
  }
  *ok = 1;
  return P::mass_of(k, x_new);
}

template <class P>
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
  typename P::K k;
};

struct StepOut {
  double qv, thd, RH_max;
  int64_t n_activating, n_deactivating, n_ripening;
  int success;
};

// one workgroup = one cell; see the head of this file
template <class P>
struct CellSolver {
  const CondArgs<P> &g;
  const int64_t *cidx;  // idx + cell_start
  int64_t n;            // super-droplets in the cell
  int64_t cell;
  int tid;
  // registers: positions tid + s * COND_CB, s < COND_CR
  int64_t c_drop[COND_CR], c_mult[COND_CR];
  double c_m[COND_CR], c_rd3[COND_CR], c_kappa[COND_CR], c_xins[COND_CR], c_mcr[COND_CR];
  // LDS
  double *col;
  double *stage;  // P::STAGE doubles (nullptr if none)
  int *s_badq;
  double *s_sum, *s_probe;
  int64_t *s_fail;
  unsigned long long *s_cnt;

  DF void load(int64_t drop, int64_t &mult, double &m, double &rd3, double &kappa,
                       double &xins, double &mcr) const {
    const typename P::K &k = g.k;
    mult = g.multiplicity[drop];
    m = g.water_mass[drop];
    const double vdry = g.vdry[drop];
    rd3 = vdry / P::pi_4_3(k);
    kappa = g.kappa[drop];
    xins = P::x_of(k, P::rho_w(k) * (vdry / 100));  // cm.py:436-440
    mcr = P::rho_w(k) * g.v_cr[drop];               // cm.py:531-533
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
          if constexpr (P::STAGE > 0) P::stage_put(stage, (int)q, P::extra_of(g.k, drop));
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
  DF double ml_new(const typename P::Cellwide &w, bool fake, int *success, int64_t *n_act,
                           int64_t *n_deact, int64_t *n_rip) {
    const typename P::K &k = g.k;
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
        typename P::Extra extra = {};
        if (base == 0) {
          drop = c_drop[s]; mult = c_mult[s]; m = c_m[s]; rd3 = c_rd3[s];
          kappa = c_kappa[s]; xins = c_xins[s];
          if constexpr (P::STAGE > 0)
            if (drop >= 0) extra = P::stage_get(stage, tid + s * COND_CB);
        } else {
          drop = cidx[q];
          if (drop >= 0 && drop < g.n_sd) {
            load(drop, mult, m, rd3, kappa, xins, mcr);
            if constexpr (P::STAGE > 0) extra = P::extra_of(k, drop);
          } else {
            drop = -1;
          }
        }
        int ok = 1;
        double contribution = 0.0;
        if (drop >= 0 && m > 0) {
          m_new[s] = drop_new_mass<P>(k, w, m, rd3, kappa, xins, extra, &ok);
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
            mcr = P::rho_w(k) * g.v_cr[drop];
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
    const typename P::K &k = g.k;
    timestep /= (double)n_substeps;
    double ml_o = ml_old();
    StepOut o = {0, 0, 0, 0, 0, 0, 1};
    for (int64_t it = 0; it < n_substeps; ++it) {
      thd += timestep * dthd_dt / 2;
      qv += timestep * dqv_dt / 2;
      rhod += timestep * drhod_dt / 2;
      typename P::Cellwide w;
      P::cellwide(g, cell, rhod, thd, qv, w);
      w.timestep = timestep;
      w.rtol_x = g.rtol_x;
      w.RH_rtol = g.RH_rtol;
      w.max_iters = g.max_iters;
      int ok = 1;
      int64_t na = 0, nd = 0, nr = 0;
      const double ml_n = ml_new(w, fake, &ok, &na, &nd, &nr);
      const double dml_dt = (ml_n - ml_o) / timestep;
      const double dqv_corr = -dml_dt / m_d;
      const double dthd_dt_corr = -w.lv * dqv_corr / P::c_pd(k) / w.T * thd * rhod;
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

// the LDS of one workgroup's CellSolver (one set per kernel: declared where this is inlined)
template <class P>
DF void attach_lds(CellSolver<P> &cs) {
  __shared__ double col[COND_CH];
  __shared__ int s_badq;
  __shared__ double s_sum, s_probe;
  __shared__ int64_t s_fail;
  __shared__ unsigned long long s_cnt[3];
  double *stage = nullptr;
  if constexpr (P::STAGE > 0) {
    __shared__ double s_stage[P::STAGE > 0 ? P::STAGE : 1];
    stage = s_stage;
  }
  cs.col = col;
  cs.stage = stage;
  cs.s_badq = &s_badq;
  cs.s_sum = &s_sum;
  cs.s_probe = &s_probe;
  cs.s_fail = &s_fail;
  cs.s_cnt = s_cnt;
}

struct SolveOut {
  StepOut o;
  int64_t n;  // the sub-step count used
  int ran;    // the real step ran (the register-cached masses are the new ones)
};

// the solve proper (solve, cm.py:636-698; adapt_substeps :190-227, step_fake :231-238) with the
// cell's scalars as arguments: k_condensation(_f) read them from CondArgs (condensation_cell), the
// parcel kernels keep them in registers from step to step (parcel_solver.h).  `n`: the previous
// sub-step count.  The caller has run cs.init() and calls cs.write_back() if `ran`.
template <class P>
DF SolveOut solve_cell(CellSolver<P> &cs, const CondArgs<P> &g, double thd, double qv,
                       double rhod, double prhod, double pthd, double pqv, double dv, int64_t n) {
  const double dthd_dt = (pthd - thd) / g.timestep;
  const double dqv_dt = (pqv - qv) / g.timestep;
  const double drhod_dt = (prhod - rhod) / g.timestep;
  const double m_d = (prhod + rhod) / 2 * dv;
  int ok = 1;
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
  SolveOut s;
  s.n = n;
  s.ran = ok;
  if (ok) s.o = cs.step_impl(thd, qv, rhod, dthd_dt, dqv_dt, drhod_dt, m_d, g.timestep, n, false);
  else s.o = StepOut{qv, thd, -1, -1, -1, -1, 0};
  return s;
}

// the body of the kernel of either instantiation (_condensation, cm.py:126-176): the cell's
// scalars from CondArgs, the solve proper, the cell's results
template <class P>
DF void condensation_cell(const CondArgs<P> &g) {
  const int64_t cell = g.cell_order[blockIdx.x];
  if (cell < 0 || cell >= g.n_cell) return;
  const int64_t start = g.cell_start[cell], end = g.cell_start[cell + 1];
  if (start < 0 || end > g.n_sd || end <= start) return;  // empty cells are skipped
  CellSolver<P> cs{g, g.idx + start, end - start, cell, (int)threadIdx.x};
  attach_lds<P>(cs);
  cs.init();

  const double thd = g.thd[cell], qv = g.qv[cell], rhod = g.rhod[cell];
  const double prhod = g.prhod[cell], pthd = g.pthd[cell], pqv = g.pqv[cell];
  __syncthreads();  // every lane has read pthd / pqv before lane 0 writes them

  const SolveOut s = solve_cell<P>(cs, g, thd, qv, rhod, prhod, pthd, pqv, g.dv,
                                   g.n_substeps[cell]);
  if (s.ran) cs.write_back();
  if (threadIdx.x == 0) {
    g.success[cell] = (uint8_t)(s.o.success != 0);
    g.pqv[cell] = s.o.qv;
    g.pthd[cell] = s.o.thd;
    g.n_substeps[cell] = s.n;
    g.n_activating[cell] = s.o.n_activating;
    g.n_deactivating[cell] = s.o.n_deactivating;
    g.n_ripening[cell] = s.o.n_ripening;
    g.RH_max[cell] = s.o.RH_max;
  }
}

}  // namespace

// the argument checks and the CondArgs fields both entry points share; `g.k` is the caller's
#define SDM_COND_FILL_ARGS(g)                                                                  \
  do {                                                                                         \
    ARG_TRY(ctx && n_sd >= 0 && n_cell >= 0 && consts);                                        \
    ARG_TRY(multiplier >= 1 && fuse >= 0 && max_iters >= 0 && timestep > 0);                   \
    ARG_TRY(n_cell <= 0x7fffffff);                                                             \
    if (dt_max > timestep) dt_max = timestep; /* make_adapt_substeps, cm.py:181-188 */         \
    ARG_TRY(dt_min != 0);                                                                      \
    if (n_cell == 0) return SDM_OK;                                                            \
    ARG_TRY(cell_start_arg && cell_order && rhod && thd && water_vapour_mixing_ratio &&        \
            prhod && pthd && predicted_water_vapour_mixing_ratio && n_substeps &&              \
            n_activating && n_deactivating && n_ripening && RH_max && success);                \
    ARG_TRY(n_sd == 0 || (water_mass && v_cr && multiplicity && vdry && idx && kappa));        \
    (g).n_sd = n_sd;                                                                           \
    (g).n_cell = n_cell;                                                                       \
    (g).cell_start = cell_start_arg;                                                           \
    (g).idx = idx;                                                                             \
    (g).multiplicity = multiplicity;                                                           \
    (g).cell_order = cell_order;                                                               \
    (g).water_mass = water_mass;                                                               \
    (g).v_cr = v_cr;                                                                           \
    (g).vdry = vdry;                                                                           \
    (g).kappa = kappa;                                                                         \
    (g).rhod = rhod;                                                                           \
    (g).thd = thd;                                                                             \
    (g).qv = water_vapour_mixing_ratio;                                                        \
    (g).prhod = prhod;                                                                         \
    (g).pthd = pthd;                                                                           \
    (g).pqv = predicted_water_vapour_mixing_ratio;                                             \
    (g).RH_max = RH_max;                                                                       \
    (g).n_substeps = n_substeps;                                                               \
    (g).n_activating = n_activating;                                                           \
    (g).n_deactivating = n_deactivating;                                                       \
    (g).n_ripening = n_ripening;                                                               \
    (g).success = success;                                                                     \
    (g).dv = dv;                                                                               \
    (g).rtol_x = rtol_x;                                                                       \
    (g).rtol_thd = rtol_thd;                                                                   \
    (g).timestep = timestep;                                                                   \
    (g).RH_rtol = RH_rtol;                                                                     \
    (g).n_min = (int64_t)ceil(timestep / dt_max);                                              \
    (g).n_max = (int64_t)floor(timestep / dt_min);                                             \
    (g).adaptive = adaptive;                                                                   \
    (g).fuse = fuse;                                                                           \
    (g).multiplier = multiplier;                                                               \
    (g).max_iters = max_iters;                                                                 \
  } while (0)

#endif  // SDM_CONDENSATION_SOLVER_H

/*
 * toms748.h -- the TOMS748 root search of the reference, PySDM/backends/impl_numba/toms748.py,
 * line for line (bracket, safe_div, secant / quadratic / cubic interpolation, toms748_solve), for
 * both compilers of this project (hipcc for gfx950, gcc for the CPU checker).
 *
 * Parametrised on the function the way a C header can be: the includer defines, before the
 * #include,
 *   TOMS748_FN            the qualifiers of every function here (e.g. SDM_MATH_FN)
 *   TOMS748_ARGS          the type of the function's arguments, passed by const pointer
 *   TOMS748_EVAL(x, args) the function value at x
 *   TOMS748_NAME(name)    optional: how `toms748_solve` (and its `toms748_bracket`) are named,
 *                         for a translation unit that searches on two functions: it includes this
 *                         file once per function, the second time with e.g. name##_wet
 * and gets `toms748_solve`.  The chemistry path, condensation_formulae.h and the initialisation
 * path include it (condensation.hip keeps the transcription bound to its own function).  Every
 * loop is bounded by max_iter or a constant.
 * Where the reference warns and returns (nan, -1) - not a < b, not fa * fb < 0 - this returns NaN
 * with *iters = -1 and does not warn.
 */
#ifndef SDM_TOMS748_H
#define SDM_TOMS748_H

#define TOMS748_EPS 2.220446049250313e-16     /* sys.float_info.epsilon */
#define TOMS748_MAX 1.7976931348623157e308    /* sys.float_info.max */
#define TOMS748_MIN 2.2250738585072014e-308   /* sys.float_info.min */

typedef struct toms748_state { double a, b, fa, fb, d, fd; } toms748_state;

TOMS748_FN double toms748_abs(double x) { return x < 0 ? -x : (x == 0 ? 0.0 : x); }

/* toms748.py:53-57 */
TOMS748_FN double toms748_safe_div(double num, double denom, double r) {
  if (toms748_abs(denom) < 1)
    if (toms748_abs(denom * TOMS748_MAX) <= toms748_abs(num)) return r;
  return num / denom;
}

/* toms748.py:61-66 */
TOMS748_FN double toms748_secant(double a, double b, double fa, double fb) {
  const double tol = TOMS748_EPS * 5;
  const double c = a - (fa / (fb - fa)) * (b - a);
  if (c <= a + toms748_abs(a) * tol || c >= b - toms748_abs(b) * tol) return (a + b) / 2;
  return c;
}

/* toms748.py:70-87 (count is 2 or 3) */
TOMS748_FN double toms748_quadratic(double a, double b, double d, double fa, double fb, double fd,
                                    int count) {
  const double B = toms748_safe_div(fb - fa, b - a, TOMS748_MAX);
  double A = toms748_safe_div(fd - fb, d - b, TOMS748_MAX);
  A = toms748_safe_div(A - B, d - a, 0.0);
  if (A == 0) return toms748_secant(a, b, fa, fb);
  double c = A * fa > 0 ? a : b;
  for (int i = 1; i <= 3; ++i)
    if (i <= count)
      c -= toms748_safe_div(fa + (B + A * (c - b)) * (c - a), B + A * (2.0 * c - a - b),
                            1.0 + c - a);
  if (c <= a || c >= b) c = toms748_secant(a, b, fa, fb);
  return c;
}

/* toms748.py:91-106 */
TOMS748_FN double toms748_cubic(double a, double b, double d, double e, double fa, double fb,
                                double fd, double fe) {
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
  if (c <= a || c >= b) c = toms748_quadratic(a, b, d, fa, fb, fd, 3);
  return c;
}

/* toms748.py:110-111 with trivia.within_tolerance: error_estimate < rtol * abs(value) */
TOMS748_FN int toms748_tol_check(double a, double b, double rtol) {
  const double aa = toms748_abs(a), ab = toms748_abs(b);
  return toms748_abs(a - b) < rtol * toms748_abs(ab < aa ? ab : aa);
}

TOMS748_FN int toms748_prof(double fa, double fb, double fd, double fe) {
  const double min_diff = TOMS748_MIN * 32;
  return toms748_abs(fa - fb) < min_diff || toms748_abs(fa - fd) < min_diff ||
         toms748_abs(fa - fe) < min_diff || toms748_abs(fb - fd) < min_diff ||
         toms748_abs(fb - fe) < min_diff || toms748_abs(fd - fe) < min_diff;
}

#endif /* SDM_TOMS748_H */

/* ---- the part that depends on the function: once per inclusion ------------------------------ */
#ifndef TOMS748_NAME
#define TOMS748_NAME(name) name
#endif

/* toms748.py:24-49 */
TOMS748_FN void TOMS748_NAME(toms748_bracket)(const TOMS748_ARGS *args, toms748_state *s,
                                              double c) {
  const double tol = TOMS748_EPS * 2;
  double a = s->a, b = s->b;
  if ((b - a) < 2 * tol * a)
    c = a + (b - a) / 2;
  else if (c <= a + toms748_abs(a) * tol)
    c = a + toms748_abs(a) * tol;
  else if (c >= b - toms748_abs(b) * tol)
    c = b - toms748_abs(a) * tol;
  const double fc = TOMS748_EVAL(c, args);
  if (fc == 0) {
    s->a = c; s->fa = 0; s->d = 0; s->fd = 0;
  } else if (s->fa * fc < 0) {
    s->d = b; s->fd = s->fb; s->b = c; s->fb = fc;
  } else {
    s->d = a; s->fd = s->fa; s->a = c; s->fa = fc;
  }
}

/* toms748.py:115-217; *iters: the reference's second return value */
TOMS748_FN double TOMS748_NAME(toms748_solve)(const TOMS748_ARGS *args, double ax, double bx,
                                              double fax, double fbx, double rtol, int max_iter,
                                              int *iters) {
  int count = max_iter;
  const double mu = 0.5;
  toms748_state s;
  s.a = ax; s.b = bx; s.fa = fax; s.fb = fbx; s.d = 0; s.fd = 0;
  if (!(s.a < s.b)) {
    *iters = -1;
    return sdm_nan();
  }
  if (toms748_tol_check(s.a, s.b, rtol) || s.fa == 0 || s.fb == 0) {
    *iters = 0;
    if (s.fa == 0) s.b = s.a;
    else if (s.fb == 0) s.a = s.b;
    return (s.a + s.b) / 2;
  }
  if (!(s.fa * s.fb < 0)) {
    *iters = -1;
    return sdm_nan();
  }
  double e = 1e5, fe = 1e5;
  s.fd = 1e5;
  double c;
  /* (fa != 0 here) */
  c = toms748_secant(s.a, s.b, s.fa, s.fb);
  TOMS748_NAME(toms748_bracket)(args, &s, c);
  count -= 1;
  if (count > 0 && s.fa != 0 && !toms748_tol_check(s.a, s.b, rtol)) {
    c = toms748_quadratic(s.a, s.b, s.d, s.fa, s.fb, s.fd, 2);
    e = s.d;
    fe = s.fd;
    TOMS748_NAME(toms748_bracket)(args, &s, c);
    count -= 1;
  }
  /* (each pass that does not break ends with count -= 1 or with a bracket at least halved: the
     reference's loop; the pass counter only makes the bound a constant of this file) */
  for (int pass = 0; pass < 4096; ++pass) {
    if (!(count > 0 && s.fa != 0 && !toms748_tol_check(s.a, s.b, rtol))) break;
    const double a0 = s.a, b0 = s.b;
    if (toms748_prof(s.fa, s.fb, s.fd, fe))
      c = toms748_quadratic(s.a, s.b, s.d, s.fa, s.fb, s.fd, 2);
    else
      c = toms748_cubic(s.a, s.b, s.d, e, s.fa, s.fb, s.fd, fe);
    e = s.d;
    fe = s.fd;
    TOMS748_NAME(toms748_bracket)(args, &s, c);
    if (count == 1 || s.fa == 0 || toms748_tol_check(s.a, s.b, rtol)) {
      count -= 1;
      break;
    }
    if (toms748_prof(s.fa, s.fb, s.fd, fe))
      c = toms748_quadratic(s.a, s.b, s.d, s.fa, s.fb, s.fd, 3);
    else
      c = toms748_cubic(s.a, s.b, s.d, e, s.fa, s.fb, s.fd, fe);
    TOMS748_NAME(toms748_bracket)(args, &s, c);
    if (count == 1 || s.fa == 0 || toms748_tol_check(s.a, s.b, rtol)) {
      count -= 1;
      break;
    }
    double u, fu;
    if (toms748_abs(s.fa) < toms748_abs(s.fb)) {
      u = s.a; fu = s.fa;
    } else {
      u = s.b; fu = s.fb;
    }
    c = u - 2 * (fu / (s.fb - s.fa)) * (s.b - s.a);
    if (toms748_abs(c - u) > (s.b - s.a) / 2) c = s.a + (s.b - s.a) / 2;
    e = s.d;
    fe = s.fd;
    TOMS748_NAME(toms748_bracket)(args, &s, c);
    if (count == 1 || s.fa == 0 || toms748_tol_check(s.a, s.b, rtol)) {
      count -= 1;
      break;
    }
    if ((s.b - s.a) < mu * (b0 - a0)) continue;
    e = s.d;
    fe = s.fd;
    TOMS748_NAME(toms748_bracket)(args, &s, s.a + (s.b - s.a) / 2);
    count -= 1;
  }
  *iters = max_iter - count;
  if (s.fa == 0) s.b = s.a;
  else if (s.fb == 0) s.a = s.b;
  return (s.a + s.b) / 2;
}

#undef TOMS748_NAME

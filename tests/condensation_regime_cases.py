"""The condensation path restated plainly, formula by formula, with the branch taken as a label.

Every formula of the condensation path - the six saturation vapour pressures, three latent heats,
four diffusion thermics, four kinetics, three ventilations, three growth laws, two
hygroscopicities, four surface tensions, both diffusion coordinates and the state-variable triplet
- and the one-sub-step solver around them (`step_impl`, `calculate_ml_old / _new`, `minfun` of the
reference's condensation_methods.py) is written ONCE below over an "arithmetic namespace" and
evaluated three times: with `mpmath` at 50 digits (`Mp50`), in float64 (`Float64`) and at 50
digits with a running first-order bound of the float64 rounding error next to every value
(`Err`).  It is written from the reference's PySDM/physics/<option>/<choice>.py, not from
csrc/condensation_formulae.h: a second reading.  The constants enter as the float64 values the
host side hands to the library (they are inputs, as the droplets are); whatever the formulae
compute from them (4 / 3 / MAC, 1 / 3 as an exponent, ...) is computed in the namespace.

The observable: `sdm_temperature_pressure_rh[_f]` gives T, p and pv / pvs(T);
`sdm_critical_volume[_f]` gives sigma and r_cr as a volume; `sdm_condensation[_f]` with
adaptive = 0, ONE sub-step, rtol_x = RTOL_X = 1e-14 and max_iters = 64 on cells of one to three
super-droplets gives, per droplet, the root of the implicit Euler equation of `minfun` and, per
cell, the mid-step RH, the vapour and heat budget and the three counters.  Roots are solved at 50
digits inside the very bracket the solver would use (x_old, max(x_insane, x_old + 2^k dx_old)),
and only where `minfun` is strictly monotone on that bracket at 50 digits (a fixed grid of
MONOTONE_GRID points): full kappa-Koehler with kappa < 1 has a pole between x_insane and x_old.

The quirks of the formulation are restated as they are: Python's `max` / `min` keep the first
argument unless the second compares greater / less; `np.maximum` / `np.minimum` propagate NaN;
`np.where(x < XTHRES, ...)` sends NaN to the second branch; sigma is evaluated with the droplet's
`vdry` at the old state and with `PI_4_3 * rd3` inside `minfun`; `Fk` and `Fd` are frozen at the
old radius; `minfun` returns `x_old - x_new` beyond `x_max`; a droplet within RH_rtol of its
equilibrium keeps x_old, and its mass comes back as mass(x(m)).

Bounds are per row and derived, none is fixed: four times the first-order float64 rounding error
of the formulation (`Err`: half an ulp per arithmetic operation and square root, MAX_ULP ulp for
exp / log / pow as tests/test_sdm_math.py pins them), for a root divided by |f'| at the root and
with the solver's contract rtol * |root| added (TOMS748 ends on |b - a| < rtol * min(|a|, |b|)).
The isotherm search of CompressedFilmRuehl is part of that formulation with rtol = 1e-6 on
f_surf: sigma = sgm_w - (A0 - A_iso / f_surf) m_sigma is then known to
|d sigma / d f_surf| * 1e-6 f_surf = (A_iso / f_surf) m_sigma 1e-6, evaluated per row.

Rows the 50-digit run cannot decide carry `float_only` (the "second list", FLOAT_ONLY_LABELS with
the reason): they are compared with the float64 run of this restatement and HIP == checker only.

`sdm_equilibrate_wet_radii` (D) with the same tight tolerance gives the root of
RH - RH_eq(r) on [r_dry, r_cr], or r_dry where the search returns early.
"""
# pylint: disable=invalid-name,too-many-locals,too-many-arguments,too-many-branches
# pylint: disable=too-many-statements,too-many-return-statements,too-many-lines
import json
import os

import numpy as np

from pysdm_amd.condensation import (CONSTANT_NAMES, COUNTERS, FORMULAE_CONSTANT_NAMES,
                                    condensation_call, descriptor_of)
from pysdm_amd.formulae import Formulae
from pysdm_amd.physics.condensation_formulae import CHOICES
from tests import condensation_formulae_cases as fc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "condensation_regimes.npz")
MEASURED = os.path.join(GOLDEN, "condensation_regimes_measured.json")

U = 2.0 ** -53  # unit roundoff: half an ulp
MAX_ULP = {"exp": 0.7, "log": 0.51, "pow": 0.7}  # (tests/test_sdm_math.py; a test compares them)
FACTOR = 4  # bound = FACTOR * the formulation's own first-order rounding error (+ contracts)
RTOL_X = 1e-14
MAX_ITERS = 64
RH_RTOL = 1e-7
RUEHL_RTOL = 1e-6
RUEHL_BRACKET = (1e-16, 1.0)
MONOTONE_GRID = 17
DV = 1e-6
MIN_ROWS_PER_LABEL = 8
MAX_DROPS = 3
DEFAULTS = {option: choices[0] for option, choices in CHOICES.items()}


# ---- the three arithmetic namespaces ------------------------------------------------------------
class Float64:
    """IEEE double: NumPy scalars, so that 1 / 0, log(0) and overflow give inf / nan and never
    raise; roots by bisection down to neighbouring doubles"""
    name = "float64"
    nan = np.float64("nan")

    @staticmethod
    def num(x):
        return np.float64(x)

    @staticmethod
    def exp(x):
        return np.exp(np.float64(x))

    @staticmethod
    def log(x):
        return np.log(np.float64(x))

    @staticmethod
    def sqrt(x):
        return np.sqrt(np.float64(x))

    @staticmethod
    def pow(x, p):
        return np.power(np.float64(x), np.float64(p))

    @staticmethod
    def tanh(x):
        return np.tanh(np.float64(x))

    @staticmethod
    def slack(x, amount):  # pylint: disable=unused-argument
        return x

    @staticmethod
    def to_float(x):
        return float(x)

    def solve(self, fun, a, b):
        fa, fb = fun(a), fun(b)
        if not fa * fb < 0:
            return self.nan
        for _ in range(4000):
            c = a + (b - a) / 2
            if c <= a or c >= b:
                break
            f = fun(c)
            if f == 0:
                return c
            if fa * f < 0:
                b, fb = c, f
            else:
                a, fa = c, f
        return a + (b - a) / 2


class Mp50:
    """mpmath at 50 digits; the real-valued conventions of IEEE where mpmath would go complex or
    raise; roots by the Illinois method to 40 digits"""
    name = "mp50"

    def __init__(self):
        import mpmath  # pylint: disable=import-outside-toplevel

        self.mp = mpmath.mp.clone()
        self.mp.dps = 50
        self.mpf = self.mp.mpf
        self.nan, self.inf = self.mp.mpf("nan"), self.mp.mpf("inf")

    def num(self, x):
        return x if isinstance(x, self.mpf) else self.mpf(float(x))

    def exp(self, x):
        return self.mp.exp(self.num(x))

    def log(self, x):
        x = self.num(x)
        if x != x or x < 0:
            return self.nan
        return -self.inf if x == 0 else self.mp.log(x)

    def sqrt(self, x):
        x = self.num(x)
        return self.nan if (x != x or x < 0) else self.mp.sqrt(x)

    def pow(self, x, p):
        x, p = self.num(x), self.num(p)
        if x != x or p != p:
            return self.nan
        if p == 0:
            return self.num(1)
        if p == int(p):
            if x == 0 and p < 0:
                return self.inf
            return x ** int(p)
        if x < 0:
            return self.nan
        if x == 0:
            return self.inf if p < 0 else self.num(0)
        return self.mp.power(x, p)

    def tanh(self, x):
        return self.mp.tanh(self.num(x))

    @staticmethod
    def slack(x, amount):  # pylint: disable=unused-argument
        return x

    @staticmethod
    def to_float(x):
        return float(x)  # rounds to nearest, once

    def solve(self, fun, a, b, tol=1e-40):
        a, b = self.num(a), self.num(b)
        fa, fb = fun(a), fun(b)
        if not fa * fb < 0:
            return self.nan
        side, last = 0, None
        for _ in range(2000):
            c = (fa * b - fb * a) / (fa - fb)
            if last is not None and abs(c - last) <= tol * abs(c):
                return c
            last = c
            f = fun(c)
            if f == 0:
                return c
            if f * fb > 0:
                b, fb = c, f
                if side == -1:
                    fa /= 2
                side = -1
            else:
                a, fa = c, f
                if side == 1:
                    fb /= 2
                side = 1
        return self.nan


class ErrNum:
    """a 50-digit value `v` and a first-order bound `e` of the absolute error its float64
    evaluation has accumulated; comparisons look at the value"""
    __slots__ = ("v", "e", "ns")

    def __init__(self, ns, v, e):
        self.ns, self.v, self.e = ns, v, e

    def _of(self, other):
        if isinstance(other, ErrNum):
            return other
        return ErrNum(self.ns, self.ns.mp50.num(other), self.ns.zero)

    def _rounded(self, v, e):
        return ErrNum(self.ns, v, e + U * abs(v))

    def __add__(self, other):
        o = self._of(other)
        return self._rounded(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, other):
        o = self._of(other)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, other):
        return self._of(other) - self

    def __mul__(self, other):
        o = self._of(other)
        return self._rounded(self.v * o.v, abs(self.v) * o.e + abs(o.v) * self.e)

    __rmul__ = __mul__

    def __truediv__(self, other):
        o = self._of(other)
        v = self.v / o.v
        return self._rounded(v, self.e / abs(o.v) + abs(v) * o.e / abs(o.v))

    def __rtruediv__(self, other):
        return self._of(other) / self

    def __neg__(self):
        return ErrNum(self.ns, -self.v, self.e)

    def __abs__(self):
        return ErrNum(self.ns, abs(self.v), self.e)

    def __float__(self):
        return float(self.v)

    def __lt__(self, other):
        return self.v < self._of(other).v

    def __le__(self, other):
        return self.v <= self._of(other).v

    def __gt__(self, other):
        return self.v > self._of(other).v

    def __ge__(self, other):
        return self.v >= self._of(other).v

    def __eq__(self, other):
        return self.v == self._of(other).v

    def __ne__(self, other):
        return self.v != self._of(other).v

    __hash__ = None


class Err:
    """values at 50 digits with the first-order bound of their float64 rounding error: U per
    arithmetic operation and square root (correctly rounded), MAX_ULP ulp for exp / log / pow, the
    exact square for pow(x, 2) and the correctly rounded root for pow(x, 0.5) (csrc/sdm_math.h);
    inputs and constants are exact.  tanh is (1 - e) / (1 + e) with e = exp(-2 |y|): three
    roundings of numbers below one after the exponential's."""
    name = "err"

    def __init__(self, mp50):
        self.mp50, self.mp = mp50, mp50.mp
        self.zero = mp50.num(0)
        self.nan = ErrNum(self, mp50.nan, self.zero)

    def num(self, x):
        return x if isinstance(x, ErrNum) else ErrNum(self, self.mp50.num(x), self.zero)

    def exp(self, x):
        x = self.num(x)
        v = self.mp50.exp(x.v)
        return ErrNum(self, v, abs(v) * x.e + MAX_ULP["exp"] * 2 * U * abs(v))

    def log(self, x):
        x = self.num(x)
        v = self.mp50.log(x.v)
        return ErrNum(self, v, x.e / abs(x.v) + MAX_ULP["log"] * 2 * U * abs(v))

    def sqrt(self, x):
        x = self.num(x)
        v = self.mp50.sqrt(x.v)
        return ErrNum(self, v, (x.e / (2 * v) if v != 0 else self.zero) + U * abs(v))

    def pow(self, x, p):
        x, p = self.num(x), self.num(p)
        v = self.mp50.pow(x.v, p.v)
        if p.v == 0 and p.e == 0:
            return ErrNum(self, v, self.zero)
        if x.v == 0:
            return ErrNum(self, v, self.zero)
        carried = abs(v) * (abs(p.v) * x.e / abs(x.v) + abs(self.mp50.log(abs(x.v))) * p.e)
        own = U if (p.e == 0 and p.v in (2, 0.5)) else MAX_ULP["pow"] * 2 * U
        return ErrNum(self, v, carried + own * abs(v))

    def tanh(self, x):
        x = self.num(x)
        v = self.mp50.tanh(x.v)
        return ErrNum(self, v, (1 - v * v) * x.e + (2 * MAX_ULP["exp"] + 3) * U)

    def slack(self, x, amount):
        """adds a contract (not a rounding error) to the bound: FACTOR * e comes out as
        FACTOR * rounding + amount"""
        x, amount = self.num(x), self.num(amount)
        return ErrNum(self, x.v, x.e + abs(amount.v) / FACTOR)

    @staticmethod
    def to_float(x):
        return float(x.v)

    def solve(self, fun, a, b):
        """the 50-digit root; its bound is the function's own at the root over |f'|"""
        a, b = self.num(a), self.num(b)
        root = self.mp50.solve(lambda x: fun(ErrNum(self, x, self.zero)).v, a.v, b.v)
        if root != root:
            return self.nan
        h = abs(root) * self.mp.mpf("1e-20")
        slope = (fun(ErrNum(self, root + h, self.zero)).v
                 - fun(ErrNum(self, root - h, self.zero)).v) / (2 * h)
        # (the bracket ends carry their own rounding error as well: a root cannot leave them,
        # so they add nothing)
        return ErrNum(self, root, fun(ErrNum(self, root, self.zero)).e / abs(slope))


def pymax(a, b):
    """Python's max(a, b)"""
    return b if b > a else a


def pymin(a, b):
    """Python's min(a, b)"""
    return b if b < a else a


def npmax(a, b):
    """np.maximum: NaN if either is"""
    if a != a:
        return a
    if b != b:
        return b
    return a if a >= b else b


def npmin(a, b):
    """np.minimum: NaN if either is"""
    if a != a:
        return a
    if b != b:
        return b
    return a if a <= b else b


# ---- constants -----------------------------------------------------------------------------------
EXTRA_CONSTANT_NAMES = ("c_pd",)


def formulae_of(options, constants=None):
    """the Formulae carrying the constants of a set (choices `Formulae` refuses travel in the
    descriptor)"""
    served = {option: choice for option, choice in options.items() if not fc.host_refused(
        {option: choice})}
    return Formulae(constants={**fc.CONSTANTS, **(constants or {})}, **served)


def constants_in(A, formulae):
    names = (*CONSTANT_NAMES, *FORMULAE_CONSTANT_NAMES, *EXTRA_CONSTANT_NAMES)
    return {name: A.num(float(getattr(formulae.constants, name))) for name in names}


# ---- state_variable_triplet/libcloudphplusplus.py, trivia.py, liquid_spheres.py ------------------
def svt_T(A, k, rhod, thd):
    return thd * A.pow(rhod * thd / k["p1000"] * k["Rd"],
                       k["Rd_over_c_pd"] / (1 - k["Rd_over_c_pd"]))


def svt_p(k, rhod, T, qv):
    return rhod * (1 + qv) * (k["Rv"] / (1 / qv + 1) + k["Rd"] / (1 + qv)) * T


def svt_pv(k, p, qv):
    return p * qv / (qv + k["eps"])


def svt_dthd_dt(k, rhod, thd, T, dqv_dt, lv):
    return -lv * dqv_dt / k["c_pd"] / T * thd * rhod


def radius(A, k, volume):
    return A.pow(volume / k["PI_4_3"], k["ONE_THIRD"])


def volume(A, k, r):
    return k["PI_4_3"] * A.pow(r, k["THREE"])


def within_tolerance(error_estimate, value, rtol):
    return error_estimate < rtol * abs(value)


def dm_dt(k, r, r_dr_dt):
    return 4 * k["PI"] * k["rho_w"] * r * r_dr_dt


# ---- diffusion_coordinate ------------------------------------------------------------------------
def x_of(A, o, mass):
    return mass if o["diffusion_coordinate"] == "WaterMass" else A.log(mass)


def mass_of(A, o, x):
    return x if o["diffusion_coordinate"] == "WaterMass" else A.exp(x)


def dx_dt(o, m, dm):
    return dm if o["diffusion_coordinate"] == "WaterMass" else dm / m


def x_max(A, o):
    return A.num(1) if o["diffusion_coordinate"] == "WaterMass" else A.num(0)


# ---- saturation_vapour_pressure ------------------------------------------------------------------
def _horner(coefficients, d):
    value = coefficients[-1]
    for c in coefficients[-2::-1]:
        value = c + d * value
    return value


def pvs_water(A, k, choice, T, labels):
    if choice in ("AugustRocheMagnus", "Bolton1980"):
        c = ([k[f"ARM_C{i}"] for i in (1, 2, 3)] if choice == "AugustRocheMagnus"
             else [k[f"B80W_G{i}"] for i in range(3)])
        return c[0] * A.exp((c[1] * (T - k["T0"])) / ((T - k["T0"]) + c[2]))
    if choice == "Lowe1977":
        # A0 + d * (A1 + d * (... + d * (A5 + d * (A6))))
        return _horner([k[f"L77W_A{i}"] for i in range(7)], T - k["T0"])
    if choice == "MurphyKoop2005":
        c = [None, *(k[f"MK05_LIQ_C{i}"] for i in range(1, 14))]
        labels.append("mk05/below_tanh_centre" if T < c[8] else "mk05/above_tanh_centre")
        return c[1] * A.exp(
            c[2] - c[3] / T - c[4] * A.log(T / c[5]) + c[6] * T
            + A.tanh(c[7] * (T - c[8]))
            * (c[9] - c[10] / T - c[11] * A.log(T / c[12]) + c[13] * T))
    if choice == "Wexler1976":
        g = [k[f"W76W_G{i}"] for i in range(9)]
        return A.exp(g[0] / A.pow(T, 2) + g[1] / T + g[2] + g[3] * T + g[4] * A.pow(T, 2)
                     + g[5] * A.pow(T, 3) + g[6] * A.pow(T, 4)
                     + g[7] * A.log(T / k["one_kelvin"])) * g[8]
    assert choice == "FlatauWalkoCotton", choice
    return _horner([k[f"FWC_C{i}"] for i in range(9)], T - k["T0"])


# ---- latent_heat_vapourisation, diffusion_thermics, diffusion_kinetics ---------------------------
def lv_of(A, k, choice, T):
    if choice == "Constant":
        return k["l_tri"]
    if choice == "Lowe2019":
        return k["l_tri"] * A.pow(k["T_tri"] / T, k["l_l19_a"] + k["l_l19_b"] * T)
    assert choice == "Kirchhoff", choice
    return k["l_tri"] + (k["c_pv"] - k["c_pw"]) * (T - k["T_tri"])


def thermics_D(A, k, choice, T, p):
    if choice == "TracyWelchPorter":
        return k["D0"] * A.pow(T / k["T0"], k["D_exp"]) * (k["p1000"] / p)
    if choice == "LoweEtAl2019":
        return k["d_l19_a"] * (k["p_STP"] / p) * A.pow(T / k["T0"], k["d_l19_b"])
    if choice == "GrabowskiEtAl2011":
        return k["diffusion_thermics_D_G11_A"] * (
            k["diffusion_thermics_D_G11_B"] * T + k["diffusion_thermics_D_G11_C"])
    assert choice == "Neglect", choice
    return k["D0"]


def thermics_K(A, k, choice, T):
    if choice == "LoweEtAl2019":
        return k["k_l19_a"] * (k["k_l19_b"] + k["k_l19_c"] * T)
    if choice == "GrabowskiEtAl2011":
        return (k["diffusion_thermics_K_G11_A"] * A.pow(T, 3)
                + k["diffusion_thermics_K_G11_B"] * A.pow(T, 2)
                + k["diffusion_thermics_K_G11_C"] * T + k["diffusion_thermics_K_G11_D"])
    assert choice in ("Neglect", "TracyWelchPorter"), choice
    return k["K0"]


def lambda_D(A, k, choice, D, T):
    if choice == "Neglect":
        return A.num(-1)
    return D / A.sqrt(2 * k["Rv"] * T)


def lambda_K(A, k, choice, T, p):
    if choice != "FuchsSutugin":
        return A.num(-1)
    return (A.num(4) / 5) * k["K0"] * T / p / A.sqrt(2 * k["Rd"] * T)


def _fuchs_sutugin(A, accommodation, value, r, lmbd):
    return (value * (1 + lmbd / r)
            / (1 + (A.num(4) / 3 / accommodation + A.num(0.377)) * lmbd / r
               + (A.num(4) / 3 / accommodation) * lmbd / r * lmbd / r))


def kinetics_D(A, k, choice, D, r, lmbd):
    if choice == "Neglect":
        return D
    if choice in ("LoweEtAl2019", "GrabowskiEtAl2011"):  # pruppacher_and_klett_2005.py
        return D / ((r / (r + k["dv_pk05"])) + 2 * A.sqrt(k["PI"]) * lmbd / r / k["MAC"])
    assert choice == "FuchsSutugin", choice
    return _fuchs_sutugin(A, k["MAC"], D, r, lmbd)


def kinetics_K(A, k, choice, K, r, lmbd):
    if choice != "FuchsSutugin":
        return K
    return _fuchs_sutugin(A, k["HAC"], K, r, lmbd)


# ---- ventilation ---------------------------------------------------------------------------------
def ventilation(A, k, choice, Re, Sc, labels):
    if choice == "Neglect":  # np.power(anything, 0)
        return A.num(1)
    x = A.pow(Re, k["ONE_HALF"]) * A.pow(Sc, k["ONE_THIRD"])
    if choice == "Froessling1938":
        return k["FROESSLING_1938_A"] + k["FROESSLING_1938_B"] * x
    assert choice == "PruppacherAndRasmussen1979", choice
    thres = k["PRUPPACHER_RASMUSSEN_1979_XTHRES"]
    if Re == 0:
        labels.append("pr79/Re_zero")
    elif abs(x - thres) <= 4 * 2 * U * abs(thres):
        labels.append("pr79/x_at_thres_below" if x < thres else
                      "pr79/x_at_thres" if x == thres else "pr79/x_at_thres_above")
    else:
        labels.append("pr79/x_below_thres" if x < thres else "pr79/x_above_thres")
    if x < thres:  # np.where: NaN takes the second branch
        return (k["PRUPPACHER_RASMUSSEN_1979_CONSTSMALL"]
                + k["PRUPPACHER_RASMUSSEN_1979_COEFFSMALL"]
                * A.pow(x, k["PRUPPACHER_RASMUSSEN_1979_POWSMALL"]))
    return (k["PRUPPACHER_RASMUSSEN_1979_CONSTBIG"]
            + k["PRUPPACHER_RASMUSSEN_1979_COEFFBIG"] * x)


# ---- drop_growth, hygroscopicity -----------------------------------------------------------------
def growth_Fk(A, k, choice, T, K, lv):
    if choice == "Fick":
        return A.num(0)
    if choice == "Howell1949":
        return k["rho_w"] * lv / T / K * (lv / T / k["Rv"])
    assert choice == "Mason1971", choice
    return k["rho_w"] * lv / T / K * (lv / T / k["Rv"] - 1)


def growth_Fd(k, T, D, pvs):
    return k["rho_w"] * k["Rv"] * T / D / pvs


def growth_r_dr_dt(choice, RH_eq, RH, Fk, Fd):
    if choice == "Fick":
        return (RH - RH_eq) / Fd
    return (RH - RH_eq) / (Fk + Fd)


def hygro_RH_eq(A, k, choice, r, T, kp, rd3, sgm):
    if choice == "KappaKoehler":
        return (A.exp((2 * sgm / k["Rv"] / T / k["rho_w"]) / r) * (A.pow(r, 3) - rd3)
                / (A.pow(r, 3) - rd3 * (1 - kp)))
    assert choice == "KappaKoehlerLeadingTerms", choice
    return 1 + (2 * sgm / k["Rv"] / T / k["rho_w"]) / r - kp * rd3 / A.pow(r, k["THREE"])


def hygro_r_cr(A, k, kp, rd3, T, sgm):
    return A.sqrt(3 * kp * rd3 / (2 * sgm / k["Rv"] / T / k["rho_w"]))


# ---- surface_tension -----------------------------------------------------------------------------
NEAR = 1e-3  # a selector closer than this (relative) to its threshold is labelled "near_..."


def _near(a, b):
    return abs(a - b) <= NEAR * abs(b)


def sigma_of(A, k, choice, T, v_wet, v_dry, f_org, labels):
    if choice == "Constant":
        return k["sgm_w"]
    if choice == "CompressedFilmOvadnevaite":
        r_wet = A.pow((3 * v_wet) / (4 * k["PI"]), A.num(1) / 3)
        v_delta = v_wet - ((4 * k["PI"]) / 3 * A.pow(r_wet - k["delta_min"], 3))
        v_beta = f_org * v_dry
        ratio = v_beta / v_delta
        labels.append("ovadnevaite/f_org_zero" if f_org == 0 else
                      "near_ovadnevaite_clamp" if _near(ratio, 1) else
                      "ovadnevaite/c_beta_below_one" if ratio < 1 else
                      "ovadnevaite/c_beta_clamped")
        c_beta = npmin(ratio, A.num(1))
        return (1 - c_beta) * k["sgm_w"] + c_beta * k["sgm_org"]
    r_wet = A.pow((3 * v_wet) / (4 * k["PI"]), A.num(1) / 3)
    if choice == "SzyszkowskiLangmuir":
        if f_org == 0:
            labels.append("szyszkowski/f_org_zero")
            sgm = k["sgm_w"]
        else:
            Cb_iso = (f_org * v_dry / k["RUEHL_nu_org"]) / (v_wet / k["water_molar_volume"])
            A_iso = (4 * k["PI"] * A.pow(r_wet, 2)) / (
                f_org * v_dry * k["N_A"] / k["RUEHL_nu_org"])
            a = -k["RUEHL_A0"] / A_iso
            b = (k["RUEHL_A0"] / A_iso + (k["RUEHL_A0"] / A_iso) * (k["RUEHL_C0"] / Cb_iso) + 1)
            c = -1
            f_surf = (-b + A.sqrt(A.pow(b, 2) - 4 * a * c)) / (2 * a)
            sgm = k["sgm_w"] - ((k["R_str"] * T) / (k["RUEHL_A0"] * k["N_A"])) * A.log(
                1 + Cb_iso * (1 - f_surf) / k["RUEHL_C0"])
            labels.append("near_szyszkowski_clamp" if _near(sgm, k["RUEHL_sgm_min"]) else
                          "szyszkowski/clamped_to_sgm_min" if sgm < k["RUEHL_sgm_min"] else
                          "szyszkowski/unclamped")
        return pymin(pymax(sgm, k["RUEHL_sgm_min"]), k["sgm_w"])
    assert choice == "CompressedFilmRuehl", choice
    if f_org == 0:
        labels.append("ruehl/f_org_zero")
        sgm = k["sgm_w"]
    elif f_org == 1:
        labels.append("ruehl/f_org_one")
        sgm = k["RUEHL_sgm_min"]
    else:
        Cb_iso = (f_org * v_dry / k["RUEHL_nu_org"]) / (v_wet / k["water_molar_volume"])
        A_iso = (4 * k["PI"] * A.pow(r_wet, 2)) / (f_org * v_dry * k["N_A"] / k["RUEHL_nu_org"])
        c = (k["RUEHL_m_sigma"] * k["N_A"]) / (2 * k["R_str"] * T)

        def minfun(f_surf):
            lhs = Cb_iso * (1 - f_surf) / k["RUEHL_C0"]
            rhs = A.exp(c * (A.pow(k["RUEHL_A0"], 2) - A.pow(A_iso / f_surf, 2)))
            return lhs - rhs

        f_surf = A.solve(minfun, A.num(RUEHL_BRACKET[0]), A.num(RUEHL_BRACKET[1]))
        sgm = k["sgm_w"] - (k["RUEHL_A0"] - A_iso / f_surf) * k["RUEHL_m_sigma"]
        contract = (A_iso / f_surf) * k["RUEHL_m_sigma"] * RUEHL_RTOL
        sgm = A.slack(sgm, contract)
        far = 100 * abs(contract)
        labels.append(
            "ruehl/no_root" if f_surf != f_surf else
            "near_ruehl_clamp" if (abs(sgm - k["RUEHL_sgm_min"]) < far
                                   or abs(sgm - k["sgm_w"]) < far) else
            "ruehl/searched_clamped_low" if sgm < k["RUEHL_sgm_min"] else
            "ruehl/searched_clamped_high" if sgm > k["sgm_w"] else "ruehl/searched_unclamped")
    return npmin(npmax(sgm, k["RUEHL_sgm_min"]), k["sgm_w"])


def ruehl_sigma_contract(T, v_wet, v_dry, f_org, constants=None):
    """per row, in float64: (sigma, what the isotherm search's rtol = 1e-6 on f_surf leaves open in
    it): (A_iso / f_surf) m_sigma 1e-6 where CompressedFilmRuehl searches, 0 where it does not or
    where the unclamped value is further than twice that from the clamp that swallows it (min and
    max never widen a difference)"""
    A = Float64()
    k = constants_in(A, formulae_of({"surface_tension": "CompressedFilmRuehl"}, constants))
    sigma, contract = [], []
    with np.errstate(all="ignore"):
        for row in zip(*(np.asarray(a, dtype=float) for a in np.broadcast_arrays(
                T, v_wet, v_dry, f_org))):
            Ti, vw, vd, fo = (A.num(x) for x in row)
            sigma.append(float(sigma_of(A, k, "CompressedFilmRuehl", Ti, vw, vd, fo, [])))
            contract.append(0.0)
            if fo in (0, 1):
                continue
            r_wet = A.pow((3 * vw) / (4 * k["PI"]), A.num(1) / 3)
            Cb_iso = (fo * vd / k["RUEHL_nu_org"]) / (vw / k["water_molar_volume"])
            A_iso = (4 * k["PI"] * A.pow(r_wet, 2)) / (fo * vd * k["N_A"] / k["RUEHL_nu_org"])
            c = (k["RUEHL_m_sigma"] * k["N_A"]) / (2 * k["R_str"] * Ti)
            f_surf = A.solve(lambda f: Cb_iso * (1 - f) / k["RUEHL_C0"] - A.exp(  # pylint: disable=cell-var-from-loop
                c * (A.pow(k["RUEHL_A0"], 2) - A.pow(A_iso / f, 2))),  # pylint: disable=cell-var-from-loop
                             A.num(RUEHL_BRACKET[0]), A.num(RUEHL_BRACKET[1]))
            if f_surf != f_surf:
                continue
            sgm = k["sgm_w"] - (k["RUEHL_A0"] - A_iso / f_surf) * k["RUEHL_m_sigma"]
            slack = (A_iso / f_surf) * k["RUEHL_m_sigma"] * RUEHL_RTOL
            if (k["RUEHL_sgm_min"] - 2 * slack) < sgm < (k["sgm_w"] + 2 * slack):
                contract[-1] = float(slack)
    return np.array(sigma), np.array(contract)


def ruehl_v_cr_rtol(T, v_wet, v_dry, f_org, constants=None):
    """the relative bound that contract puts on v_cr = PI_4_3 r_cr^3 ~ sigma^-3/2, per row"""
    sigma, contract = ruehl_sigma_contract(T, v_wet, v_dry, f_org, constants)
    with np.errstate(all="ignore"):
        return np.where(contract > 0, 1.5 * contract / sigma, 0.0)


# ---- A: temperature_pressure_rh ------------------------------------------------------------------
def eval_tprh(A, k, o, row, labels):
    rhod, thd, qv = (A.num(row[key]) for key in ("rhod", "thd", "qv"))
    T = svt_T(A, k, rhod, thd)
    p = svt_p(k, rhod, T, qv)
    choice = o["saturation_vapour_pressure"]
    RH = svt_pv(k, p, qv) / pvs_water(A, k, choice, T, labels)
    labels.append(f"pvs/{choice}/" + ("T_below_253K" if T < 253 else
                                      "T_253_to_293K" if T < 293 else "T_above_293K"))
    return {"T": T, "p": p, "RH": RH}


# ---- B: critical_volume --------------------------------------------------------------------------
def eval_vcr(A, k, o, row, labels):
    kappa, f_org, v_dry, v_wet, T = (A.num(row[key]) for key in
                                     ("kappa", "f_org", "v_dry", "v_wet", "T"))
    sgm = sigma_of(A, k, o["surface_tension"], T, v_wet, v_dry, f_org, labels)
    labels.append(f"r_cr/{o['surface_tension']}/{o['hygroscopicity']}")
    r_cr = hygro_r_cr(A, k, kappa, v_dry / k["PI_4_3"], T, sgm)
    return {"v_cr": volume(A, k, r_cr)}


# ---- D: equilibrate_wet_radii --------------------------------------------------------------------
def eval_wet(A, k, o, row, labels, monotone=None):
    """r_wet_init_impl of the reference's initialisation/equilibrate_wet_radii.py for one particle;
    None where its search has no bracket"""
    r_dry, ktdv, f_org, T, RH = (A.num(row[key]) for key in
                                 ("r_dry", "kappa_times_dry_volume", "f_org", "T", "RH"))
    kappa = ktdv / volume(A, k, r_dry)
    rd3 = A.pow(r_dry, 3)
    a = r_dry
    b = hygro_r_cr(A, k, kappa, rd3, T, k["sgm_w"])
    if not a < b:
        labels.append("wet/a_not_below_b")
        return {"r_wet": r_dry}
    if RH < 0:
        labels.append("wet/RH_clamped_at_zero")
    elif RH > 1:
        labels.append("wet/RH_clamped_at_one")
    RH = npmax(A.num(0), npmin(A.num(1), RH))

    def minfun(r, where=None):
        sgm = sigma_of(A, k, o["surface_tension"], T, volume(A, k, r), k["PI_4_3"] * rd3, f_org,
                       [] if where is None else where)
        return RH - hygro_RH_eq(A, k, o["hygroscopicity"], r, T, kappa, rd3, sgm)

    fa = minfun(a)
    if fa < 0:
        labels.append("wet/fa_negative")
        return {"r_wet": r_dry}
    fb = minfun(b)
    if fa == 0:  # TOMS748 returns an end of the bracket on which the function vanishes
        labels.append("wet/fa_zero")
        return {"r_wet": a}
    if not fa * fb < 0:
        labels.append("wet/no_bracket")
        return None
    if monotone is not None:
        monotone.append(is_monotone(A, minfun, a, b))
    root = A.solve(minfun, a, b)
    if root != root:
        labels.append("wet/no_root")
        return None
    minfun(root, labels)
    labels.append(f"wet/solved/{o['surface_tension']}/{o['hygroscopicity']}")
    return {"r_wet": A.slack(root, RTOL_X * abs(root))}


# ---- C: one fixed sub-step of step_impl ----------------------------------------------------------
def minfun_of(A, k, o, x_old, timestep, kappa, f_org, rd3, T, RH, Fk, Fd):
    """cm.py minfun; sigma sees PI_4_3 * rd3 as the dry volume"""
    def minfun(x_new):
        if x_new > x_max(A, o):
            return x_old - x_new
        mass_new = mass_of(A, o, x_new)
        volume_new = mass_new / k["rho_w"]
        r_new = radius(A, k, volume_new)
        RH_eq = hygro_RH_eq(A, k, o["hygroscopicity"], r_new, T, kappa, rd3, sigma_of(
            A, k, o["surface_tension"], T, volume_new, k["PI_4_3"] * rd3, f_org, []))
        r_dr_dt = growth_r_dr_dt(o["drop_growth"], RH_eq, RH, Fk, Fd)
        return x_old - x_new + timestep * dx_dt(o, mass_new, dm_dt(k, r_new, r_dr_dt))
    return minfun


def ldexp(A, x, n):
    return x * A.num(2.0 ** n)


def new_mass(A, k, o, w, drop, labels, monotone=None):
    """the per-droplet body of calculate_ml_new for a droplet with water mass > 0; `w` holds the
    sub-step's cell scalars.  Returns the new mass, or None where the reference gives up."""
    m, vdry, kappa, f_org, Re = (A.num(drop[key]) for key in
                                 ("water_mass", "vdry", "kappa", "f_org", "reynolds_number"))
    T, RH = w["T"], w["RH"]
    v_drop = m / k["rho_w"]
    x_old = x_of(A, o, m)
    r_old = radius(A, k, v_drop)
    x_insane = x_of(A, o, k["rho_w"] * (vdry / 100))
    rd3 = vdry / k["PI_4_3"]
    sgm = sigma_of(A, k, o["surface_tension"], T, v_drop, vdry, f_org, labels)
    RH_eq = hygro_RH_eq(A, k, o["hygroscopicity"], r_old, T, kappa, rd3, sgm)
    if not within_tolerance(abs(RH - RH_eq), RH, w["RH_rtol"]):
        Dr = kinetics_D(A, k, o["diffusion_kinetics"], w["DTp"], r_old, w["lambdaD"])
        Kr = kinetics_K(A, k, o["diffusion_kinetics"], w["KTp"], r_old, w["lambdaK"])
        vent = ventilation(A, k, o["ventilation"], Re, w["Sc"], labels)
        Fk = growth_Fk(A, k, o["drop_growth"], T, Kr * vent, w["lv"])
        Fd = growth_Fd(k, T, Dr * vent, w["pvs"])
        minfun = minfun_of(A, k, o, x_old, w["timestep"], kappa, f_org, rd3, T, RH, Fk, Fd)
        r_dr_dt_old = growth_r_dr_dt(o["drop_growth"], RH_eq, RH, Fk, Fd)
        mass_old = mass_of(A, o, x_old)
        dx_old = w["timestep"] * dx_dt(o, mass_old, dm_dt(k, r_old, r_dr_dt_old))
    else:
        dx_old = A.num(0)
    if dx_old == 0:
        labels.append("solver/dx_old_zero")
        x_new = x_old
    else:
        labels.append("solver/growth" if dx_old > 0 else "solver/evaporation")
        a = x_old
        b = pymax(x_insane, a + dx_old)
        fa, fb = minfun(a), minfun(b)
        counter = 0
        while not fa * fb < 0:
            counter += 1
            if counter > w["max_iters"]:
                labels.append("solver/no_bracket")
                return None
            b = pymax(x_insane, a + ldexp(A, dx_old, counter))
            fb = minfun(b)
        labels.append("solver/bracket_at_once" if counter == 0 else "solver/bracket_doubled")
        if counter > 0:
            labels.append(f"solver/doublings_{counter}")
        if b == x_insane:
            labels.append("solver/x_insane_clamp")
        if b > x_max(A, o):
            labels.append("solver/beyond_x_max")
        if a != b:
            if a > b:
                a, b = b, a
            if monotone is not None:
                monotone.append(is_monotone(A, minfun, a, b))
            x_new = A.solve(minfun, a, b)
            if x_new != x_new:
                labels.append("solver/no_root")
                return None
            x_new = A.slack(x_new, w["rtol_x"] * abs(x_new))
        else:
            labels.append("solver/a_equals_b")
            x_new = x_old
    return mass_of(A, o, x_new)


def is_monotone(A, fun, a, b):
    """strictly monotone on the fixed grid of MONOTONE_GRID points of [a, b]"""
    values = [fun(a + (b - a) * A.num(i) / (MONOTONE_GRID - 1)) for i in range(MONOTONE_GRID)]
    steps = [values[i + 1] - values[i] for i in range(MONOTONE_GRID - 1)]
    return all(s > 0 for s in steps) or all(s < 0 for s in steps)


def eval_cond(A, k, o, row, labels, monotone=None):
    """step_impl with n_substeps = 1 and fake = False on one cell"""
    n_drops = int(row["n_drops"])
    drops = [{key: row[key][i] for key in DROP_COLUMNS} for i in range(n_drops)]
    timestep = A.num(row["timestep"])
    rhod, thd, qv, prhod, pthd, pqv = (A.num(row[key]) for key in (
        "rhod", "thd", "qv", "prhod", "pthd", "pqv"))
    dthd_dt_pred = (pthd - thd) / timestep
    dqv_dt_pred = (pqv - qv) / timestep
    drhod_dt = (prhod - rhod) / timestep
    m_d = (prhod + rhod) / 2 * A.num(row["dv"])
    # calculate_ml_old
    ml_old = A.num(0)
    for drop in drops:
        if drop["water_mass"] > 0:
            ml_old = ml_old + A.num(drop["multiplicity"]) * A.num(drop["water_mass"])
    thd = thd + timestep * dthd_dt_pred / 2
    qv = qv + timestep * dqv_dt_pred / 2
    rhod = rhod + timestep * drhod_dt / 2
    T = svt_T(A, k, rhod, thd)
    p = svt_p(k, rhod, T, qv)
    pv = svt_pv(k, p, qv)
    lv = lv_of(A, k, o["latent_heat_vapourisation"], T)
    pvs = pvs_water(A, k, o["saturation_vapour_pressure"], T, labels)
    DTp = thermics_D(A, k, o["diffusion_thermics"], T, p)
    KTp = thermics_K(A, k, o["diffusion_thermics"], T)
    RH = pv / pvs
    Sc = A.num(row["air_dynamic_viscosity"]) / DTp / A.num(row["air_density"])
    w = {"T": T, "RH": RH, "Sc": Sc, "lv": lv, "pvs": pvs, "DTp": DTp, "KTp": KTp,
         "timestep": timestep, "rtol_x": RTOL_X, "RH_rtol": RH_RTOL, "max_iters": MAX_ITERS,
         "lambdaK": lambda_K(A, k, o["diffusion_kinetics"], T, p),
         "lambdaD": lambda_D(A, k, o["diffusion_kinetics"], DTp, T)}
    # calculate_ml_new
    ml_new = A.num(0)
    n_activating = n_deactivating = n_growing = 0
    masses = [A.num(drop["water_mass"]) for drop in drops]
    for i, drop in enumerate(drops):
        if drop["water_mass"] <= 0:
            labels.append("solver/mass_not_positive")
            continue
        if drop["multiplicity"] == 0:
            labels.append("solver/multiplicity_zero")
        mass_new = new_mass(A, k, o, w, drop, labels, monotone)
        if mass_new is None:
            return None
        mass_cr = k["rho_w"] * A.num(drop["v_cr"])
        n = int(drop["multiplicity"])
        ml_new = ml_new + A.num(n) * mass_new
        old = A.num(drop["water_mass"])
        if mass_new > mass_cr and mass_new > old:
            n_growing += n
        if mass_new > mass_cr > old:
            n_activating += n
        if mass_new < mass_cr < old:
            n_deactivating += n
        masses[i] = mass_new
    n_ripening = n_growing if n_deactivating > 0 else 0
    if n_activating > 0:
        labels.append("counters/activating")
    if n_deactivating > 0:
        labels.append("counters/deactivating")
        labels.append("counters/ripening" if n_ripening > 0 else "counters/deactivating_alone")
    elif n_growing > 0 and n_drops > 1:
        labels.append("counters/ripening_suppressed")
    dml_dt = (ml_new - ml_old) / timestep
    dqv_dt_corr = -dml_dt / m_d
    dthd_dt_corr = svt_dthd_dt(k, rhod, thd, T, dqv_dt_corr, lv)
    thd_new = thd + timestep * (dthd_dt_pred / 2 + dthd_dt_corr)
    qv_new = qv + timestep * (dqv_dt_pred / 2 + dqv_dt_corr)
    out = {"pthd": thd_new, "pqv": qv_new, "RH_max": pymax(A.num(0), RH)}
    for i in range(MAX_DROPS):
        out[f"mass{i}"] = masses[i] if i < n_drops else A.num(0)
    out["n_activating"], out["n_deactivating"], out["n_ripening"] = (
        n_activating, n_deactivating, n_ripening)
    # what a relative error of 1e-9 in lv / in the n * m sum would move (the budget is observed
    # where that exceeds the row's bound)
    out["budget_thd"] = abs(timestep * dthd_dt_corr) * 1e-9
    out["budget_qv"] = abs(ml_new / m_d) * 1e-9
    return out


DROP_COLUMNS = ("water_mass", "multiplicity", "vdry", "kappa", "f_org", "reynolds_number", "v_cr")
CELL_COLUMNS = ("rhod", "thd", "qv", "prhod", "pthd", "pqv", "air_density",
                "air_dynamic_viscosity", "dv", "timestep", "n_drops")
GROUPS = {  # group: (evaluator, input columns, float outputs, integer outputs)
    "tprh": (eval_tprh, ("rhod", "thd", "qv"), ("T", "p", "RH"), ()),
    "vcr": (eval_vcr, ("kappa", "f_org", "v_dry", "v_wet", "T"), ("v_cr",), ()),
    "wet": (eval_wet, ("r_dry", "kappa_times_dry_volume", "f_org", "T", "RH"), ("r_wet",), ()),
    "cond": (eval_cond, (*CELL_COLUMNS, *DROP_COLUMNS),
             ("mass0", "mass1", "mass2", "pthd", "pqv", "RH_max"),
             ("n_activating", "n_deactivating", "n_ripening")),
}

# ---- the formulae sets ---------------------------------------------------------------------------
# "default" runs through sdm_condensation, "default/general" the same rows through the general
# kernel; MAC != HAC (both 1 by default) tells the two accommodation coefficients apart
SETS = {"default": {"options": {}},
        "default/general": {"options": {}, "general": True},
        "default/MAC_HAC": {"options": {}, "constants": {"MAC": 0.3, "HAC": 0.7}},
        "general/MAC_HAC": {"options": {}, "constants": {"MAC": 0.3, "HAC": 0.7},
                            "general": True},
        **{name: {"options": dict(cfg["options"])} for name, cfg in fc.SETS.items()}}
SETS["LoweEtAl2019/MAC"] = {"options": {"diffusion_kinetics": "LoweEtAl2019"},
                            "constants": {"MAC": 0.3}}

COND_SETS = tuple(SETS)
# the pointwise sets of B: every surface tension with either hygroscopicity
VCR_SETS = {}
for _sgm in CHOICES["surface_tension"]:
    for _hygro in CHOICES["hygroscopicity"]:
        _key = f"vcr/{_sgm}/{_hygro}"
        SETS[_key] = {"options": {"surface_tension": _sgm, "hygroscopicity": _hygro},
                      "pointwise": True}
        VCR_SETS[f"{_sgm}|{_hygro}"] = _key


def options_of(name):
    return {**DEFAULTS, **SETS[name]["options"]}


def set_formulae(name):
    return formulae_of(SETS[name]["options"], SETS[name].get("constants"))


def set_descriptor(name):
    """None: the formulae's own (PySDM's defaults: the default descriptor)"""
    options = SETS[name]["options"]
    if not fc.host_refused(options):
        return None
    return descriptor_of(options, set_formulae(name).constants)


# ---- labels --------------------------------------------------------------------------------------
def _set_labels():
    return tuple(f"set/{name}" for name in COND_SETS)


LABELS = tuple(
    [f"pvs/{choice}/{band}" for choice in CHOICES["saturation_vapour_pressure"]
     for band in ("T_below_253K", "T_253_to_293K", "T_above_293K")]
    + ["mk05/below_tanh_centre", "mk05/above_tanh_centre"]
    + [f"r_cr/{sgm}/{hygro}" for sgm in CHOICES["surface_tension"]
       for hygro in CHOICES["hygroscopicity"]]
    + ["ovadnevaite/f_org_zero", "ovadnevaite/c_beta_below_one", "ovadnevaite/c_beta_clamped",
       "szyszkowski/f_org_zero", "szyszkowski/unclamped", "szyszkowski/clamped_to_sgm_min",
       "ruehl/f_org_zero", "ruehl/f_org_one", "ruehl/searched_unclamped",
       "ruehl/searched_clamped_low", "ruehl/searched_clamped_high",
       "pr79/Re_zero", "pr79/x_below_thres", "pr79/x_above_thres",
       "pr79/x_at_thres", "pr79/x_at_thres_below",
       "solver/dx_old_zero", "solver/growth", "solver/evaporation", "solver/x_insane_clamp",
       "solver/bracket_at_once", "solver/bracket_doubled", "solver/mass_not_positive",
       "solver/multiplicity_zero",
       "counters/activating", "counters/deactivating", "counters/ripening",
       "counters/ripening_suppressed"]
    + ["wet/a_not_below_b", "wet/fa_negative", "wet/RH_clamped_at_zero", "wet/RH_clamped_at_one"]
    + [f"wet/solved/{sgm}/{hygro}" for sgm in CHOICES["surface_tension"]
       for hygro in CHOICES["hygroscopicity"]]
    + [f"budget/{choice}" for choice in CHOICES["latent_heat_vapourisation"]]
    + list(_set_labels()))
# the second list: labels that the 50-digit run cannot decide, with the reason
FLOAT_ONLY_LABELS = {
    "pr79/x_at_thres": "x = sqrt(Re) cbrt(Sc) is itself rounded: whether it EQUALS the threshold "
                       "is a property of the rounding (searched over Re with the float64 run)",
    "pr79/x_at_thres_below": "the same: x is the threshold's lower float64 neighbour",
}


class Evaluator:
    """evaluates rows of a group in one namespace, caching the constants per set"""

    def __init__(self, A):
        self.A, self._k = A, {}

    def constants(self, name):
        if name not in self._k:
            self._k[name] = constants_in(self.A, set_formulae(name))
        return self._k[name]

    def __call__(self, group, row, monotone=None):  # (monotone: for "cond" and "wet")
        """({output: value in the namespace} or None, labels)"""
        name = str(row["set"])
        labels = [f"set/{name}"] if group == "cond" else []
        args = (self.A, self.constants(name), options_of(name), row, labels)
        with np.errstate(all="ignore"):
            out = (GROUPS[group][0](*args, monotone) if group in ("cond", "wet")
                   else GROUPS[group][0](*args))
        return out, labels


def label_string(labels):
    return ";".join(sorted(set(labels)))


# ---- planting ------------------------------------------------------------------------------------
K0 = set_formulae("default").constants  # float64 constants for building inputs


def _ambient(rng, T, p, RH):
    """(rhod, thd, qv) of a state close to (T, p, RH by the default pvs)"""
    d = T - K0.T0
    pvs = np.polyval([getattr(K0, f"FWC_C{i}") for i in range(8, -1, -1)], d)
    pv = RH * pvs
    qv = K0.eps * pv / (p - pv)
    rhod = (p - pv) / K0.Rd / T
    thd = T * (K0.p1000 / (p - pv)) ** K0.Rd_over_c_pd
    return float(rhod), float(thd * (1 + rng.uniform(-1e-4, 1e-4))), float(qv)


def plant_tprh():
    rng = np.random.default_rng(20261019)
    rows = []
    for choice in CHOICES["saturation_vapour_pressure"]:
        temps = list(np.linspace(233.5, 312.5, 30))
        if choice == "MurphyKoop2005":  # either side of the tanh centre, 218.8 K
            centre = float(K0.MK05_LIQ_C8)
            temps += [centre + d for d in (-12, -6, -3, -1, -0.3, -0.1, -0.03, -0.01, -1e-3,
                                           1e-3, 0.01, 0.03, 0.1, 0.3, 1, 3, 6, 12)]
        for T in temps:
            rhod, thd, qv = _ambient(rng, T + rng.uniform(-0.4, 0.4),
                                     rng.uniform(3e4, 1.02e5), rng.uniform(0.3, 1.05))
            rows.append({"set": choice, "rhod": rhod, "thd": thd, "qv": qv})
    return rows


for _choice in CHOICES["saturation_vapour_pressure"][1:]:
    assert _choice in SETS  # (the single sets are named after their choice)
SETS_OF_PVS = {choice: ("default" if i == 0 else choice)
               for i, choice in enumerate(CHOICES["saturation_vapour_pressure"])}


def plant_vcr():
    rng = np.random.default_rng(20261020)
    rows = []
    for sgm in CHOICES["surface_tension"]:
        for hygro in CHOICES["hygroscopicity"]:
            for i in range(60 if sgm != "Constant" else 10):
                r_dry = np.exp(rng.uniform(np.log(0.01e-6), np.log(0.5e-6)))
                ratio = np.exp(rng.uniform(np.log(1.02), np.log(40)))
                f_org = float(rng.uniform(0, 1)) if i % 6 else float(i % 12 == 0)
                if i % 6 == 1:
                    f_org = float(np.exp(rng.uniform(np.log(1e-4), 0)))
                rows.append({"set": f"{sgm}|{hygro}", "kappa": float(rng.uniform(0.05, 1.3)),
                             "f_org": f_org, "v_dry": float(K0.PI_4_3 * r_dry ** 3),
                             "v_wet": float(K0.PI_4_3 * (r_dry * ratio) ** 3),
                             "T": float(rng.uniform(240, 310))})
    return rows


def _droplet(rng, *, r_dry=None, ratio=None, kappa=None, f_org=0.0, Re=0.0, n=None):
    r_dry = np.exp(rng.uniform(np.log(0.02e-6), np.log(0.3e-6))) if r_dry is None else r_dry
    ratio = rng.uniform(1.5, 20) if ratio is None else ratio
    kappa = rng.uniform(0.2, 1.3) if kappa is None else kappa
    n = int(rng.integers(100, 5000)) if n is None else n
    return {"water_mass": float(K0.rho_w * K0.PI_4_3 * (r_dry * ratio) ** 3),
            "multiplicity": n, "vdry": float(K0.PI_4_3 * r_dry ** 3), "kappa": float(kappa),
            "f_org": float(f_org), "reynolds_number": float(Re), "v_cr": 0.0}


def _cell(rng, name, drops, *, T=None, RH=None, timestep=1.0):
    T = rng.uniform(265, 303) if T is None else T
    RH = rng.uniform(0.96, 1.012) if RH is None else RH
    p = rng.uniform(5e4, 1.01e5)
    rhod, thd, qv = _ambient(rng, T, p, RH)
    eta = (K0.ZOGRAFOS_1987_COEFF_T3 * T ** 3 + K0.ZOGRAFOS_1987_COEFF_T2 * T ** 2
           + K0.ZOGRAFOS_1987_COEFF_T1 * T + K0.ZOGRAFOS_1987_COEFF_T0)
    row = {"set": name, "rhod": rhod, "thd": thd, "qv": qv,
           "prhod": rhod * (1 + rng.uniform(-2e-4, 0)), "pthd": thd + rng.uniform(-0.05, 0.05),
           "pqv": qv * (1 + rng.uniform(-5e-4, 5e-4)), "air_density": rhod * (1 + qv),
           "air_dynamic_viscosity": float(eta), "dv": DV, "timestep": float(timestep),
           "n_drops": len(drops)}
    for key in DROP_COLUMNS:
        values = [d[key] for d in drops] + [0] * (MAX_DROPS - len(drops))
        row[key] = np.array(values, dtype=np.int64 if key == "multiplicity" else float)
    return row


def _needs(name):
    o = SETS[name]["options"]
    return (o.get("surface_tension", "Constant") != "Constant",
            o.get("ventilation", "Neglect") != "Neglect",
            o.get("hygroscopicity") == "KappaKoehler")


def _f_org(rng, i):
    return (0.0, 1.0, float(rng.uniform(0.02, 0.98)), float(np.exp(rng.uniform(-7, 0))))[i % 4]


def _float_run():
    if not _FLOAT_RUN:
        _FLOAT_RUN.append(Evaluator(Float64()))
    return _FLOAT_RUN[0]


_FLOAT_RUN = []


def _with_critical_volume(row, out):
    """v_cr is an input like any other: the default formulae's critical volume, or - every third
    droplet - the geometric mean of the old and the new volume, which makes a growing droplet
    activate and a shrinking one deactivate, far from either comparison's edge"""
    v_cr = row["v_cr"].copy()
    for i in range(int(row["n_drops"])):
        if row["water_mass"][i] <= 0:
            continue
        new = float(out[f"mass{i}"])
        if row["_cross"][i] and new > 0 and new != row["water_mass"][i]:
            v_cr[i] = np.sqrt(row["water_mass"][i] * new) / K0.rho_w
        else:
            T = 285.0
            rd3 = row["vdry"][i] / K0.PI_4_3
            v_cr[i] = K0.PI_4_3 * np.sqrt(3 * row["kappa"][i] * rd3 / (
                2 * K0.sgm_w / K0.Rv / T / K0.rho_w)) ** 3
    # (six digits: the planted input does not hang on the last bits of the float64 run)
    row["v_cr"] = np.array([float(f"{value:.5e}") for value in v_cr])


def _pr79_threshold_rows(rng, name):
    """Reynolds numbers for which the float64 x equals XTHRES or its lower neighbour"""
    rows = []
    run = _float_run()
    thres = np.float64(K0.PRUPPACHER_RASMUSSEN_1979_XTHRES)
    for want in (thres, np.nextafter(thres, 0)) * 12:
        row = _cell(rng, name, [_droplet(rng, ratio=rng.uniform(30, 200), Re=1.0)])
        k = run.constants(name)
        # Sc of this cell, as eval_cond has it
        A = run.A
        T = svt_T(A, k, *(A.num(v) for v in _mid_state(row)[:2]))
        rhod, thd, qv = _mid_state(row)
        p = svt_p(k, A.num(rhod), T, A.num(qv))
        D = thermics_D(A, k, options_of(name)["diffusion_thermics"], T, p)
        Sc = A.num(row["air_dynamic_viscosity"]) / D / A.num(row["air_density"])
        cbrt = A.pow(Sc, k["ONE_THIRD"])
        Re = np.float64((thres / cbrt) ** 2)
        for _ in range(400):
            x = A.pow(Re, k["ONE_HALF"]) * cbrt
            if x == want:
                break
            Re = np.nextafter(Re, np.inf if x < want else 0)
        else:
            continue
        row["reynolds_number"][0] = Re
        rows.append(row)
    return rows


def _mid_state(row):
    """rhod, thd, qv at the middle of the step, in float64 as eval_cond forms them"""
    dt = np.float64(row["timestep"])
    return tuple(np.float64(row[a]) + dt * ((np.float64(row[b]) - np.float64(row[a])) / dt) / 2
                 for a, b in (("rhod", "prhod"), ("thd", "pthd"), ("qv", "pqv")))


def _equilibrium_rows(rng, name, mp50, count):
    """droplets planted at the 50-digit equilibrium of the mid-step state: dx_old == 0"""
    rows = []
    evaluator = Evaluator(mp50)
    for _ in range(count * 3):
        if len(rows) == count:
            break
        RH = rng.uniform(0.93, 0.995)
        row = _cell(rng, name, [_droplet(rng)], RH=RH)
        k, o, A = evaluator.constants(name), options_of(name), mp50
        rhod, thd, qv = (A.num(row[a]) + (A.num(row[b]) - A.num(row[a])) / 2
                         for a, b in (("rhod", "prhod"), ("thd", "pthd"), ("qv", "pqv")))
        T = svt_T(A, k, rhod, thd)
        RH_mid = svt_pv(k, svt_p(k, rhod, T, qv), qv) / pvs_water(
            A, k, o["saturation_vapour_pressure"], T, [])
        vdry, kappa = A.num(row["vdry"][0]), A.num(row["kappa"][0])
        rd3 = vdry / k["PI_4_3"]
        r_dry = radius(A, k, vdry)
        r_cr = hygro_r_cr(A, k, kappa, rd3, T, k["sgm_w"])
        root = A.solve(lambda r: RH_mid - hygro_RH_eq(A, k, o["hygroscopicity"], r, T, kappa,
                                                      rd3, k["sgm_w"]),
                       r_dry * A.num(1.05), r_cr)
        if root != root:
            continue
        row["water_mass"][0] = float(k["rho_w"] * volume(A, k, root))
        row["_always"] = True
        rows.append(row)
    return rows


def plant_cond(mp50):
    """candidate cells per set, picked by the labels of the float64 run"""
    rng = np.random.default_rng(20261021)
    run = _float_run()
    picked = []
    counts = {}
    for name in COND_SETS:
        film, ventilated, full_koehler = _needs(name)
        candidates = []
        for i in range(CANDIDATES_PER_SET):
            kwargs = {}
            if film:
                kwargs["f_org"] = _f_org(rng, i)
            if ventilated:
                kwargs["Re"] = (0.0, float(rng.uniform(0.05, 2.0)), float(rng.uniform(5, 300)))[
                    i % 3]
                kwargs["ratio"] = rng.uniform(5, 300)
            if full_koehler:
                kwargs["kappa"] = rng.uniform(1.0, 1.4)
            timestep = (1.0, 1.0, 5.0, 0.2)[i % 4]
            n_drops = (1, 1, 2, 3)[i % 4]
            drops = [_droplet(rng, **kwargs) for _ in range(n_drops)]
            if name.startswith("default") and i % 5 == 4:  # small droplets in dry air: the clamp
                drops = [_droplet(rng, ratio=rng.uniform(1.2, 3)) for _ in range(n_drops)]
                candidates.append(_cell(rng, name, drops, RH=rng.uniform(0.5, 0.9),
                                        timestep=20.0))
                continue
            if n_drops > 1 and i % 8 == 2:
                drops[0]["water_mass"] = (0.0, -drops[0]["water_mass"])[i % 16 == 2]
            if n_drops > 1 and i % 8 == 3:
                drops[1]["multiplicity"] = 0
            if n_drops > 1 and i % 8 in (6, 7):
                # a large solution droplet grows while a small dilute one evaporates
                drops[0] = _droplet(rng, r_dry=0.25e-6, ratio=3, kappa=1.2,
                                    **{a: b for a, b in kwargs.items() if a in ("f_org", "Re")})
                drops[1] = _droplet(rng, r_dry=0.012e-6, ratio=60, kappa=0.3,
                                    **{a: b for a, b in kwargs.items() if a in ("f_org", "Re")})
                candidates.append(_cell(rng, name, drops, RH=rng.uniform(0.9990, 0.9999),
                                        timestep=timestep))
                candidates[-1]["_cross"] = np.ones(MAX_DROPS, dtype=bool)
                continue
            candidates.append(_cell(rng, name, drops, timestep=timestep))
        if name == "PruppacherAndRasmussen1979":
            candidates += _pr79_threshold_rows(rng, name)
        if name in ("default", "default/general", "KappaKoehler", "WaterMass"):
            candidates += _equilibrium_rows(rng, name, mp50, 10)
        for at, row in enumerate(candidates):
            row.setdefault("_cross", np.array([(at + i) % 3 == 0 for i in range(MAX_DROPS)]))
            monotone = []
            out, labels = run("cond", row, monotone)
            if not all(monotone):
                continue
            if out is None or any(lab.startswith("near_") or lab in (
                    "solver/no_root", "solver/no_bracket", "ruehl/no_root", "solver/a_equals_b")
                                  for lab in labels):
                continue
            _with_critical_volume(row, out)
            out, labels = run("cond", row)
            labels = set(labels)
            if not row.pop("_always", False) and not any(
                    counts.get(lab, 0) < PER_LABEL for lab in labels
                    if lab in LABELS or lab.startswith("solver/doublings")):
                continue
            for lab in labels:
                counts[lab] = counts.get(lab, 0) + 1
            del row["_cross"]
            picked.append(row)
    return picked


PER_LABEL = 10
CANDIDATES_PER_SET = 160


def plant(mp50):
    """{group: rows}"""
    return {"tprh": [dict(row, set=SETS_OF_PVS[row["set"]]) for row in plant_tprh()],
            "vcr": _pick_vcr(plant_vcr()), "wet": _pick_vcr(plant_wet(), "wet"),
            "cond": plant_cond(mp50)}


def plant_wet():
    rng = np.random.default_rng(20261022)
    rows = []
    for key in VCR_SETS:
        for i in range(120):
            r_dry = np.exp(rng.uniform(np.log(0.01e-6), np.log(0.5e-6)))
            kappa = rng.uniform(0.05, 1.3)
            RH = rng.uniform(0.3, 0.999)
            kind = i % 12
            if kind == 0:  # the critical radius is not above the dry one
                r_dry, kappa = np.exp(rng.uniform(np.log(1e-10), np.log(2e-9))), rng.uniform(
                    0.01, 0.1)
            elif kind == 1:  # dry air and little solute: already too wet at the dry radius
                kappa, RH = rng.uniform(0.02, 0.3), rng.uniform(0.05, 0.6)
            elif kind == 2:
                RH = rng.uniform(-0.5, -0.01)
                kappa = rng.uniform(1.05, 1.3)
            elif kind == 3:
                RH = rng.uniform(1.0001, 1.05)
            f_org = (0.0, 1.0, float(rng.uniform(0.02, 0.98)))[i % 3]
            rows.append({"set": key, "r_dry": float(r_dry),
                         "kappa_times_dry_volume": float(kappa * K0.PI_4_3 * r_dry ** 3),
                         "f_org": f_org, "T": float(rng.uniform(250, 305)), "RH": float(RH)})
    return rows


def _pick_vcr(rows, group="vcr"):
    run = _float_run()
    picked, counts = [], {}
    for row in rows:
        row = dict(row, set=VCR_SETS[row["set"]])
        monotone = []
        out, labels = run(group, row, monotone)
        if out is None or not all(monotone) or any(
                lab.startswith("near_") or lab == "ruehl/no_root" for lab in labels):
            continue
        if not all(np.isfinite(float(value)) for value in out.values()):
            continue
        key = tuple(sorted(labels))
        if counts.get(key, 0) >= PER_LABEL:
            continue
        counts[key] = counts.get(key, 0) + 1
        picked.append(row)
    return picked


# ---- the fixture ---------------------------------------------------------------------------------
def columns_of(group, rows):
    names = ("set", *GROUPS[group][1])
    return {key: np.array([row[key] for row in rows]) for key in names}


def generate(report=print):
    """the fixture's arrays and the float64 run's worst error over bound per label group"""
    mp50 = Mp50()
    runs = {"float64": _float_run(), "mp50": Evaluator(mp50), "err": Evaluator(Err(mp50))}
    out, ratios = {}, {}
    for group, rows in plant(mp50).items():
        floats, ints = GROUPS[group][2], GROUPS[group][3]
        kept, dropped = [], {}
        for row in rows:
            plain, labels = runs["float64"](group, row)
            monotone = []
            precise, labels_mp = runs["mp50"](group, row, monotone)
            second = any(lab in FLOAT_ONLY_LABELS for lab in labels)
            why = None
            if not second:
                why = ("gives up at 50 digits" if precise is None else
                       "the precisions take different branches" if set(labels) != set(labels_mp)
                       else "minfun is not monotone on the bracket" if not all(monotone) else
                       "the counters differ" if any(plain[key] != precise[key] for key in ints)
                       else None)
            bounded = None if why else runs["err"](group, row)[0]
            if why is None and bounded is None:
                why = "no bound"
            if why:
                dropped[why] = dropped.get(why, 0) + 1
                continue
            record = {"row": row, "labels": list(labels), "float_only": second}
            for key in floats:
                value = bounded[key]
                record[f"expected/{key}"] = (float(plain[key]) if second
                                             else float(precise[key]))
                record[f"float64/{key}"] = float(plain[key])
                record[f"bound/{key}"] = (float(FACTOR * value.e / abs(value.v))
                                          if value.v != 0 else 0.0)
                record[f"exact/{key}"] = float(precise[key]) if precise is not None else np.nan
            for key in ints:
                record[f"expected/{key}"] = int(plain[key] if second else precise[key])
            if group == "cond":
                lv = options_of(str(row["set"]))["latent_heat_vapourisation"]
                seen_thd = float(bounded["budget_thd"].v) > record["bound/pthd"] * abs(
                    record["expected/pthd"])
                seen_qv = float(bounded["budget_qv"].v) > record["bound/pqv"] * abs(
                    record["expected/pqv"])
                if seen_thd and seen_qv and not second:
                    record["labels"].append(f"budget/{lv}")
            kept.append(record)
        report(f"{group}: {len(kept)} rows of {len(rows)} candidates "
               f"({sum(r['float_only'] for r in kept)} on the second list; not planted: {dropped})")
        for key, values in columns_of(group, [r["row"] for r in kept]).items():
            out[f"{group}/in/{key}"] = values
        out[f"{group}/labels"] = np.array([label_string(r["labels"]) for r in kept])
        out[f"{group}/float_only"] = np.array([r["float_only"] for r in kept])
        for key in floats:
            for kind in ("expected", "float64", "bound"):
                out[f"{group}/{kind}/{key}"] = np.array([r[f"{kind}/{key}"] for r in kept])
        for key in ints:
            out[f"{group}/expected/{key}"] = np.array([r[f"expected/{key}"] for r in kept],
                                                      dtype=np.int64)
        # the error model against the float64 run of the restatement itself
        for r in kept:
            if r["float_only"]:
                continue
            for key in floats:
                ratio = _ratio(r[f"float64/{key}"], r[f"exact/{key}"], r[f"bound/{key}"])
                for tag in _ratio_groups(group, key, r["labels"]):
                    ratios[tag] = max(ratios.get(tag, 0.0), ratio)
    return out, ratios


def _ratio(got, want, bound):
    """error over bound (0 / 0: 0)"""
    if got == want:
        return 0.0
    if bound == 0 or want == 0:
        return float("inf")
    return abs(got - want) / abs(want) / bound


def _ratio_groups(group, key, labels):
    """the label groups a row's ratio is reported under"""
    quantity = "mass" if key.startswith("mass") else key
    if group != "cond":
        return [f"{group}/{quantity}/{lab}" for lab in labels
                if lab.startswith(("pvs/", "r_cr/", "wet/"))]
    return [f"{group}/{quantity}/{lab[4:]}" for lab in labels if lab.startswith("set/")]


# ---- reading the fixture and running the library -------------------------------------------------
class Fixture:
    def __init__(self, path=FIXTURE):
        data = np.load(path)
        self.data = {key: data[key] for key in data.files}
        self.groups = tuple(GROUPS)

    def inputs(self, group):
        prefix = f"{group}/in/"
        return {key[len(prefix):]: value for key, value in self.data.items()
                if key.startswith(prefix)}

    def labels(self, group):
        return self.data[f"{group}/labels"]

    def float_only(self, group):
        return self.data[f"{group}/float_only"]

    def outputs(self, group, kind):
        prefix = f"{group}/{kind}/"
        return {key[len(prefix):]: value for key, value in self.data.items()
                if key.startswith(prefix)}


_FIXTURE = []


def fixture():
    if not _FIXTURE:
        _FIXTURE.append(Fixture())
    return _FIXTURE[0]


def _consts(formulae):
    return [float(getattr(formulae.constants, name)) for name in CONSTANT_NAMES]


def _descriptor(name):
    descriptor = set_descriptor(name)
    if descriptor is None:
        from pysdm_amd.condensation import check_formulae  # pylint: disable=import-outside-toplevel
        descriptor = check_formulae(set_formulae(name))
    return descriptor


def _is_default(name):
    return not SETS[name]["options"] and not SETS[name].get("general")


def run_tprh(engine, columns, general=False):
    """`sdm_temperature_pressure_rh` for the default saturation vapour pressure (`general`: its
    `_f` form with the default descriptor), `_f` for the others"""
    up, down = engine.upload, engine.download
    n_all = len(columns["set"])
    out = {key: np.full(n_all, np.nan) for key in ("T", "p", "RH")}
    for name in sorted(set(columns["set"].tolist())):
        sel = np.flatnonzero(columns["set"] == name)
        args = [up(np.ascontiguousarray(columns[key][sel])) for key in ("rhod", "thd", "qv")]
        res = [up(np.zeros(len(sel))) for _ in range(3)]
        consts = _consts(set_formulae(name))
        if _is_default(name) and not general:
            engine.call_condensation("sdm_temperature_pressure_rh", *args, *res, len(sel), consts)
        else:
            engine.call_condensation_formulae("sdm_temperature_pressure_rh_f", *args, *res,
                                              len(sel), consts, _descriptor(name))
        for key, value in zip(("T", "p", "RH"), res):
            out[key][sel] = down(value)
    return out


def run_vcr(engine, columns, general=False):
    up, down = engine.upload, engine.download
    n_all = len(columns["set"])
    out = {"v_cr": np.full(n_all, np.nan)}
    for name in sorted(set(columns["set"].tolist())):
        sel = np.flatnonzero(columns["set"] == name)
        n = len(sel)
        col = {key: up(np.ascontiguousarray(columns[key][sel]))
               for key in ("kappa", "f_org", "v_dry", "v_wet", "T")}
        v_cr, cell = up(np.zeros(n)), up(np.arange(n, dtype=np.int64))
        args = (v_cr, col["kappa"], col["f_org"], col["v_dry"], col["v_wet"], col["T"], cell, n,
                _consts(set_formulae(name)))
        descriptor = _descriptor(name)
        if not any(descriptor.option) and not general:
            engine.call_condensation("sdm_critical_volume", *args)
        else:
            engine.call_condensation_formulae("sdm_critical_volume_f", *args, descriptor)
        out["v_cr"][sel] = down(v_cr)
    return out


def run_wet(engine, columns):
    """`sdm_equilibrate_wet_radii` with the tight tolerance, every particle in a cell of its own"""
    from pysdm_amd import initialisation as init  # pylint: disable=import-outside-toplevel

    n_all = len(columns["set"])
    out = {"r_wet": np.full(n_all, np.nan)}
    for name in sorted(set(columns["set"].tolist())):
        sel = np.flatnonzero(columns["set"] == name)
        pick = lambda key: np.ascontiguousarray(columns[key][sel])  # noqa: E731  pylint: disable=cell-var-from-loop
        r_wet, _, status = init.wet_radii_call(
            engine, set_formulae(name), r_dry=pick("r_dry"),
            kappa_times_dry_volume=pick("kappa_times_dry_volume"), T=pick("T"), RH=pick("RH"),
            f_org=pick("f_org"), cell_id=np.arange(len(sel), dtype=np.int64), rtol=RTOL_X,
            max_iters=MAX_ITERS, descriptor=_descriptor(name))
        words = engine.download(status)
        for word in (init.STATUS_FAILED, init.STATUS_MAX_ITERS, init.STATUS_SIGMA_FAILED):
            assert words[word] == 0, (name, words)
        out["r_wet"][sel] = engine.download(r_wet)
    return out


def run_cond(engine, columns):
    """one library call per (set, timestep): adaptive = 0, one sub-step, cells of 1 - 3 droplets
    in a shuffled order of cells, with a reversed permutation inside each cell's slice"""
    up, down = engine.upload, engine.download
    n_all = len(columns["set"])
    out = {key: np.full(n_all, np.nan) for key in GROUPS["cond"][2]}
    out.update({key: np.full(n_all, -7, dtype=np.int64) for key in GROUPS["cond"][3]})
    out["success"] = np.zeros(n_all, dtype=np.int64)
    calls = sorted(set(zip(columns["set"].tolist(), columns["timestep"].tolist())))
    for name, timestep in calls:
        sel = np.flatnonzero((columns["set"] == name) & (columns["timestep"] == timestep))
        n_cell = len(sel)
        counts = columns["n_drops"][sel].astype(np.int64)
        cell_start = np.zeros(n_cell + 1, dtype=np.int64)
        cell_start[1:] = np.cumsum(counts)
        n_sd = int(cell_start[-1])
        where = [(c, i) for c in range(n_cell) for i in range(int(counts[c]))]
        drop = {key: np.array([columns[key][sel[c]][i] for c, i in where],
                              dtype=np.int64 if key == "multiplicity" else float)
                for key in DROP_COLUMNS}
        cell = {key: np.ascontiguousarray(columns[key][sel], dtype=float) for key in CELL_COLUMNS}
        formulae = set_formulae(name)
        arrays = {key: up(value) for key, value in (
            ("cell_start", cell_start), ("water_mass", drop["water_mass"]),
            ("v_cr", drop["v_cr"]), ("multiplicity", drop["multiplicity"]),
            ("vdry", drop["vdry"]), ("idx", np.arange(n_sd, dtype=np.int64)),
            ("rhod", cell["rhod"]), ("thd", cell["thd"]),
            ("water_vapour_mixing_ratio", cell["qv"]), ("prhod", cell["prhod"]),
            ("pthd", cell["pthd"]), ("predicted_water_vapour_mixing_ratio", cell["pqv"]),
            ("kappa", drop["kappa"]), ("f_org", drop["f_org"]),
            ("reynolds_number", drop["reynolds_number"]), ("air_density", cell["air_density"]),
            ("air_dynamic_viscosity", cell["air_dynamic_viscosity"]),
            ("cell_order", np.arange(n_cell, dtype=np.int64)[::-1].copy()))}
        counters = {key: up(np.full(n_cell, 1 if key == "n_substeps" else -1, dtype=np.int64))
                    for key in COUNTERS}
        RH_max, success = up(np.full(n_cell, np.nan)), up(np.zeros(n_cell, dtype=np.uint8))
        condensation_call(
            engine, formulae=formulae, n_sd=n_sd, n_cell=n_cell, dv=float(cell["dv"][0]),
            rtol_x=RTOL_X, rtol_thd=1e-9, timestep=float(timestep), dt_range=(1e-4, timestep),
            fuse=32, multiplier=2, RH_rtol=RH_RTOL, max_iters=MAX_ITERS, adaptive=False,
            counters=counters, RH_max=RH_max, success=success,
            general=bool(SETS[name].get("general")), descriptor=set_descriptor(name), **arrays)
        assert (cell["dv"] == cell["dv"][0]).all()
        mass = down(arrays["water_mass"])
        for at, (c, i) in enumerate(where):
            out[f"mass{i}"][sel[c]] = mass[at]
        for c in range(n_cell):
            for i in range(int(counts[c]), MAX_DROPS):
                out[f"mass{i}"][sel[c]] = 0.0
        out["pthd"][sel] = down(arrays["pthd"])
        out["pqv"][sel] = down(arrays["predicted_water_vapour_mixing_ratio"])
        out["RH_max"][sel] = down(RH_max)
        out["success"][sel] = down(success)
        for key in GROUPS["cond"][3]:
            out[key][sel] = down(counters[key])
        assert (down(counters["n_substeps"]) == 1).all()
    return out


def checker_engine(group):
    """the CPU checker engine that serves a group's symbols: the wet radii have one of their own"""
    if group == "wet":
        from tests.initialisation_checker import InitialisationCheckerEngine  # pylint: disable=import-outside-toplevel

        return InitialisationCheckerEngine.get()
    from tests.condensation_formulae_checker import CheckerEngine  # pylint: disable=import-outside-toplevel

    return CheckerEngine.get()


RUNNERS = {"tprh": run_tprh, "vcr": run_vcr, "wet": run_wet, "cond": run_cond}


def run_group(engine, group, fix=None, **kwargs):
    fix = fix or fixture()
    return RUNNERS[group](engine, fix.inputs(group), **kwargs)


# ---- the checks ----------------------------------------------------------------------------------
def count_labels(fix=None, compared_only=True):
    fix = fix or fixture()
    counts = {}
    for group in fix.groups:
        for labels, second in zip(fix.labels(group), fix.float_only(group)):
            for lab in str(labels).split(";"):
                if compared_only and second and lab not in FLOAT_ONLY_LABELS:
                    continue
                counts[lab] = counts.get(lab, 0) + 1
    return counts


def check_coverage(fix=None):
    """every label on at least MIN_ROWS_PER_LABEL rows compared at 50 digits (the labels of the
    second list: on that many float-only rows), and the float-only rows are exactly the declared
    ones"""
    fix = fix or fixture()
    counts = count_labels(fix)
    short = {lab: counts.get(lab, 0) for lab in LABELS if counts.get(lab, 0) < MIN_ROWS_PER_LABEL}
    assert not short, short
    assert any(lab.startswith("solver/doublings_") for lab in counts)
    for group in fix.groups:
        for labels, second in zip(fix.labels(group), fix.float_only(group)):
            declared = any(lab in FLOAT_ONLY_LABELS for lab in str(labels).split(";"))
            assert bool(second) == declared, (group, labels)
    cells = fix.inputs("cond")["n_drops"]
    assert set(cells.tolist()) == {1, 2, 3}


def errors_over_bounds(group, got, fix=None):
    """{output: error over bound per row} against the fixture's expected values"""
    fix = fix or fixture()
    expected, bounds = fix.outputs(group, "expected"), fix.outputs(group, "bound")
    return {key: np.array([_ratio(float(g), float(e), float(b))
                           for g, e, b in zip(got[key], expected[key], bounds[key])])
            for key in GROUPS[group][2]}


def check_group(engine, group, fix=None, report=None, **kwargs):
    """the library against the fixture: integers exactly, floats within the per-row bounds"""
    fix = fix or fixture()
    got = run_group(engine, group, fix, **kwargs)
    expected = fix.outputs(group, "expected")
    labels = fix.labels(group)
    if group == "cond":
        assert (got["success"] == 1).all(), labels[got["success"] != 1][:5]
    for key in GROUPS[group][3]:
        bad = np.flatnonzero(got[key] != expected[key])
        assert bad.size == 0, (key, [(int(i), str(labels[i]), int(got[key][i]),
                                      int(expected[key][i])) for i in bad[:5]])
    ratios = errors_over_bounds(group, got, fix)
    worst = {}
    for key, ratio in ratios.items():
        for i, value in enumerate(ratio):
            for tag in _ratio_groups(group, key, str(labels[i]).split(";")):
                worst[tag] = max(worst.get(tag, 0.0), float(value))
        bad = np.flatnonzero(~(ratio <= 1))
        assert bad.size == 0, (group, key, [
            (int(i), str(labels[i]), float(got[key][i]), float(expected[key][i]),
             float(ratio[i])) for i in bad[:5]])
    if report is not None:
        report.update(worst)
    return worst


def check_equilibrium_rows(engine, fix=None):
    """a droplet planted at its equilibrium keeps x_old: its mass comes back as mass(x(m)), which
    the row's bound holds to the mass it had"""
    fix = fix or fixture()
    got = run_group(engine, "cond", fix)
    columns, bounds = fix.inputs("cond"), fix.outputs("cond", "bound")
    rows = [i for i, labels in enumerate(fix.labels("cond"))
            if "solver/dx_old_zero" in str(labels).split(";") and columns["n_drops"][i] == 1]
    assert len(rows) >= MIN_ROWS_PER_LABEL
    for i in rows:
        before = columns["water_mass"][i][0]
        assert abs(got["mass0"][i] - before) <= bounds["mass0"][i] * before, i
        if options_of(str(columns["set"][i]))["diffusion_coordinate"] == "WaterMass":
            assert got["mass0"][i] == before


def check_same_bits(engine, other, group, fix=None, **kwargs):
    a = run_group(engine, group, fix, **kwargs)
    b = run_group(other, group, fix, **kwargs)
    for key, value in a.items():
        np.testing.assert_array_equal(np.asarray(value).view(np.uint8),
                                      np.asarray(b[key]).view(np.uint8), err_msg=f"{group} {key}")


def measured():
    with open(MEASURED, encoding="utf-8") as file:
        return json.load(file)

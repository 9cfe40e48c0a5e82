"""Host-side (NumPy) forms of the condensation formulae that code outside the kernels evaluates:
`saturation_vapour_pressure.pvs_water`, `surface_tension.sigma` and `hygroscopicity.r_cr` of every
choice `pysdm_amd.formulae.Formulae` accepts (set-up code uses them to initialise wet radii and
critical volumes).  The kernels have their own forms (csrc/condensation_formulae.h); these follow
the same published formulae, cited per class, with the constants bound at construction and array
arguments throughout.  `CHOICES` lists every option of the condensation path with its choices,
PySDM's default first.
"""
import numpy as np

CHOICES = {
    "diffusion_coordinate": ("WaterMassLogarithm", "WaterMass"),
    "saturation_vapour_pressure": ("FlatauWalkoCotton", "AugustRocheMagnus", "Bolton1980",
                                   "Lowe1977", "MurphyKoop2005", "Wexler1976"),
    "latent_heat_vapourisation": ("Kirchhoff", "Constant", "Lowe2019"),
    "hygroscopicity": ("KappaKoehlerLeadingTerms", "KappaKoehler"),
    "drop_growth": ("Mason1971", "Howell1949", "Fick"),
    "surface_tension": ("Constant", "CompressedFilmOvadnevaite", "SzyszkowskiLangmuir",
                        "CompressedFilmRuehl"),
    "diffusion_kinetics": ("FuchsSutugin", "Neglect", "LoweEtAl2019", "GrabowskiEtAl2011"),
    "diffusion_thermics": ("Neglect", "TracyWelchPorter", "LoweEtAl2019", "GrabowskiEtAl2011"),
    "ventilation": ("Neglect", "Froessling1938", "PruppacherAndRasmussen1979"),
}
# Choices the library serves (include/sdm_condensation_formulae.h, reachable with an explicit
# descriptor: pysdm_amd.condensation.descriptor_of) but `Formulae` and `check_formulae` go on
# refusing: their refusal is what the tests of the default path and of the deposition path pin
# (tests/test_condensation_checker.py, tests/test_deposition_checker.py).  `WaterMass` is refused
# by condensation only: `Formulae` accepts it for the deposition path.
HOST_REFUSED = {
    "drop_growth": ("Fick",),
    "ventilation": ("Froessling1938",),
    "diffusion_kinetics": ("Neglect",),
    "diffusion_coordinate": ("WaterMass",),
}
# the options with a single choice in PySDM, which stay as they are
FIXED = {"state_variable_triplet": "LibcloudphPlusPlus",
         "air_dynamic_viscosity": "ZografosEtAl1987"}
_RUEHL = ("RUEHL_nu_org", "RUEHL_A0", "RUEHL_C0", "RUEHL_sgm_min")
# constants a choice needs to be finite (what the reference's classes assert when constructed)
FINITE = {
    ("surface_tension", "CompressedFilmOvadnevaite"): ("sgm_org", "delta_min"),
    ("surface_tension", "SzyszkowskiLangmuir"): _RUEHL,
    ("surface_tension", "CompressedFilmRuehl"): (*_RUEHL, "RUEHL_m_sigma"),
}
# constants a choice needs to be zero
ZERO = {("diffusion_kinetics", "LoweEtAl2019"): ("dv_pk05",)}


class _Option:  # pylint: disable=too-few-public-methods
    """a chosen option: `__name__` is the choice (as PySDM's namespaces have it)"""

    def __init__(self, name, constants):
        self.__name__ = name
        self.const = constants


class SaturationVapourPressure(_Option):
    """pvs_water(T) in Pa: Flatau, Walko & Cotton 1992 (eighth-order fit), the August-Roche-
    Magnus formula, Bolton 1980 eq. 10, Lowe 1977 (sixth-order fit), Murphy & Koop 2005 eq. 10,
    Wexler 1976"""

    def pvs_water(self, T):  # pylint: disable=too-many-return-statements
        k, name = self.const, self.__name__
        T = np.asarray(T, dtype=float)
        d = T - k.T0
        if name == "AugustRocheMagnus":
            return k.ARM_C1 * np.exp(k.ARM_C2 * d / (d + k.ARM_C3))
        if name == "Bolton1980":
            return k.B80W_G0 * np.exp(k.B80W_G1 * d / (d + k.B80W_G2))
        if name == "Lowe1977":
            return np.polyval([getattr(k, f"L77W_A{i}") for i in range(6, -1, -1)], d)
        if name == "MurphyKoop2005":
            c = [None, *(getattr(k, f"MK05_LIQ_C{i}") for i in range(1, 14))]
            return c[1] * np.exp(
                c[2] - c[3] / T - c[4] * np.log(T / c[5]) + c[6] * T
                + np.tanh(c[7] * (T - c[8]))
                * (c[9] - c[10] / T - c[11] * np.log(T / c[12]) + c[13] * T))
        if name == "Wexler1976":
            g = [getattr(k, f"W76W_G{i}") for i in range(9)]
            return g[8] * np.exp(g[0] / T ** 2 + g[1] / T + g[2] + g[3] * T + g[4] * T ** 2
                                 + g[5] * T ** 3 + g[6] * T ** 4
                                 + g[7] * np.log(T / k.one_kelvin))
        return np.polyval([getattr(k, f"FWC_C{i}") for i in range(8, -1, -1)], d)


class Hygroscopicity(_Option):
    """Petters & Kreidenweis 2007; the critical radius is the leading-terms one in both choices"""

    def r_cr(self, kp, rd3, T, sgm):
        k = self.const
        return np.sqrt(3 * np.asarray(kp) * rd3 / (2 * np.asarray(sgm) / k.Rv / T / k.rho_w))


def _bisect(function, low, high, steps=200):
    """elementwise root of a function that changes sign on [low, high]"""
    f_low = function(low)
    for _ in range(steps):
        mid = (low + high) / 2
        f_mid = function(mid)
        same = np.sign(f_mid) == np.sign(f_low)
        low, f_low = np.where(same, mid, low), np.where(same, f_mid, f_low)
        high = np.where(same, high, mid)
    return (low + high) / 2


class SurfaceTension(_Option):
    """sigma(T, v_wet, v_dry, f_org) in J / m^2: constant; the compressed film of Ovadnevaite et
    al. 2017 (all organics in a surface layer at least `delta_min` thick); the Szyszkowski-Langmuir
    and compressed-film isotherms of Ruehl et al. 2016 (suppl. eq. 12-15)"""

    def _isotherm_inputs(self, v_wet, v_dry, f_org):
        k = self.const
        r_wet = np.cbrt(3 * v_wet / (4 * np.pi))
        with np.errstate(divide="ignore", invalid="ignore"):
            bulk = (f_org * v_dry / k.RUEHL_nu_org) / (v_wet / k.water_molar_volume)
            area = 4 * np.pi * r_wet ** 2 / (f_org * v_dry * k.N_A / k.RUEHL_nu_org)
        return bulk, area

    def sigma(self, T, v_wet, v_dry, f_org):
        k, name = self.const, self.__name__
        T, v_wet, v_dry, f_org = np.broadcast_arrays(*(np.asarray(a, dtype=float)
                                                       for a in (T, v_wet, v_dry, f_org)))
        if name == "Constant":
            return np.full(T.shape, k.sgm_w)
        if name == "CompressedFilmOvadnevaite":
            r_wet = np.cbrt(3 * v_wet / (4 * np.pi))
            v_delta = v_wet - 4 * np.pi / 3 * (r_wet - k.delta_min) ** 3
            c_beta = np.minimum(f_org * v_dry / v_delta, 1)
            return (1 - c_beta) * k.sgm_w + c_beta * k.sgm_org
        bulk, area = self._isotherm_inputs(v_wet, v_dry, f_org)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if name == "SzyszkowskiLangmuir":
                a = -k.RUEHL_A0 / area
                b = k.RUEHL_A0 / area * (1 + k.RUEHL_C0 / bulk) + 1
                f_surf = (-b + np.sqrt(b ** 2 + 4 * a)) / (2 * a)
                sgm = k.sgm_w - k.R_str * T / (k.RUEHL_A0 * k.N_A) * np.log(
                    1 + bulk * (1 - f_surf) / k.RUEHL_C0)
            else:  # CompressedFilmRuehl
                c = k.RUEHL_m_sigma * k.N_A / (2 * k.R_str * T)
                f_surf = _bisect(
                    lambda f: bulk * (1 - f) / k.RUEHL_C0
                    - np.exp(c * (k.RUEHL_A0 ** 2 - (area / f) ** 2)),
                    np.full(T.shape, 1e-16), np.ones(T.shape))
                sgm = k.sgm_w - (k.RUEHL_A0 - area / f_surf) * k.RUEHL_m_sigma
                sgm = np.where(f_org == 1, k.RUEHL_sgm_min, sgm)
        sgm = np.where(f_org == 0, k.sgm_w, sgm)
        return np.minimum(np.maximum(sgm, k.RUEHL_sgm_min), k.sgm_w)


OPTION_CLASSES = {"saturation_vapour_pressure": SaturationVapourPressure,
                  "hygroscopicity": Hygroscopicity, "surface_tension": SurfaceTension}


def make_option(option, name, constants):
    return OPTION_CLASSES.get(option, _Option)(name, constants)

"""`Formulae`: the options + constants object a PySDM-shaped backend is constructed with (a
stand-in for PySDM's own where PySDM is absent; under PySDM the real one is passed in).

Collision-path subset of PySDM/formulae.py:27-67 (same keyword names: `seed`, `constants`,
`terminal_velocity`, `fragmentation_function`, `handle_all_breakups`,
`particle_shape_and_density`, `particle_advection`), the options of the condensation path (the
choices of pysdm_amd/physics/condensation_formulae.py `CHOICES` but `HOST_REFUSED`) and of the freezing path (`particle_shape_and_density="MixedPhaseSpheres"`,
`heterogeneous_ice_nucleation_rate`, `homogeneous_ice_nucleation_rate`) and of vapour deposition on
ice (`diffusion_ice_capacity`, `diffusion_ice_kinetics`, `latent_heat_sublimation`,
`diffusion_coordinate="WaterMass"`); aqueous chemistry has no options, only `trivia` entries and
constants; everything unrelated to these paths is absent.
"""
import math
from types import SimpleNamespace

import numpy as np

from .physics import condensation_formulae as _cond
from .physics import constants as _const


# PySDM/formulae.py:27-67 defaults of the options the condensation path depends on
CONDENSATION_DEFAULTS = {
    "diffusion_coordinate": "WaterMassLogarithm",
    "saturation_vapour_pressure": "FlatauWalkoCotton",
    "latent_heat_vapourisation": "Kirchhoff",
    "hygroscopicity": "KappaKoehlerLeadingTerms",
    "drop_growth": "Mason1971",
    "surface_tension": "Constant",
    "diffusion_kinetics": "FuchsSutugin",
    "diffusion_thermics": "Neglect",
    "ventilation": "Neglect",
    "state_variable_triplet": "LibcloudphPlusPlus",
    "air_dynamic_viscosity": "ZografosEtAl1987",
}
# the choices the freezing path implements (pysdm_amd/freezing.py), PySDM's default first, and
# the constants each needs to be finite (as the reference's classes assert when instantiated)
FREEZING_OPTIONS = {
    "heterogeneous_ice_nucleation_rate": ("Null", "Constant", "ABIFM"),
    "homogeneous_ice_nucleation_rate": ("Null", "Constant", "Koop2000", "Koop_Correction",
                                        "KoopMurray2016"),
}
_FINITE = {
    ("heterogeneous_ice_nucleation_rate", "Constant"): ("J_HET",),
    ("heterogeneous_ice_nucleation_rate", "ABIFM"): ("ABIFM_M", "ABIFM_C"),
    ("homogeneous_ice_nucleation_rate", "Constant"): ("J_HOM",),
}
PARTICLE_SHAPES = ("LiquidSpheres", "MixedPhaseSpheres")
# the choices the deposition path implements (pysdm_amd/deposition.py), PySDM's default first.
# `diffusion_coordinate` is shared with condensation, whose `check_formulae` goes on refusing
# "WaterMass" (the library's general kernel serves it: condensation.descriptor_of)
DEPOSITION_OPTIONS = {
    "diffusion_ice_capacity": ("Spherical", "Columnar"),
    "diffusion_ice_kinetics": ("Standard", "Neglect"),
    "latent_heat_sublimation": ("MurphyKoop2005",),
}
DIFFUSION_COORDINATES = ("WaterMassLogarithm", "WaterMass")


def check_condensation_constants(option, value, constants):
    """the assertions the reference's classes make on the constants when constructed (finite
    sgm_org / delta_min / RUEHL_*, dv_pk05 == 0 for LoweEtAl2019), naming option and constant"""
    for name in _cond.FINITE.get((option, value), ()):
        if not math.isfinite(getattr(constants, name, math.nan)):
            raise NotImplementedError(f"{option}={value!r} needs the constant {name} "
                                      f"(pass constants={{'{name}': ...}})")
    for name in _cond.ZERO.get((option, value), ()):
        if getattr(constants, name, math.nan) != 0:
            raise ValueError(f"{option}={value!r} needs the constant {name} to be 0")


class _Trivia:  # PySDM/physics/trivia.py:19-28
    @staticmethod
    def volume(radius):
        return _const.PI_4_3 * np.power(radius, 3)

    @staticmethod
    def radius(volume):
        return np.power(volume / _const.PI_4_3, _const.ONE_THIRD)

    # trivia.py:39-64, what the aqueous-chemistry path's host side needs (pysdm_amd/chemistry.py)
    @staticmethod
    def within_tolerance(error_estimate, value, rtol):
        return error_estimate < rtol * np.abs(value)

    @staticmethod
    def H2pH(H):
        return -np.log10(H * 1e-3)

    @staticmethod
    def pH2H(pH):
        return np.power(10, -pH) * 1e3

    @staticmethod
    def mole_fraction_2_mixing_ratio(mole_fraction, specific_gravity):
        return specific_gravity * mole_fraction / (1 - mole_fraction)

    @staticmethod
    def mixing_ratio_2_mole_fraction(mixing_ratio, specific_gravity):
        return mixing_ratio / (specific_gravity + mixing_ratio)


class _LiquidSpheres:  # PySDM/physics/particle_shape_and_density/liquid_spheres.py:9-23
    __name__ = "LiquidSpheres"

    @staticmethod
    def supports_mixed_phase(_=None):
        return False

    @staticmethod
    def mass_to_volume(mass):
        return mass / _const.rho_w

    @staticmethod
    def volume_to_mass(volume):
        return _const.rho_w * volume


class _MixedPhaseSpheres:  # PySDM/physics/particle_shape_and_density/mixed_phase_spheres.py
    __name__ = "MixedPhaseSpheres"

    def __init__(self, constants):
        self._rho_w, self._rho_i = constants.rho_w, constants.rho_i

    @staticmethod
    def supports_mixed_phase(_=None):
        return True

    def mass_to_volume(self, mass):
        return np.maximum(0.0, mass) / self._rho_w + np.minimum(0.0, mass) / self._rho_i

    def volume_to_mass(self, volume):
        return np.maximum(0.0, volume) * self._rho_w + np.minimum(0.0, volume) * self._rho_i


class _ImplicitInSpace:  # PySDM/physics/particle_advection/implicit_in_space.py:11-13
    __name__ = "ImplicitInSpace"
    scheme_id = 0  # SDM scheme code of sdm_calculate_displacement

    @staticmethod
    def displacement(position_in_cell, c_l, c_r):
        return (c_l * (1 - position_in_cell) + c_r * position_in_cell) / (1 - c_r + c_l)


class _ExplicitInSpace:  # PySDM/physics/particle_advection/explicit_in_space.py:11-13
    __name__ = "ExplicitInSpace"
    scheme_id = 1

    @staticmethod
    def displacement(position_in_cell, c_l, c_r):
        return c_l * (1 - position_in_cell) + c_r * position_in_cell


class Formulae:  # pylint: disable=too-few-public-methods,too-many-arguments
    def __init__(
        self,
        *,
        constants=None,
        seed=None,
        fastmath=True,
        fragmentation_function="AlwaysN",
        particle_shape_and_density="LiquidSpheres",
        terminal_velocity="GunnKinzer1949",
        handle_all_breakups=False,
        particle_advection="ImplicitInSpace",
        heterogeneous_ice_nucleation_rate="Null",
        homogeneous_ice_nucleation_rate="Null",
        diffusion_ice_capacity="Spherical",
        diffusion_ice_kinetics="Standard",
        latent_heat_sublimation="MurphyKoop2005",
        **condensation_options,
    ):
        if particle_shape_and_density not in PARTICLE_SHAPES:
            raise NotImplementedError(
                f"particle_shape_and_density={particle_shape_and_density!r}")
        # the condensation path: any choice of `CHOICES`, freely combined (pysdm_amd/condensation.py)
        for option, value in condensation_options.items():
            if option not in CONDENSATION_DEFAULTS:
                raise TypeError(f"Formulae got an unexpected keyword argument '{option}'")
            allowed = _cond.CHOICES.get(option, (CONDENSATION_DEFAULTS[option],))
            if value not in allowed:
                raise NotImplementedError(f"{option}={value!r}")
            # (the coordinate is shared with deposition, which serves "WaterMass")
            if option != "diffusion_coordinate" and value in _cond.HOST_REFUSED.get(option, ()):
                raise NotImplementedError(
                    f"{option}={value!r}: served by the library, not yet through Formulae")
        for option, value in (("diffusion_ice_capacity", diffusion_ice_capacity),
                              ("diffusion_ice_kinetics", diffusion_ice_kinetics),
                              ("latent_heat_sublimation", latent_heat_sublimation)):
            if value not in DEPOSITION_OPTIONS[option]:
                raise NotImplementedError(f"{option}={value!r}")
            setattr(self, option, SimpleNamespace(__name__=value))
        if terminal_velocity not in ("GunnKinzer1949", "RogersYau", "PowerSeries"):
            raise NotImplementedError(terminal_velocity)
        values = {
            k: getattr(_const, k)
            for k in dir(_const)
            if not k.startswith("_") and isinstance(getattr(_const, k), (int, float))
        }
        values.update(constants or {})
        if "water_molar_volume" not in (constants or {}):  # constants_defaults.py:770
            values["water_molar_volume"] = values["Mv"] / values["rho_w"]
        self.constants = SimpleNamespace(**values)
        for option, default in CONDENSATION_DEFAULTS.items():
            value = condensation_options.get(option, default)
            check_condensation_constants(option, value, self.constants)
            setattr(self, option, _cond.make_option(option, value, self.constants))
        self.seed = seed if seed is not None else _const.default_random_seed
        self.fastmath = fastmath
        self.fragmentation_function = fragmentation_function
        self.handle_all_breakups = handle_all_breakups
        self.trivia = _Trivia()
        if particle_shape_and_density == "MixedPhaseSpheres":
            self.particle_shape_and_density = _MixedPhaseSpheres(self.constants)
        else:
            self.particle_shape_and_density = _LiquidSpheres()
        for option, value in (
                ("heterogeneous_ice_nucleation_rate", heterogeneous_ice_nucleation_rate),
                ("homogeneous_ice_nucleation_rate", homogeneous_ice_nucleation_rate)):
            if value not in FREEZING_OPTIONS[option]:
                raise NotImplementedError(f"{option}={value!r}")
            for name in _FINITE.get((option, value), ()):
                if not math.isfinite(getattr(self.constants, name)):
                    raise ValueError(f"{option}={value!r} needs the constant {name} "
                                     f"(pass constants={{'{name}': ...}})")
            setattr(self, option, SimpleNamespace(__name__=value))
        self.terminal_velocity = terminal_velocity
        schemes = {"ImplicitInSpace": _ImplicitInSpace, "ExplicitInSpace": _ExplicitInSpace}
        if particle_advection not in schemes:
            raise NotImplementedError(particle_advection)
        self.particle_advection = schemes[particle_advection]()

    def __str__(self):
        return f"Formulae(seed={self.seed}, fragmentation_function={self.fragmentation_function})"

"""Vapour deposition on ice on the library (include/sdm_deposition.h).

PySDM's `VapourDepositionOnIce` dynamic (PySDM/dynamics/vapour_deposition_on_ice.py) is one call
of `Particulator.deposition` per time step: every ice super-droplet (signed water mass not > 0)
grows or sublimates by vapour diffusion, and its cell's predicted water vapour mixing ratio and
dry potential temperature change accordingly.  `DepositionRunner` steps the signed water masses
of a `Population` over an `AmbientColumns(..., mixed_phase=True)` through `sdm_deposition`, one
call per time step and no synchronisation.

Supported: `particle_shape_and_density="MixedPhaseSpheres"`, `diffusion_coordinate` in
{WaterMassLogarithm, WaterMass}, `diffusion_ice_capacity` in {Spherical, Columnar},
`diffusion_ice_kinetics` in {Standard, Neglect}, `latent_heat_sublimation="MurphyKoop2005"`, and
PySDM's defaults for what else the path reads (`check_formulae`); any other choice raises
NotImplementedError naming the option.
"""
import numpy as np

from .abi import DepositionCfg
from .engine import INT

# the order of include/sdm_deposition.h SDM_DEP_K_*
CONSTANT_NAMES = (
    "rho_w", "rho_i", "Rv", "Rd", "c_pd", "eps", "p1000", "Rd_over_c_pd", "PI", "PI_4_3",
    "ONE_THIRD", "T0", *(f"FWC_I{i}" for i in range(9)), "Mv",
    *(f"MK05_SUB_C{i}" for i in range(1, 6)), "D0", "K0", "lmbd_w_0", "T_STP", "p_STP", "C_cunn",
    "MAC_ice", "HAC_ice", "capacity_columnar_ice_A1", "capacity_columnar_ice_B1",
    "capacity_columnar_ice_A2", "capacity_columnar_ice_B2",
)
# SDM_DEP_COORD_* / SDM_DEP_CAPACITY_* / SDM_DEP_KINETICS_* / SDM_DEP_SUM_*
OPTION_CODES = {
    "diffusion_coordinate": {"WaterMassLogarithm": 0, "WaterMass": 1},
    "diffusion_ice_capacity": {"Spherical": 0, "Columnar": 1},
    "diffusion_ice_kinetics": {"Standard": 0, "Neglect": 1},
}
SUMS = {"ordered": 0, "blocked": 1}
# what else the path evaluates (PySDM's defaults)
REQUIRED_OPTIONS = {
    "latent_heat_sublimation": "MurphyKoop2005",
    "saturation_vapour_pressure": "FlatauWalkoCotton",
    "diffusion_thermics": "Neglect",
    "drop_growth": "Mason1971",
    "state_variable_triplet": "LibcloudphPlusPlus",
    "ventilation": "Neglect",
}


def _option_name(value):
    if isinstance(value, str):
        return value
    return getattr(value, "__name__", type(value).__name__)


def check_formulae(formulae):
    """refuses what the deposition path does not implement, naming the option"""
    shape = getattr(formulae, "particle_shape_and_density", None)
    if shape is None or not shape.supports_mixed_phase():
        raise NotImplementedError(
            "deposition needs particle_shape_and_density='MixedPhaseSpheres', not "
            f"{_option_name(shape)!r}")
    if _option_name(shape) != "MixedPhaseSpheres":
        raise NotImplementedError(f"particle_shape_and_density={_option_name(shape)!r}")
    for option, codes in OPTION_CODES.items():
        value = getattr(formulae, option, None)
        if value is None:
            raise NotImplementedError(f"deposition: formulae lack `{option}`")
        if _option_name(value) not in codes:
            raise NotImplementedError(f"{option}={_option_name(value)!r}")
    for option, default in REQUIRED_OPTIONS.items():
        value = getattr(formulae, option, None)
        if value is not None and _option_name(value) != default:
            raise NotImplementedError(
                f"deposition on this backend supports {option}={default!r} only, "
                f"not {_option_name(value)!r}")


def constants_of(formulae):
    """`formulae.constants` as the `consts` array of include/sdm_deposition.h"""
    k = formulae.constants
    return [float(getattr(k, name)) for name in CONSTANT_NAMES]


def deposition_cfg(formulae, time_step, cell_volume, sum="ordered"):  # pylint: disable=redefined-builtin
    """`sdm_deposition_cfg` of a formulae object (checked first)"""
    check_formulae(formulae)
    if sum not in SUMS:
        raise ValueError(f"sum={sum!r}: one of {sorted(SUMS)}")
    cfg = DepositionCfg()
    cfg.coordinate = OPTION_CODES["diffusion_coordinate"][
        _option_name(formulae.diffusion_coordinate)]
    cfg.capacity = OPTION_CODES["diffusion_ice_capacity"][
        _option_name(formulae.diffusion_ice_capacity)]
    cfg.kinetics = OPTION_CODES["diffusion_ice_kinetics"][
        _option_name(formulae.diffusion_ice_kinetics)]
    cfg.sum = SUMS[sum]
    cfg.time_step, cfg.cell_volume = float(time_step), float(cell_volume)
    return cfg


def raise_if_exceeded(count):
    """the reference asserts on the first such row (deposition_methods.py:112-113)"""
    if count != 0:
        raise RuntimeError(
            f"deposition: {int(count)} super-droplet(s) would take more vapour from their cell "
            "than it holds (-delta_rv_i > current_vapour_mixing_ratio)")


class DepositionRunner:  # pylint: disable=too-many-instance-attributes
    """PySDM's `VapourDepositionOnIce` over a `Population` (its mass column is the signed water
    mass) and an `AmbientColumns(..., mixed_phase=True)`: `step()` reads the ambient's current
    columns and adds to its predicted qv / thd; the caller decides when
    `ambient.accept_predictions()` runs.  `sum`: "ordered" (the reference's bits) or "blocked"
    (include/sdm_deposition.h: SDM_DEP_SUM_BLOCKED).  The rows for which the reference would
    assert are counted on the device over all steps; `check()` / `snapshot()` read the count and
    raise if it is not zero."""

    def __init__(self, population, ambient, *, dt, dv, formulae=None, sum="ordered"):  # pylint: disable=redefined-builtin
        self.population, self.ambient = population, ambient
        self.formulae = formulae or ambient.formulae
        if not getattr(ambient, "mixed_phase", False):
            raise ValueError("deposition needs AmbientColumns(..., mixed_phase=True): a_w_ice")
        self.cfg = deposition_cfg(self.formulae, dt, dv, sum)
        self.consts = constants_of(self.formulae)
        eng = self.engine = population.engine
        self.n_sd, self.n_cell = int(population.n_sd), int(population.n_cell)
        self.n_exceeded_step = eng.zeros(1, INT)
        self.n_exceeded = eng.zeros(1, INT)

    @property
    def signed_water_mass(self):
        pop = self.population
        return pop.signed_water_mass if hasattr(pop, "signed_water_mass") else pop.mass

    def step(self):
        """one `Particulator.deposition()`: one `sdm_deposition` call, nothing is waited for"""
        pop, amb = self.population, self.ambient
        self.engine.call_deposition(
            "sdm_deposition", self.cfg, self.n_sd, self.n_cell, pop.multiplicity,
            self.signed_water_mass, pop.cell_id, amb.T, amb.p, amb.RH, amb.a_w_ice, amb.qv,
            amb.rhod, amb.thd, amb.pqv, amb.pthd, self.n_exceeded_step, self.consts)
        self.n_exceeded += self.n_exceeded_step  # (on the device: the call sets its count)
        if hasattr(pop, "touch_state"):
            pop.touch_state()

    def run(self, n_steps):
        for _ in range(int(n_steps)):
            self.step()

    def check(self):
        """raises if, in any step so far, a row took more vapour than its cell held"""
        raise_if_exceeded(int(np.asarray(self.engine.download(self.n_exceeded))[0]))

    def snapshot(self):
        """host copies: signed water mass and the ambient's current and predicted columns"""
        self.check()
        down, amb = self.engine.download, self.ambient
        return {"signed_water_mass": down(self.signed_water_mass), "qv": down(amb.qv),
                "thd": down(amb.thd), "pqv": down(amb.pqv), "pthd": down(amb.pthd)}

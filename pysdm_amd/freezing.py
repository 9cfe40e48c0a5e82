"""Droplet freezing on the library (include/sdm_freezing.h).

`FreezingSetup` holds the keywords of PySDM's `Freezing` dynamic (PySDM/dynamics/freezing.py:12-27)
plus `record_freezing_temperature` (what requesting the attribute "temperature of last freezing"
does under PySDM); `FreezingRunner` steps the signed water masses of a `Population` - or of plain
columns - through `sdm_freezing_step`, one launch per time step, and keeps the position in the
NumPy-PCG64 stream as PySDM's `Random` does (n_sd numbers per stochastic pass).

A super-droplet's phase is the sign of its signed water mass (> 0 liquid, < 0 ice), which needs
`particle_shape_and_density="MixedPhaseSpheres"`.  Supported: `heterogeneous_ice_nucleation_rate`
in {Constant, ABIFM}, `homogeneous_ice_nucleation_rate` in {Constant, Koop2000, Koop_Correction,
KoopMurray2016} (Null where the pass is off); any other choice raises NotImplementedError naming
the option (`check_formulae`).
"""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from .abi import FreezingCfg, pcg64_state_inc
from .engine import FLOAT

# the order of include/sdm_freezing.h SDM_FRZ_K_*
CONSTANT_NAMES = (
    "T0", "rho_w", "rho_i", "eps", *(f"FWC_I{i}" for i in range(9)),
    "J_HET", "ABIFM_M", "ABIFM_C", "ABIFM_UNIT", "J_HOM",
    *(f"KOOP_2000_C{i}" for i in range(1, 5)), "KOOP_CORR", "KOOP_UNIT", "KOOP_MIN_DA_W_ICE",
    "KOOP_MAX_DA_W_ICE", *(f"KOOP_MURRAY_C{i}" for i in range(7)),
)
# SDM_FRZ_JHET_* / SDM_FRZ_JHOM_* / SDM_FRZ_RATES_*
J_HET_CODES = {"Constant": 0, "ABIFM": 1}
J_HOM_CODES = {"Constant": 0, "Koop2000": 1, "Koop_Correction": 2, "KoopMurray2016": 3}
RATES = {"auto": 0, "per_droplet": 1, "per_cell": 2}
# a_w_ice / RH_ice are written for these (PySDM's defaults)
REQUIRED_OPTIONS = {"saturation_vapour_pressure": "FlatauWalkoCotton",
                    "state_variable_triplet": "LibcloudphPlusPlus"}


def _option_name(value):
    if isinstance(value, str):
        return value
    return getattr(value, "__name__", type(value).__name__)


def _rate_name(formulae, option):
    value = getattr(formulae, option, None)
    return "Null" if value is None else _option_name(value)


def check_formulae(formulae):
    """refuses what the freezing path does not implement, naming the option"""
    shape = getattr(formulae, "particle_shape_and_density", None)
    if shape is None or not shape.supports_mixed_phase():
        raise NotImplementedError(
            "freezing needs particle_shape_and_density='MixedPhaseSpheres', not "
            f"{_option_name(shape)!r}")
    if _option_name(shape) != "MixedPhaseSpheres":
        raise NotImplementedError(f"particle_shape_and_density={_option_name(shape)!r}")
    for option, default in REQUIRED_OPTIONS.items():
        value = getattr(formulae, option, None)
        if value is not None and _option_name(value) != default:
            raise NotImplementedError(
                f"freezing on this backend supports {option}={default!r} only, "
                f"not {_option_name(value)!r}")
    for option, codes in (("heterogeneous_ice_nucleation_rate", J_HET_CODES),
                          ("homogeneous_ice_nucleation_rate", J_HOM_CODES)):
        name = _rate_name(formulae, option)
        if name != "Null" and name not in codes:
            raise NotImplementedError(f"{option}={name!r}")


def constants_of(formulae):
    """`formulae.constants` as the `consts` array of include/sdm_freezing.h"""
    k = formulae.constants
    return [float(getattr(k, name)) for name in CONSTANT_NAMES]


def j_het_code(formulae):
    """SDM_FRZ_JHET_* of `formulae.heterogeneous_ice_nucleation_rate`"""
    name = _rate_name(formulae, "heterogeneous_ice_nucleation_rate")
    if name not in J_HET_CODES:
        raise NotImplementedError(f"heterogeneous_ice_nucleation_rate={name!r}")
    return J_HET_CODES[name]


def j_hom_code(formulae):
    """SDM_FRZ_JHOM_* of `formulae.homogeneous_ice_nucleation_rate`"""
    name = _rate_name(formulae, "homogeneous_ice_nucleation_rate")
    if name not in J_HOM_CODES:
        raise NotImplementedError(f"homogeneous_ice_nucleation_rate={name!r}")
    return J_HOM_CODES[name]


@dataclass(frozen=True)
class FreezingSetup:
    """PySDM's `Freezing(...)` keywords; `record_freezing_temperature` keeps the per-droplet
    "temperature of last freezing" (NaN while liquid); `rates`: how the fused step obtains the
    nucleation rates ("auto", "per_droplet", "per_cell": same results, different speed)"""

    singular: bool = True
    homogeneous_freezing: bool = False
    immersion_freezing: bool = True
    thaw: bool = False
    record_freezing_temperature: bool = False
    rates: str = "auto"

    def __post_init__(self):
        if self.rates not in RATES:
            raise ValueError(f"rates={self.rates!r}: one of {sorted(RATES)}")
        if self.record_freezing_temperature and self.singular:
            # attributes/ice/freezing_temperature.py: the attribute asserts `not singular`
            raise ValueError("the temperature of last freezing is recorded in the "
                             "time-dependent regime only (singular=False)")

    @property
    def n_stochastic_passes(self):
        return int(self.immersion_freezing and not self.singular) + int(
            self.homogeneous_freezing)


def freezing_cfg(setup, formulae, timestep, seed):
    """`sdm_freezing_cfg` of a setup (the rate codes only of the passes that are on, as
    `Freezing.register` asserts them, dynamics/freezing.py:40-52)"""
    cfg = FreezingCfg()
    cfg.singular, cfg.thaw = int(setup.singular), int(setup.thaw)
    cfg.immersion_freezing = int(setup.immersion_freezing)
    cfg.homogeneous_freezing = int(setup.homogeneous_freezing)
    cfg.j_het = j_het_code(formulae) if setup.immersion_freezing and not setup.singular else 0
    cfg.j_hom = j_hom_code(formulae) if setup.homogeneous_freezing else 0
    cfg.rates = RATES[setup.rates]
    cfg.timestep = float(timestep)
    cfg.rng_state_inc[:] = pcg64_state_inc(int(seed))
    return cfg


class PrescribedAmbient:  # pylint: disable=too-few-public-methods
    """per-cell T, RH, a_w_ice and RH_ice set by the caller (what PySDM's `Box` holds); an
    `AmbientColumns(..., mixed_phase=True)` computes them from rhod / thd / qv instead"""

    NAMES = ("T", "RH", "a_w_ice", "RH_ice")

    def __init__(self, engine, n_cell=1, **values):
        self.engine = engine
        for name in self.NAMES:
            setattr(self, name, engine.full(int(n_cell), FLOAT, np.nan))
        self.set(**values)

    def set(self, **values):
        for name, value in values.items():
            if name not in self.NAMES:
                raise KeyError(name)
            column = getattr(self, name)
            host = np.broadcast_to(np.asarray(value, dtype=float), tuple(column.shape))
            self.engine.assign(column, self.engine.upload(np.ascontiguousarray(host)))


class FreezingRunner:  # pylint: disable=too-many-instance-attributes
    """PySDM's `Freezing` dynamic over a population: a `Population` (its mass column is the signed
    water mass) or any object with `engine`, `n_sd`, `n_cell`, `signed_water_mass` and `cell_id`
    (engine arrays; `columns(...)` builds one).  Per-droplet inputs: `freezing_temperature`
    (singular) or `immersed_surface_area` (time-dependent immersion freezing).  The volume of the
    homogeneous pass is the MixedPhaseSpheres volume of the current mass, as PySDM's `volume`
    attribute, unless a fixed `volume` column is given."""

    def __init__(self, population, setup, ambient, dt, seed, *, formulae,
                 freezing_temperature=None, immersed_surface_area=None, volume=None):
        check_formulae(formulae)
        self.population, self.setup, self.ambient = population, setup, ambient
        self.formulae, self.dt = formulae, float(dt)
        eng = self.engine = population.engine
        self.n_sd, self.n_cell = int(population.n_sd), int(population.n_cell)
        self.cfg = freezing_cfg(setup, formulae, dt, seed)
        self.consts = constants_of(formulae)
        self.rng_offset = 0

        def column(values, what):
            if values is None:
                raise ValueError(f"this Freezing setup needs `{what}`")
            return eng.upload(np.ascontiguousarray(values, dtype=float))

        singular_pass = setup.immersion_freezing and setup.singular
        stochastic_pass = setup.immersion_freezing and not setup.singular
        self.freezing_temperature = (column(freezing_temperature, "freezing_temperature")
                                     if singular_pass else None)
        self.immersed_surface_area = (column(immersed_surface_area, "immersed_surface_area")
                                      if stochastic_pass else None)
        self.volume = None if volume is None else column(volume, "volume")
        self.temperature_of_last_freezing = (eng.full(self.n_sd, FLOAT, np.nan)
                                             if setup.record_freezing_temperature else None)

    @property
    def signed_water_mass(self):
        pop = self.population
        return pop.signed_water_mass if hasattr(pop, "signed_water_mass") else pop.mass

    def step(self):
        """one `Freezing.__call__` (and the attribute update behind it): one launch"""
        amb, setup = self.ambient, self.setup
        self.engine.call_freezing(
            "sdm_freezing_step", self.cfg, self.rng_offset, self.n_sd, self.n_cell,
            self.signed_water_mass, self.freezing_temperature, self.immersed_surface_area,
            self.volume, self.population.cell_id, self.temperature_of_last_freezing, amb.T, amb.RH,
            amb.a_w_ice, amb.RH_ice, self.consts)
        self.rng_offset += self.n_sd * setup.n_stochastic_passes
        if hasattr(self.population, "touch_state"):
            self.population.touch_state()

    def run(self, n_steps):
        for _ in range(int(n_steps)):
            self.step()

    def snapshot(self):
        """host copies: signed water mass (and the temperature of last freezing, if recorded)"""
        out = {"signed_water_mass": self.engine.download(self.signed_water_mass)}
        if self.temperature_of_last_freezing is not None:
            out["temperature_of_last_freezing"] = self.engine.download(
                self.temperature_of_last_freezing)
        return out


def columns(engine, *, signed_water_mass, cell_id=None, n_cell=1):
    """the minimal population `FreezingRunner` accepts, from host arrays"""
    mass = np.ascontiguousarray(signed_water_mass, dtype=float)
    cells = (np.zeros(mass.shape[0], dtype=np.int64) if cell_id is None
             else np.ascontiguousarray(cell_id, dtype=np.int64))
    return SimpleNamespace(engine=engine, n_sd=int(mass.shape[0]), n_cell=int(n_cell),
                           signed_water_mass=engine.upload(mass), cell_id=engine.upload(cells))

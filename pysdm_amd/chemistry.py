"""Aqueous chemistry on the library (include/sdm_chemistry.h).

PySDM's `AqueousChemistry` dynamic (PySDM/dynamics/aqueous_chemistry.py) walks the whole state
6 x `n_substep` times per time step: the pH of every super-droplet by a TOMS748 root search
(`equilibrate_H`), six dissociation factors, a Henry-law relaxation of six gases (`dissolution`)
and an explicit Euler step of S(IV) oxidation by O3 and H2O2 (`oxidation`).  `ChemistryRunner`
steps the seven mole columns, the pH and the flag of a `Population` over an `AmbientColumns`
through `sdm_chemistry_step`, one call per time step and no synchronisation;
`step_by_stages()` is the same sequence through the stage symbols, which are the reference's
backend methods.

The path has no formulae options: it reads `trivia` and constants only.  `check_formulae` refuses
constants the path cannot work with, by name.  Nothing here imports `chempy`: the molar masses
the reference takes from it are the table `MOLAR_MASS` below.
"""
import numpy as np

from .abi import ChemistryCfg
from .engine import FLOAT, INT
from .physics import constants as _const

# the orders of include/sdm_chemistry.h
GASES = ("HNO3", "H2O2", "NH3", "SO2", "CO2", "O3")            # SDM_CHEM_GAS_*
GAS_KEYS = ("N_V", "H2O2", "N_mIII", "S_IV", "C_IV", "O3")      # the aqueous column of each gas
AQUEOUS = ("S_IV", "O3", "H2O2", "C_IV", "N_V", "N_mIII", "S_VI")  # SDM_CHEM_AQ_*
EQUILIBRIUM = ("K_HNO3", "K_SO2", "K_NH3", "K_CO2", "K_HSO3", "K_HCO3", "K_HSO4")
KINETIC = ("k0", "k1", "k2", "k3")
CONC = ("N_mIII", "N_V", "C_IV", "S_IV", "S_VI")                # SDM_CHEM_CONC_*
SYSTEM_TYPES = {"open": 0, "closed": 1}
SUMS = {"ordered": 0, "blocked": 1}
CONSTANTS_ROUTES = {"auto": 0, "per_row": 1, "per_cell": 2}  # SDM_CHEM_CONSTS_*
LDS_CELLS = 256  # SDM_CHEM_LDS_CELLS

# PySDM/dynamics/impl/chemistry_utils.py (Kreidenweis et al. 2003, Table 4): value at ROOM_TEMP in
# the unit named, dT in K
_EQUILIBRIUM = {"K_HNO3": (15.4, 8700), "K_SO2": (1.3e-2, 1960), "K_NH3": (1.7e-5, -450),
                "K_CO2": (4.3e-7, -1000), "K_HSO3": (6.6e-8, 1500), "K_HCO3": (4.68e-11, -1760),
                "K_HSO4": (1.2e-2, 2720)}                        # x M
_HENRY = {"HNO3": (2.1e5, 8700), "H2O2": (7.45e4, 7300), "NH3": (62, 4110), "SO2": (1.23, 3150),
          "CO2": (3.4e-2, 2440), "O3": (1.13e-2, 2540)}          # x H_u
_KINETIC = {"k0": (2.4e4, 1, 0), "k1": (3.5e5, 1, -5530), "k2": (1.5e9, 1, -5280),
            "k3": (7.45e7, 2, -4430)}                            # / M (once or twice)
DIFFUSION_CONST = {"HNO3": 65.25e-6, "H2O2": 87.00e-6, "NH3": 19.78e-6, "SO2": 10.89e-6,
                   "CO2": 13.81e-6, "O3": 14.44e-6}
MASS_ACCOMMODATION_COEFFICIENTS = {"HNO3": 0.05, "H2O2": 0.018, "NH3": 0.05, "SO2": 0.035,
                                   "CO2": 0.05, "O3": 0.00053}

# Molar masses of the six gases in g / mol, where the reference asks
# `chempy.Substance.from_formula(compound).mass`: sums of standard atomic weights in the order of
# the formula.  NOBODY HAS COMPARED THIS TABLE WITH `chempy` ITSELF: the recorded goldens were
# generated with the same sums in place of it.  A caller who has chempy's
# values passes them as `molar_mass=` (`constants_of`, `ChemistryRunner`, the backend's
# `chemistry_molar_mass` attribute).
ATOMIC_WEIGHTS = {"H": 1.008, "C": 12.011, "N": 14.007, "O": 15.999, "S": 32.06}
_COMPOSITION = {"HNO3": (("H", 1), ("N", 1), ("O", 3)), "H2O2": (("H", 2), ("O", 2)),
                "NH3": (("N", 1), ("H", 3)), "SO2": (("S", 1), ("O", 2)),
                "CO2": (("C", 1), ("O", 2)), "O3": (("O", 3),)}


def _mass(composition):
    mass = 0.0
    for element, count in composition:
        mass += ATOMIC_WEIGHTS[element] * count
    return mass


MOLAR_MASS = {gas: _mass(_COMPOSITION[gas]) for gas in GASES}

# the order of include/sdm_chemistry.h SDM_CHEM_K_*
CONSTANT_NAMES = (
    "R_str", "Md", "Rd", "ROOM_TEMP", "K_H2O", "M", "PI_4_3", "ONE_THIRD", "pi", "k4",
    *(f"DIFFUSION_CONST_{g}" for g in GASES), *(f"MASS_ACCOMMODATION_{g}" for g in GASES),
    *(f"MOLAR_MASS_{g}" for g in GASES),
    *EQUILIBRIUM, *(f"dT_{k}" for k in EQUILIBRIUM),
    *(f"HENRY_{g}" for g in GASES), *(f"dT_HENRY_{g}" for g in GASES),
    *KINETIC, *(f"dT_{k}" for k in KINETIC),
)
# PySDM/dynamics/aqueous_chemistry.py:18-20 (ionic_strength_threshold: 0.02 M)
DEFAULTS = {"pH_min": -1.0, "pH_max": 14.0, "pH_rtol": 1e-6, "ionic_strength_threshold": 0.02}


def _constant(formulae, name):
    """a constant of the formulae object, else this package's (PySDM's defaults)"""
    value = getattr(formulae.constants, name, None)
    return getattr(_const, name) if value is None else value


def constants_table(formulae, molar_mass=None):
    """{name: value} in the order of CONSTANT_NAMES.  Every entry can be overridden by a constant
    of that name in `formulae.constants` (`Formulae(constants={"K_SO2": ...})`); the values at
    ROOM_TEMP are otherwise built from M, H_u and dT_u as chemistry_utils.py builds them.
    `molar_mass`: {gas: g / mol} replacing entries of MOLAR_MASS"""
    get = lambda name: float(_constant(formulae, name))  # noqa: E731
    M, H_u, dT_u = get("M"), get("H_u"), get("dT_u")
    table = {name: get(name) for name in ("R_str", "Md", "Rd", "ROOM_TEMP", "K_H2O", "M", "PI_4_3",
                                          "ONE_THIRD")}
    table["pi"] = float(np.pi)
    table["k4"] = 13 / M
    masses = dict(MOLAR_MASS)
    unknown = set(molar_mass or {}) - set(GASES)
    if unknown:
        raise ValueError(f"molar_mass of {sorted(unknown)}: the gases are {GASES}")
    masses.update(molar_mass or {})
    for gas in GASES:
        table[f"DIFFUSION_CONST_{gas}"] = DIFFUSION_CONST[gas]
    for gas in GASES:
        table[f"MASS_ACCOMMODATION_{gas}"] = MASS_ACCOMMODATION_COEFFICIENTS[gas]
    for gas in GASES:
        table[f"MOLAR_MASS_{gas}"] = float(masses[gas])
    for name in EQUILIBRIUM:
        table[name] = _EQUILIBRIUM[name][0] * M
    for name in EQUILIBRIUM:
        table[f"dT_{name}"] = _EQUILIBRIUM[name][1] * dT_u
    for gas in GASES:
        table[f"HENRY_{gas}"] = _HENRY[gas][0] * H_u
    for gas in GASES:
        table[f"dT_HENRY_{gas}"] = _HENRY[gas][1] * dT_u
    for name in KINETIC:
        value, order, _ = _KINETIC[name]
        table[name] = value / M if order == 1 else value / M / M
    for name in KINETIC:
        table[f"dT_{name}"] = _KINETIC[name][2] * dT_u
    for name in CONSTANT_NAMES[10:]:
        override = getattr(formulae.constants, name, None)
        if override is not None and not name.startswith("MOLAR_MASS_"):
            table[name] = float(override)
    return {name: float(table[name]) for name in CONSTANT_NAMES}


def constants_of(formulae, molar_mass=None):
    """the `consts` array of include/sdm_chemistry.h"""
    return list(constants_table(formulae, molar_mass).values())


def check_formulae(formulae, molar_mass=None):
    """refuses constants the chemistry path cannot work with, naming them"""
    trivia = getattr(formulae, "trivia", None)
    if trivia is None or not hasattr(trivia, "pH2H"):
        raise NotImplementedError("chemistry: formulae lack `trivia.pH2H`")
    table = constants_table(formulae, molar_mass)
    for name, value in table.items():
        if not np.isfinite(value):
            raise ValueError(f"chemistry: the constant {name} is {value}")
        if value <= 0 and not name.startswith("dT_"):
            raise ValueError(f"chemistry: the constant {name} must be positive, not {value}")
    return table


def specific_gravities(formulae, molar_mass=None):
    """{gas: molar mass / Md} as chemistry_utils.SpecificGravities computes it for the six gases"""
    table = constants_table(formulae, molar_mass)
    return {gas: table[f"MOLAR_MASS_{gas}"] * 1e-3 / table["Md"] for gas in GASES}


def mixing_ratios_of(mole_fractions, formulae, molar_mass=None):
    """{gas: mixing ratio} of {gas: mole fraction} (trivia.mole_fraction_2_mixing_ratio, as
    AqueousChemistry.register does); values may be scalars or per-cell arrays"""
    gravity = specific_gravities(formulae, molar_mass)
    missing = [gas for gas in GASES if gas not in mole_fractions]
    if missing:
        raise ValueError(f"mole fractions of {missing} are missing")
    return {gas: gravity[gas] * np.asarray(mole_fractions[gas], dtype=float)
            / (1 - np.asarray(mole_fractions[gas], dtype=float)) for gas in GASES}


class TemperatureDependent:  # pylint: disable=too-few-public-methods
    """host-side `.at(T)` of one constant (chemistry_utils.EqConst / KinConst), for callers that
    read `backend.HENRY_CONST.HENRY_CONST[...]` and the like; the library evaluates its own"""

    def __init__(self, table, value, dT, kinetic):
        self.K, self.dT, self.kinetic = value, dT, kinetic
        self.R_str, self.T0 = table["R_str"], table["ROOM_TEMP"]

    def at(self, T):
        enthalpy = -self.dT * self.R_str
        if self.kinetic:
            A = self.K * np.exp(enthalpy / (self.R_str * self.T0))
            return A * np.exp(-enthalpy / (self.R_str * T))
        return self.K * np.exp(-enthalpy / self.R_str * (1 / T - 1 / self.T0))


def raise_if_counted(counts):
    """the reference asserts on the first such event (chemistry_methods.py:147,154,426)"""
    failed, negative, exceeded = (int(c) for c in counts)
    if failed:
        raise RuntimeError(f"chemistry: {failed} pH solve(s) did not converge (used all their "
                           "iterations, or the bracket H_min .. H_max holds no sign change)")
    if negative:
        raise RuntimeError(f"chemistry: {negative} new mole amount(s) not >= 0 in dissolution")
    if exceeded:
        raise RuntimeError(f"chemistry: {exceeded} gas(es) of a cell would lose more than the "
                           "cell holds (delta_mr > env_mixing_ratio)")


class ChemistrySetup:  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """the arguments of PySDM's `AqueousChemistry` that shape the step, with its DEFAULTS;
    `sum`: "ordered" (the reference's bits) or "blocked" (SDM_CHEM_SUM_BLOCKED); `constants`:
    where the fused step gets a cell's constants from, "auto", "per_row" or "per_cell" (up to
    LDS_CELLS cells; the same bits either way)"""

    def __init__(self, system_type, n_substep, *, ionic_strength_threshold=None, pH_H_min=None,
                 pH_H_max=None, pH_rtol=DEFAULTS["pH_rtol"], sum="ordered", constants="auto"):  # pylint: disable=redefined-builtin
        if system_type not in SYSTEM_TYPES:
            raise ValueError(f"system_type={system_type!r}: one of {sorted(SYSTEM_TYPES)}")
        if not (isinstance(n_substep, (int, np.integer)) and n_substep > 0):
            raise ValueError(f"n_substep={n_substep!r}: a positive integer")
        if sum not in SUMS:
            raise ValueError(f"sum={sum!r}: one of {sorted(SUMS)}")
        if constants not in CONSTANTS_ROUTES:
            raise ValueError(f"constants={constants!r}: one of {sorted(CONSTANTS_ROUTES)}")
        self.system_type, self.n_substep, self.sum = system_type, int(n_substep), sum
        self.constants = constants
        self.ionic_strength_threshold = ionic_strength_threshold
        self.pH_H_min, self.pH_H_max, self.pH_rtol = pH_H_min, pH_H_max, float(pH_rtol)

    def cfg(self, formulae, timestep, cell_volume):
        """`sdm_chemistry_cfg`; the defaults that depend on the formulae are resolved here
        (aqueous_chemistry.py:76-79: H_max = pH2H(pH_min), H_min = pH2H(pH_max))"""
        cfg = ChemistryCfg()
        cfg.n_substep = self.n_substep
        cfg.system_type, cfg.sum = SYSTEM_TYPES[self.system_type], SUMS[self.sum]
        cfg.constants = CONSTANTS_ROUTES[self.constants]
        cfg.timestep, cfg.cell_volume = float(timestep), float(cell_volume)
        pH2H = formulae.trivia.pH2H
        cfg.H_min = float(pH2H(DEFAULTS["pH_max"]) if self.pH_H_min is None else self.pH_H_min)
        cfg.H_max = float(pH2H(DEFAULTS["pH_min"]) if self.pH_H_max is None else self.pH_H_max)
        threshold = self.ionic_strength_threshold
        if threshold is None:
            threshold = DEFAULTS["ionic_strength_threshold"] * float(_constant(formulae, "M"))
        cfg.ionic_strength_threshold = float(threshold)
        cfg.rtol = self.pH_rtol
        return cfg


class ChemistryRunner:  # pylint: disable=too-many-instance-attributes
    """PySDM's `AqueousChemistry` over a `Population` whose extensive rows include the seven
    `moles_*` columns, and an `AmbientColumns` (T, p, rhod).  The runner owns `pH` (filled with
    `pH_w`), `do_chemistry_flag` and the six per-cell mixing ratios (from `mole_fractions`).
    `step()` is one `sdm_chemistry_step`; `step_by_stages()` the same sequence through the stage
    symbols.  What the reference asserts on is counted on the device over all steps; `check()` /
    `snapshot()` read the three counts and raise if one is not zero."""

    def __init__(self, population, setup, ambient, *, dt, dv, mole_fractions, formulae=None,
                 molar_mass=None, volume=None):
        """`volume`: the droplet volumes as a host array, where they are not to be derived from
        the population's water masses (`Population.volume()`)"""
        self.population, self.setup, self.ambient = population, setup, ambient
        self.formulae = formulae or ambient.formulae
        check_formulae(self.formulae, molar_mass)
        missing = [f"moles_{k}" for k in AQUEOUS if f"moles_{k}" not in population.rows]
        if missing:
            raise ValueError(f"the population lacks the extensive rows {missing}")
        if int(population.live) != int(population.n_sd):
            raise ValueError("chemistry steps every row: compact the population first "
                             f"({population.live} of {population.n_sd} rows are live)")
        eng = self.engine = population.engine
        self.n_sd, self.n_cell = int(population.n_sd), int(population.n_cell)
        self.dt, self.dv = float(dt), float(dv)
        self.cfg = setup.cfg(self.formulae, dt, dv)
        self.consts = constants_of(self.formulae, molar_mass)
        self.pH = eng.full(self.n_sd, FLOAT, float(_constant(self.formulae, "pH_w")))
        self.do_chemistry_flag = eng.zeros(self.n_sd, np.uint8)
        ratios = mixing_ratios_of(mole_fractions, self.formulae, molar_mass)
        self.mixing_ratios = [eng.upload(np.broadcast_to(ratios[g], (self.n_cell,)).copy())
                              for g in GASES]
        self.counts_step = eng.zeros(3, INT)
        self.counts = eng.zeros(3, INT)
        self._volume = None if volume is None else eng.upload(np.asarray(volume, dtype=float))
        self._stage = None

    def volume(self):
        return self.population.volume() if self._volume is None else self._volume

    def moles(self, key):
        return self.population.extensive[self.population.rows[f"moles_{key}"]]

    def _columns(self):
        return [self.moles(k) for k in AQUEOUS]

    def _index(self):
        pop = self.population
        cell_start = pop.sorted_cell_start()
        return pop.perm, cell_start

    def step(self):
        """one `AqueousChemistry.__call__`: one `sdm_chemistry_step`, nothing is waited for"""
        pop, amb = self.population, self.ambient
        idx, cell_start = self._index()
        self.engine.call_chemistry(
            "sdm_chemistry_step", self.cfg, self.n_sd, self.n_cell, idx, cell_start, pop.cell_id,
            pop.multiplicity, self.volume(), self._columns(), self.pH, self.do_chemistry_flag,
            amb.T, amb.p, amb.rhod, self.mixing_ratios, self.counts_step, self.consts)
        self.counts += self.counts_step  # (on the device: the call sets its counts)

    def step_by_stages(self):
        """the definition of `sdm_chemistry_step` (include/sdm_chemistry.h) through the stage
        symbols, with conc = moles / volume by the engine's arrays"""
        eng, pop, amb = self.engine, self.population, self.ambient
        if self._stage is None:
            cells = lambda n: [eng.empty(self.n_cell, FLOAT) for _ in range(n)]  # noqa: E731
            rows = lambda n: [eng.empty(self.n_sd, FLOAT) for _ in range(n)]  # noqa: E731
            self._stage = {"eq": cells(7), "kin": cells(4), "henry": cells(6), "conc": rows(5),
                           "df": rows(6), "count": eng.zeros(1, INT), "count2": eng.zeros(1, INT),
                           "cfg": ChemistryCfg.from_buffer_copy(self.cfg)}
        st = self._stage
        st["cfg"].timestep = self.dt / self.setup.n_substep
        idx, cell_start = self._index()
        volume = self.volume()
        call = eng.call_chemistry
        call("sdm_chem_recalculate_cell_data", self.n_cell, amb.T, st["eq"], st["kin"],
             st["henry"], self.consts)
        gas_moles = [self.moles(k) for k in GAS_KEYS]
        for _ in range(self.setup.n_substep):
            for half in range(2):
                for out, key in zip(st["conc"], CONC):
                    eng.assign(out, self.moles(key) / volume)
                call("sdm_equilibrate_H", self.cfg, self.n_sd, pop.cell_id, st["conc"], st["eq"],
                     self.pH, self.do_chemistry_flag, st["count"], self.consts)
                self.counts[0:1] += st["count"]
                call("sdm_chem_recalculate_drop_data", self.n_sd, self.pH, pop.cell_id, st["eq"],
                     st["df"], self.consts)
                if half == 0:
                    call("sdm_dissolution", st["cfg"], self.n_sd, self.n_cell, idx, cell_start,
                         self.do_chemistry_flag, gas_moles, self.mixing_ratios, amb.T, amb.p,
                         amb.rhod, st["henry"], st["df"], volume, pop.multiplicity, st["count"],
                         st["count2"], self.consts)
                    self.counts[1:2] += st["count"]
                    self.counts[2:3] += st["count2"]
                else:
                    call("sdm_oxidation", self.n_sd, pop.cell_id, self.do_chemistry_flag,
                         st["kin"], st["eq"], st["cfg"].timestep, volume, self.pH,
                         st["df"][GASES.index("SO2")], self.moles("O3"), self.moles("H2O2"),
                         self.moles("S_IV"), self.moles("S_VI"), self.consts)

    def run(self, n_steps):
        for _ in range(int(n_steps)):
            self.step()

    def check(self):
        """raises if, in any step so far, one of the reference's assertions would have fired"""
        raise_if_counted(np.asarray(self.engine.download(self.counts)))

    def snapshot(self):
        """host copies: the seven mole columns, pH, the flag and the six mixing ratios"""
        self.check()
        down = self.engine.download
        return {"moles": np.stack([down(c) for c in self._columns()]), "pH": down(self.pH),
                "flag": down(self.do_chemistry_flag).astype(bool),
                "mixing_ratio": np.stack([down(c) for c in self.mixing_ratios])}

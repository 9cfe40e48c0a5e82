"""Relaxed fall velocity on the library (include/sdm_relaxed_velocity.h).

`RelaxedVelocityRunner` is PySDM's `RelaxedVelocity` dynamic (PySDM/dynamics/relaxed_velocity.py)
over a `Population` that carries the extensive row "relative fall momentum" and takes its fall
velocity from it (`Population(..., velocity_source="momentum")`): per step the momentum of every
slot is relaxed towards terminal velocity x water mass with the time scale `tau = c` (`constant`)
or `c * sqrt(radius)`,

    momentum += (terminal velocity * water mass - momentum) * (1 - exp(-dt / tau)),

and "relative fall velocity" - what the gravitational collision kernels, the Straub and Low-List
efficiencies and the sedimentation of the displacement read - is momentum / water mass
(PySDM/attributes/physics/relative_fall_velocity.py).

Routes: "fused" - one `sdm_relaxed_velocity_step` per step, which also leaves the new velocity
column in the population's cache - and "stages" - the reference's sequence of Storage operations,
one `sdm_elementwise_f64` each, over the attribute derivations water mass -> volume -> radius ->
square root of radius / terminal velocity; that one runs on any engine.  Same results to the bit.
Both work on all `n_sd` slots, as the reference does on whole columns.
"""
import numpy as np

from . import abi
from .engine import FLOAT, INT
from .physics import constants as const
from .population import MOMENTUM_ROW
from .terminal_velocity import LAWS, GunnKinzerTable, law_name

ROUTES = ("fused", "stages")
LAW_CODES = {"GunnKinzer1949": 0, "RogersYau": 1}
STATUS_ABOVE_TOP, STATUS_WORDS = 0, 2
# SDM_EW_* of include/sdm_hip.h
_ADD, _SUB, _MUL, _DIV, _POW, _EXP, _ABS, _FILL = 0, 1, 2, 3, 4, 7, 8, 9


def _radius_of_water_mass(engine, out, water_mass, n, rho_w):
    """attributes/physics/volume.py + radius.py on a column of (unsigned) water masses"""
    engine.call("sdm_volume_of_water_mass", out, water_mass, n, rho_w)
    engine.call("sdm_elementwise_f64", _MUL, out, out, None, 1 / const.PI_4_3, n)
    engine.call("sdm_elementwise_f64", _POW, out, out, None, 1 / 3, n)


def init_fall_momenta(engine, water_mass, law="GunnKinzer1949", zero=False, rho_w=const.rho_w):
    """initial values of the "relative fall momentum" row (PySDM/initialisation/
    init_fall_momenta.py): terminal velocity x water mass, or zeros; a host array.  The radius
    goes through the library's derivation (volume x 1 / (4/3 pi), then the cube root), so what comes
    back is the momentum the first relaxation step would leave unchanged."""
    water_mass = np.ascontiguousarray(water_mass, dtype=float)
    if zero:
        return np.zeros_like(water_mass)
    name = law_name(law)
    law = LAWS[name](engine) if isinstance(law, str) else law
    n = int(water_mass.shape[0])
    mass = engine.upload(np.abs(water_mass))
    radius, velocity = engine.empty(n, FLOAT), engine.empty(n, FLOAT)
    _radius_of_water_mass(engine, radius, mass, n, rho_w)
    law.evaluate(engine, velocity, radius, n)
    engine.call("sdm_elementwise_f64", _MUL, velocity, velocity, mass, 0.0, n)
    return engine.download(velocity)


class RelaxedVelocityRunner:  # pylint: disable=too-many-instance-attributes
    """`RelaxedVelocity(c=c, constant=constant)` on `population` with the time step `dt`"""

    def __init__(self, population, *, c=8, constant=False, dt, terminal_velocity="GunnKinzer1949",
                 route="fused", formulae="LiquidSpheres"):
        if route not in ROUTES:
            raise ValueError(f"route={route!r}: one of {ROUTES}")
        if formulae != "LiquidSpheres":
            raise NotImplementedError(
                f"particle_shape_and_density={formulae!r}: the relaxed fall velocity is "
                "implemented for LiquidSpheres")
        if MOMENTUM_ROW not in population.rows or population.velocity_source != "momentum":
            raise ValueError(f"the population needs the extensive row {MOMENTUM_ROW!r} and "
                             "velocity_source='momentum'")
        name = law_name(terminal_velocity)
        if route == "fused" and name == "PowerSeries":
            raise NotImplementedError("terminal_velocity='PowerSeries' is not offered on the "
                                      "fused route of RelaxedVelocityRunner; use route='stages'")
        self.population, self.route = population, route
        self.c, self.constant, self.dt = float(c), bool(constant), float(dt)
        eng = self.engine = population.engine
        self.law_name = name
        self.law = (LAWS[name](eng) if isinstance(terminal_velocity, str) else terminal_velocity)
        self.n_steps = 0
        self._cfg = None
        self._status = eng.zeros(STATUS_WORDS, INT) if route == "fused" else None
        self._tmp = {}

    # ---- the reference's own pieces (PySDM calls them by these names) -----------------------------
    def calculate_tau(self, output, sqrt_radius):
        n = self.population.n_sd
        self.engine.call("sdm_elementwise_f64", _FILL, output, None, None, self.c, n)
        if not self.constant:
            self.engine.call("sdm_elementwise_f64", _MUL, output, output, sqrt_radius, 0.0, n)

    def calculate_scale_factor(self, output, tau):
        ew, n = self.engine.call, self.population.n_sd
        ew("sdm_elementwise_f64", _FILL, output, None, None, -self.dt, n)
        ew("sdm_elementwise_f64", _DIV, output, output, tau, 0.0, n)
        ew("sdm_elementwise_f64", _EXP, output, output, None, 0.0, n)
        ew("sdm_elementwise_f64", _MUL, output, output, None, -1.0, n)
        ew("sdm_elementwise_f64", _ADD, output, output, None, 1.0, n)

    # ---- running ------------------------------------------------------------------------------------
    def step(self):
        """one `RelaxedVelocity.__call__`"""
        if self.route == "fused":
            self._step_fused()
        else:
            self._step_stages()
        self.n_steps += 1

    __call__ = step

    def run(self, n_steps):
        for _ in range(int(n_steps)):
            self.step()

    def cfg(self):
        if self._cfg is None:
            pop = self.population
            cfg = abi.RelaxedVelocityCfg()
            cfg.n_sd, cfg.dt, cfg.c, cfg.constant = pop.n_sd, self.dt, self.c, int(self.constant)
            cfg.rho_w = pop.rho_w
            cfg.law = LAW_CODES[self.law_name]
            if isinstance(self.law, GunnKinzerTable):
                cfg.gk_table_len, cfg.gk_factor = self.law.length, float(self.law.factor)
                cfg.gk_top = float(self.law.maximum_radius)
            else:
                cfg.rogers_yau = (abi.c_f64 * 5)(*self.law.consts)
            self._cfg = cfg
        return self._cfg

    def _step_fused(self):
        pop, eng = self.population, self.engine
        table = isinstance(self.law, GunnKinzerTable)
        velocity = pop.derived_buffer("fall velocity")
        eng.relaxed_velocity_call(
            "sdm_relaxed_velocity_step", self.cfg(), pop.mass, pop.momentum, velocity,
            self.law.a if table else None, self.law.b if table else None, self._status)
        if table and int(eng.download(self._status)[STATUS_ABOVE_TOP]) != 0:
            # nothing was stored; the reference's error with the reference's numbers (`evaluate`
            # finds the largest radius and raises; the last line is for a count it does not confirm)
            self._radius(self._scratch("radius"))
            self.law.evaluate(eng, self._scratch("terminal"), self._scratch("radius"), pop.n_sd)
            raise ValueError(f"Radii can be interpolated up to {self.law.maximum_radius} m")
        pop.touch_state()
        pop.publish_derived("fall velocity")

    def _scratch(self, name):
        if name not in self._tmp:
            self._tmp[name] = self.engine.empty(self.population.n_sd, FLOAT)
        return self._tmp[name]

    def _radius(self, out):
        pop, n = self.population, self.population.n_sd
        mass = self._scratch("water mass")
        self.engine.call("sdm_elementwise_f64", _ABS, mass, pop.mass, None, 0.0, n)
        _radius_of_water_mass(self.engine, out, mass, n, pop.rho_w)
        return mass

    def _step_stages(self):
        pop, eng, n = self.population, self.engine, self.population.n_sd
        ew = eng.call
        radius, terminal = self._scratch("radius"), self._scratch("terminal")
        diff, tau, scale = self._scratch("diff"), self._scratch("tau"), self._scratch("scale")
        mass = self._radius(radius)
        self.law.evaluate(eng, terminal, radius, n)  # (the table: raises above its top)
        ew("sdm_elementwise_f64", _MUL, diff, terminal, mass, 0.0, n)
        ew("sdm_elementwise_f64", _SUB, diff, diff, pop.momentum, 0.0, n)
        sqrt_radius = None
        if not self.constant:
            sqrt_radius = self._scratch("sqrt radius")
            ew("sdm_elementwise_f64", _POW, sqrt_radius, radius, None, 0.5, n)
        self.calculate_tau(tau, sqrt_radius)
        self.calculate_scale_factor(scale, tau)
        ew("sdm_elementwise_f64", _MUL, diff, diff, scale, 0.0, n)
        ew("sdm_elementwise_f64", _ADD, pop.momentum, pop.momentum, diff, 0.0, n)
        pop.touch_state()


"""Plugging this package into an unmodified PySDM installation.

1. The backend.  PySDM picks its backend by object - `Builder(n_sd, backend=<instance>, ...)`
   (PySDM/builder.py:25-38) - insisting only that it is an instance of its own `BackendMethods`
   (PySDM/particulator.py:22).  `HIP` already carries every method, `Storage` and `Random` the
   front-end calls, with PySDM's names and signatures; what remains is the base class:

       from pysdm_amd.pysdm_plugin import install
       HIP = install()                       # also reachable as PySDM.backends.HIP afterwards
       builder = Builder(n_sd, backend=HIP(Formulae(...)), environment=Box(...))

   PySDM's own `Coalescence` / `Collision` / `Breakup` then run stage by stage on the device.

2. The fused step.  `fuse(dynamic)` wraps one of PySDM's collision dynamics so that, registered
   with PySDM's Builder in its place, each call is ONE `sdm_collision_step` on PySDM's own
   attribute arrays (no copies: the particle state is adopted where it lies):

       builder.add_dynamic(fuse(Coalescence(collision_kernel=Golovin(b=1.5e3))))

   The dynamic's parts are translated to this package's `CollisionSetup` by class name and
   parameters (`setup_from_pysdm`); counters (`collision_rate`, ...) stay attributes of the
   returned object, as PySDM's products expect.

3. Seeding.  `fuse(Seeding(...))` likewise: every injecting time step is ONE `sdm_seeding_step`
   (shuffle of the seed index, injection, identity index, compaction) on PySDM's own arrays; the
   position in the random stream is the one PySDM's `Random` of the wrapped dynamic holds.

4. Relaxed fall velocity.  `fuse(RelaxedVelocity(...))` likewise: every call is ONE
   `sdm_relaxed_velocity_step` on PySDM's own "signed water mass" and "relative fall momentum"
   rows.  With `RelaxedVelocity` among the dynamics PySDM's "relative fall velocity" is momentum /
   water mass; `fuse(<collision dynamic>)` beside it reads the velocity from that row
   (sdm_step_cfg.velocity_source) where the engine's fused step can, and refuses where it cannot.

5. The fall-velocity law.  `fuse(<collision dynamic>)` evaluates the law of
   `Formulae(terminal_velocity=...)` (`velocity_law_from_pysdm`): the Gunn-Kinzer table,
   Rogers-Yau with the formulae's constants, or the default power series; an engine whose fused
   step lacks the law refuses by name.

6. Initialisation.  `equilibrate_wet_radii(**kwargs)` has the signature of
   PySDM.initialisation.equilibrate_wet_radii and returns an ndarray, so it replaces that import
   in a user's script (`from pysdm_amd.pysdm_plugin import equilibrate_wet_radii`); the search per
   super-droplet is ONE `sdm_equilibrate_wet_radii`, and `environment["T"]` / `environment["RH"]`
   are read where the backend's storages keep them.

PySDM itself is imported lazily: this module loads (and fails loudly) only where PySDM exists.
PySDM's ParticleAttributes keeps the permutation index, `cell_start`, the sorted flag and the
number of valid super-droplets as name-mangled members (PySDM/impl/particle_attributes.py:13-46);
that is how PySDM's `Particulator` itself reaches them (particulator.py:301-313) and how the
fused step hands the state back.
"""
import copy
import ctypes
import importlib
import warnings

import numpy as np

from . import abi
from . import initialisation as init
from . import recipe as R
from . import relaxed_velocity as relax
from . import seeding as seed
from .collisions import CollisionRunner
from .population import Population
from .terminal_velocity import PowerSeries, RogersYau

_PRIVATE = "_ParticleAttributes__"


def _pysdm_backend_methods():
    try:
        module = importlib.import_module("PySDM.backends.impl_common.backend_methods")
    except ImportError as error:
        raise ImportError("pysdm_amd.pysdm_plugin needs an importable PySDM") from error
    return module.BackendMethods


def as_pysdm_backend(backend_class):
    """`backend_class` (HIP; the tests pass its CPU-oracle twin) as a class PySDM's Particulator
    accepts"""
    base = _pysdm_backend_methods()
    if issubclass(backend_class, base):
        return backend_class

    def __init__(self, formulae=None, double_precision=True, **options):
        # next to PySDM the default formulae are PySDM's (numba.py:44: `formulae or Formulae()`):
        # its attributes build their physics from members this package's own, smaller Formulae
        # does not have (formulae.terminal_velocity_class, attributes/physics/terminal_velocity.py:19)
        if formulae is None:
            formulae = importlib.import_module("PySDM.formulae").Formulae()
        backend_class.__init__(self, formulae, double_precision, **options)

    return type(backend_class.__name__, (backend_class, base), {
        "__init__": __init__, "__doc__": backend_class.__doc__,
        "__module__": backend_class.__module__})


def install():
    """registers `PySDM.backends.HIP` next to CPU / GPU (PySDM/backends/__init__.py:75-83)"""
    from .backends.hip import HIP  # pylint: disable=import-outside-toplevel

    plugged = as_pysdm_backend(HIP)
    setattr(importlib.import_module("PySDM.backends"), "HIP", plugged)
    return plugged


# ---- PySDM's collision parts -> this package's recipe ---------------------------------------------
def _part(obj):
    """a PySDM kernel / efficiency / fragmentation object as the recipe part of the same name"""
    kind = type(obj).__name__
    limits = {"vmin": getattr(obj, "vmin", 0.0), "nfmax": getattr(obj, "nfmax", None)}
    table = {
        "Golovin": lambda: R.Golovin(b=obj.b),
        "Geometric": lambda: R.Geometric(collection_efficiency=obj.collection_efficiency),
        "ConstantK": lambda: R.ConstantK(a=obj.a),
        "Electric": R.Electric, "Hydrodynamic": R.Hydrodynamic,
        "SimpleGeometric": lambda: R.SimpleGeometric(C=obj.C),
        "ConstEc": lambda: R.ConstEc(Ec=obj.Ec), "ConstEb": lambda: R.ConstEb(Eb=obj.Eb),
        "Berry1967": R.Berry1967,
        "SpecifiedEff": lambda: R.SpecifiedEff(params=tuple(obj.params)),
        "Straub2010Ec": R.Straub2010Ec, "LowList1982Ec": R.LowList1982Ec,
        "AlwaysN": lambda: R.AlwaysN(n=obj.N), "ConstantMass": lambda: R.ConstantMass(c=obj.C),
        "Exponential": lambda: R.Exponential(scale=obj.scale, **limits),
        "Gaussian": lambda: R.Gaussian(mu=obj.mu, sigma=obj.sigma, **limits),
        "Feingold1988": lambda: R.Feingold1988(scale=obj.scale, fragtol=obj.fragtol, **limits),
        "SLAMS": lambda: R.SLAMS(**limits),
        "Straub2010Nf": lambda: R.Straub2010Nf(**limits),
        "LowList1982Nf": lambda: R.LowList1982Nf(**limits),
    }
    if kind not in table:
        raise NotImplementedError(f"{kind} has no device-side description; use PySDM's own "
                                  "dynamic with the plugged backend (stage-by-stage route)")
    return table[kind]()


def setup_from_pysdm(dynamic, formulae):
    """`CollisionSetup` equivalent of a PySDM `Collision` / `Coalescence` / `Breakup` object"""
    return R.CollisionSetup(
        kernel=_part(dynamic.collision_kernel),
        coalescence_efficiency=_part(dynamic.compute_coalescence_efficiency),
        breakup_efficiency=_part(dynamic.compute_breakup_efficiency),
        fragmentation=_part(dynamic.compute_number_of_fragments),
        breakup=bool(dynamic.enable_breakup), adaptive=bool(dynamic.adaptive),
        substeps=int(getattr(dynamic, "_Collision__substeps", 1)), dt_range=tuple(dynamic.dt_coal_range),
        croupier=dynamic.croupier or "local", optimized_random=bool(dynamic.optimized_random),
        warn_overflows=bool(dynamic.warn_overflows),
        handle_all_breakups=bool(formulae.handle_all_breakups), seed=int(formulae.seed),
        max_multiplicity=int(dynamic.max_multiplicity))


def velocity_law_from_pysdm(formulae):
    """`formulae.terminal_velocity` as this package's law: the name of the table (built per
    engine), Rogers-Yau with `formulae.constants`, or the power series with the default
    coefficients, which is what `formulae.terminal_velocity_class(particulator)` builds"""
    # (PySDM: the physics module of that name; this package's Formulae: the name; a formulae
    # object that names no law has the default of both)
    law = getattr(formulae, "terminal_velocity", "GunnKinzer1949")
    name = law if isinstance(law, str) else getattr(law, "__name__", type(law).__name__)
    if name == "GunnKinzer1949":
        return name
    if name == "RogersYau":
        return RogersYau(constants=formulae.constants)
    if name == "PowerSeries":
        return PowerSeries()
    raise NotImplementedError(f"terminal_velocity={name!r} has no counterpart in this package")


class _AdoptedState:
    """PySDM's ParticleAttributes seen as a Population (arrays shared, bookkeeping copied in
    before and back after every fused call)"""

    def __init__(self, particulator, velocity_source="terminal"):
        self.attributes = attrs = particulator.attributes
        self.idx = getattr(attrs, _PRIVATE + "idx")
        self.caretaker = getattr(attrs, _PRIVATE + "cell_caretaker")
        keys = list(attrs.get_extensive_attribute_keys())
        self.population = Population.adopt(
            particulator.backend.engine, perm=self.idx.data, perm_spare=self.caretaker.tmp_idx.data,
            multiplicity=attrs["multiplicity"].data,
            extensive=attrs.get_extensive_attribute_storage().data,
            rows={name: row for row, name in enumerate(keys)}, cell_id=attrs["cell id"].data,
            cell_order=attrs.cell_idx.data, cell_start=getattr(attrs, _PRIVATE + "cell_start").data,
            live=getattr(attrs, _PRIVATE + "valid_n_sd"), ordered=getattr(attrs, _PRIVATE + "sorted"),
            rho_w=particulator.formulae.constants.rho_w, velocity_source=velocity_source)
        self.stamps = None

    def _stamps(self):
        members = getattr(self.attributes, _PRIVATE + "attributes")
        names = ["multiplicity", "cell id"] + list(self.attributes.get_extensive_attribute_keys())
        return tuple(members[name].timestamp for name in names)

    def before(self):
        attrs, pop = self.attributes, self.population
        attrs.sanitize()
        stamps = self._stamps()
        if stamps != self.stamps:  # someone else touched the state since the last fused call
            pop.perm, pop.perm_spare = self.idx.data, self.caretaker.tmp_idx.data
            pop.live = pop.working = len(self.idx)
            pop.ordered = bool(getattr(attrs, _PRIVATE + "sorted"))
            if self.stamps is None or stamps[0] != self.stamps[0] or stamps[2:] != self.stamps[2:]:
                pop.touch_state()
            pop.host_dirty = True

    def after(self):
        attrs, pop = self.attributes, self.population
        self.idx.data, self.caretaker.tmp_idx.data = pop.perm, pop.perm_spare
        setattr(attrs, _PRIVATE + "valid_n_sd", int(pop.live))
        self.idx.length = self.idx.INT(int(pop.live))
        setattr(attrs, _PRIVATE + "sorted", bool(pop.ordered))
        attrs.mark_updated("multiplicity")
        for key in attrs.get_extensive_attribute_keys():
            attrs.mark_updated(key)
        self.stamps = self._stamps()


class Collision:  # pylint: disable=too-few-public-methods
    """root class: PySDM's Builder files a dynamic under the name of the class right below
    `object` in its MRO (builder.py:55) - the fused dynamic takes PySDM's "Collision" slot"""


class FusedCollision(Collision):
    """a PySDM dynamic (register / instantiate / __call__ protocol of PySDM's Builder) running
    the wrapped PySDM collision dynamic's configuration as the fused step"""

    _OWN = ("inner", "particulator", "runner", "_state")

    def __init__(self, dynamic):
        self.inner = dynamic
        self.particulator = None
        self.runner = None
        self._state = None

    def __setattr__(self, name, value):
        # options belong to the wrapped dynamic: PySDM's SpinUp observer switches collisions off
        # with setattr(particulator.dynamics["Collision"], "enable", False)
        # (examples/PySDM_examples/Arabas_et_al_2015/spin_up.py), and that lands here
        if name in self._OWN or "inner" not in self.__dict__:
            object.__setattr__(self, name, value)
        else:
            setattr(self.__dict__["inner"], name, value)

    def register(self, builder):
        self.particulator = builder.particulator
        self.inner.register(builder)  # requests the attributes the parts need

    def instantiate(self, *, builder):
        own = copy.copy(self)
        own.inner = copy.deepcopy(self.inner)
        own.register(builder)
        return own

    def __getattr__(self, name):
        # diagnostics live on the runner once it exists; options on the wrapped dynamic
        if name.startswith("__") or "inner" not in self.__dict__:
            raise AttributeError(name)
        runner = self.__dict__.get("runner")
        if runner is not None and name in ("collision_rate", "collision_rate_deficit",
                                           "coalescence_rate", "breakup_rate",
                                           "breakup_rate_deficit", "stats_n_substep",
                                           "stats_dt_min"):
            storage = self.particulator.backend.Storage
            array = getattr(runner, name)
            return storage(array, tuple(array.shape), storage.INT if "dt_min" not in name
                           else storage.FLOAT)
        return getattr(self.__dict__["inner"], name)

    def __call__(self):
        if not self.inner.enable:  # collision.py:175
            return
        part = self.particulator
        if self.runner is None:
            # with RelaxedVelocity among the dynamics "relative fall velocity" is momentum / water
            # mass (relative_fall_velocity.py:14,27): the step reads it from the extensive row
            relaxed = "RelaxedVelocity" in getattr(part, "dynamics", ())
            if relaxed and not part.backend.engine.fused_momentum_velocity:
                # a fused step that derives the velocity from the radius would run and differ
                raise NotImplementedError(
                    "fuse(<collision dynamic>) beside RelaxedVelocity: the fused collision step "
                    f"of engine `{part.backend.engine.name}` cannot take the fall velocity from "
                    "the relative fall momentum; register PySDM's own dynamic instead")
            velocity = "momentum" if relaxed else "terminal"
            self._state = _AdoptedState(part, velocity_source=velocity)
            setup = setup_from_pysdm(self.inner, part.formulae)
            self.runner = CollisionRunner(self._state.population, setup, dt=part.dt,
                                          dv=part.mesh.dv, route="fused",
                                          constants=part.formulae.constants, velocity=velocity,
                                          terminal_velocity=velocity_law_from_pysdm(
                                              part.formulae))
        self._state.before()
        self.runner.run(1)
        self._state.after()


class Seeding:  # pylint: disable=too-few-public-methods
    """root class: the fused dynamic takes PySDM's "Seeding" slot (see `Collision`)"""


class FusedSeeding(Seeding):
    """PySDM's `Seeding` dynamic (dynamics/seeding.py) with `Particulator.seeding`
    (particulator.py:447-499) as one `sdm_seeding_step` per injecting time step.  As in PySDM a
    seed is not placed in space: the slot keeps its cell id and position."""

    def __init__(self, dynamic):
        self.inner = dynamic
        self.particulator = None

    def register(self, builder):
        self.particulator = builder.particulator
        self.inner.register(builder)

    def instantiate(self, *, builder):
        own = copy.copy(self)
        own.inner = copy.copy(self.inner)
        own.register(builder)
        return own

    def __getattr__(self, name):
        if name.startswith("__") or "inner" not in self.__dict__:
            raise AttributeError(name)
        return getattr(self.__dict__["inner"], name)

    def __call__(self):
        part, inner = self.particulator, self.inner
        if part.n_steps == 0:
            inner.post_register_setup_when_attributes_are_known()
        number = inner.super_droplet_injection_rate(part.n_steps * part.dt)
        if not number > 0:  # seeding.py:77: no shuffle, no random number
            return
        number = int(number)
        n_seeds = len(inner.seeded_particle_multiplicity)
        assert number <= n_seeds
        attrs = part.attributes
        seed.check_counts(part.n_sd, attrs.super_droplet_count, n_seeds, number)
        idx = getattr(attrs, _PRIVATE + "idx")
        rows = attrs.get_extensive_attribute_storage().data
        rnd = inner.rnd  # this package's Random: the stream and the position in it
        new_length = ctypes.c_int64(-1)
        try:
            part.backend.engine.seeding_call(
                "sdm_seeding_step", idx.data, attrs["multiplicity"].data, rows,
                int(rows.shape[0]), int(part.n_sd), inner.index.data,
                inner.seeded_particle_multiplicity.data,
                inner.seeded_particle_extensive_attributes.data, n_seeds, number,
                int(rnd is not None), rnd.state_inc if rnd is not None else (0, 0, 0, 0),
                rnd.offset if rnd is not None else 0, new_length)
        except RuntimeError as error:
            # refused on the device (the count check above makes that a matter of broken
            # bookkeeping): the index was shuffled, so the numbers are spent, as on PySDM's own route
            if rnd is not None and seed.shuffled_before_failing(error):
                rnd.offset += n_seeds
            raise
        if rnd is not None:
            rnd.offset += n_seeds
        # what reset_idx() and sanitize() leave behind (particle_attributes.py:67-73,122-125)
        live = int(new_length.value)
        setattr(attrs, _PRIVATE + "valid_n_sd", live)
        idx.length = idx.INT(live)
        attrs.healthy = True
        setattr(attrs, _PRIVATE + "sorted", False)
        attrs.mark_updated("multiplicity")
        for key in attrs.get_extensive_attribute_keys():
            attrs.mark_updated(key)


class RelaxedVelocity:  # pylint: disable=too-few-public-methods
    """root class: the fused dynamic takes PySDM's "RelaxedVelocity" slot (see `Collision`),
    which is what PySDM's attribute variants look for (relative_fall_velocity.py:14,27)"""


class FusedRelaxedVelocity(RelaxedVelocity):
    """PySDM's `RelaxedVelocity` dynamic (dynamics/relaxed_velocity.py) as one
    `sdm_relaxed_velocity_step` per call on PySDM's own rows"""

    _OWN = ("inner", "particulator", "_cfg", "_table", "_status")

    def __init__(self, dynamic):
        self.inner = dynamic
        self.particulator = None
        self._cfg = self._table = self._status = None

    def __setattr__(self, name, value):
        # options (c, constant) belong to the wrapped dynamic
        if name in self._OWN or "inner" not in self.__dict__:
            object.__setattr__(self, name, value)
        else:
            setattr(self.__dict__["inner"], name, value)
            object.__setattr__(self, "_cfg", None)

    def register(self, builder):
        self.particulator = builder.particulator
        formulae = builder.particulator.formulae
        shape = getattr(formulae, "particle_shape_and_density", None)
        shape_name = shape if isinstance(shape, str) else getattr(
            shape, "__name__", type(shape).__name__)
        if shape_name != "LiquidSpheres":
            raise NotImplementedError(f"fuse(RelaxedVelocity): particle_shape_and_density="
                                      f"{shape_name!r}; implemented for 'LiquidSpheres'")
        if self._law_name() not in relax.LAW_CODES:
            raise NotImplementedError(
                f"fuse(RelaxedVelocity): terminal_velocity={self._law_name()!r} is not offered "
                "fused; register PySDM's own dynamic (stage-by-stage route)")
        self.inner.register(builder)

    def instantiate(self, *, builder):
        own = copy.copy(self)
        own.inner = copy.copy(self.inner)
        own.register(builder)
        return own

    def __getattr__(self, name):
        # calculate_tau / calculate_scale_factor and the options are the wrapped dynamic's
        if name.startswith("__") or "inner" not in self.__dict__:
            raise AttributeError(name)
        return getattr(self.__dict__["inner"], name)

    def _law_name(self):
        law = self.particulator.formulae.terminal_velocity
        return law if isinstance(law, str) else getattr(law, "__name__", type(law).__name__)

    def _config(self):
        part, inner = self.particulator, self.inner
        if self._cfg is None:
            cfg = abi.RelaxedVelocityCfg()
            cfg.n_sd, cfg.dt = int(part.n_sd), float(part.dt)
            cfg.c, cfg.constant = float(inner.c), int(bool(inner.constant))
            cfg.rho_w = part.formulae.constants.rho_w
            cfg.law = relax.LAW_CODES[self._law_name()]
            self._table = (None, None)
            if cfg.law == 0:
                table = inner.terminal_vel_attr.approximation
                cfg.gk_table_len, cfg.gk_factor = len(table.a), float(table.factor)
                cfg.gk_top = float(table.maximum_radius)
                self._table = (table.a.data, table.b.data)
            else:
                k = part.formulae.constants
                cfg.rogers_yau = (abi.c_f64 * 5)(
                    k.ROGERS_YAU_TERM_VEL_SMALL_K, k.ROGERS_YAU_TERM_VEL_MEDIUM_K,
                    k.ROGERS_YAU_TERM_VEL_LARGE_K, k.ROGERS_YAU_TERM_VEL_SMALL_R_LIMIT,
                    k.ROGERS_YAU_TERM_VEL_MEDIUM_R_LIMIT)
            self._cfg = cfg
        return self._cfg

    def __call__(self):
        part, inner = self.particulator, self.inner
        engine, attrs = part.backend.engine, part.attributes
        keys = list(attrs.get_extensive_attribute_keys())
        rows = attrs.get_extensive_attribute_storage().data
        cfg = self._config()
        if self._status is None:
            self._status = engine.zeros(relax.STATUS_WORDS, int)
        engine.relaxed_velocity_call(
            "sdm_relaxed_velocity_step", cfg, rows[keys.index("signed water mass")],
            rows[keys.index("relative fall momentum")], None, *self._table, self._status)
        if cfg.law == 0 and int(engine.download(self._status)[relax.STATUS_ABOVE_TOP]) != 0:
            # nothing was stored: PySDM's own error, raised by PySDM's own attribute
            inner.terminal_vel_attr.get()
            raise ValueError(f"Radii can be interpolated up to {cfg.gk_top} m")
        attrs.mark_updated("relative fall momentum")


def equilibrate_wet_radii(*, r_dry, environment, kappa_times_dry_volume, f_org=None,
                          cell_id=None, rtol=init.DEFAULT_RTOL, max_iters=init.DEFAULT_MAX_ITERS):
    """PySDM/initialisation/equilibrate_wet_radii.py:16-25 on the library: same keywords, an
    ndarray back.  `environment["T"]` and `environment["RH"]` are used as the storages of this
    package's backend that they are (no `to_ndarray`); storages of another backend are copied to
    the HIP engine.  Formulae and constants are `environment.particulator.formulae`'s.  Where the
    reference's closing assertion fires this raises pysdm_amd.initialisation.WetRadiusError, an
    AssertionError"""
    T, RH = environment["T"], environment["RH"]
    # (a Storage of this package's backend classes knows its engine: backends/storage.py)
    engine_getter = getattr(type(T), "engine_getter", None)
    if engine_getter is None:
        import torch  # pylint: disable=import-outside-toplevel

        from .engine import HipEngine  # pylint: disable=import-outside-toplevel

        if not torch.cuda.is_available():
            raise NotImplementedError(
                f"equilibrate_wet_radii: environment['T'] is a {type(T).__name__} of another "
                "backend and there is no GPU to copy it to; build the environment on "
                "PySDM.backends.HIP (pysdm_plugin.install()) or keep PySDM's own function")
        engine = HipEngine.get()
        T, RH = T.to_ndarray(), RH.to_ndarray()
    else:
        engine, T, RH = engine_getter(), T.data, RH.data
    r_wet = init.equilibrate_wet_radii(
        engine, environment.particulator.formulae, r_dry=np.asarray(r_dry, dtype=float),
        kappa_times_dry_volume=np.asarray(kappa_times_dry_volume, dtype=float), T=T, RH=RH,
        f_org=None if f_org is None else np.asarray(f_org, dtype=float),
        cell_id=None if cell_id is None else np.asarray(cell_id, dtype=np.int64),
        rtol=rtol, max_iters=max_iters)
    return engine.download(r_wet)


def fuse(dynamic):
    """`dynamic`: a PySDM Collision / Coalescence / Breakup instance, a PySDM Seeding or a PySDM
    RelaxedVelocity"""
    if type(dynamic).__name__ == "Seeding":
        return FusedSeeding(dynamic)
    if type(dynamic).__name__ == "RelaxedVelocity":
        return FusedRelaxedVelocity(dynamic)
    return FusedCollision(dynamic)


# ---- the adiabatic parcel: whole ascents in one call -------------------------------------------------
_PARCEL_VARS = {"z": "z", "rhod": "rhod", "thd": "thd", "qv": "water_vapour_mixing_ratio",
                "T": "T", "p": "p", "RH": "RH"}


def _coalescence_asked_for(particulator, breakup=False):
    """whether the dynamics are AmbientThermodynamics, Condensation, Coalescence in that order;
    the same three in another order, a Breakup or a Collision are refused by name - unless
    `breakup`, which serves all three kinds"""
    names = list(particulator.dynamics)
    if "Collision" not in names:  # (PySDM files Collision, Coalescence and Breakup under it)
        return False
    kind = type(particulator.dynamics["Collision"]).__name__
    if isinstance(particulator.dynamics["Collision"], FusedCollision):
        kind = type(particulator.dynamics["Collision"].inner).__name__
    if kind != "Coalescence" and not (breakup and kind in ("Collision", "Breakup")):
        raise ValueError(f"run_parcel serves Coalescence as the third dynamic, not {kind} "
                         "(breakup stays on particulator.run unless asked for with breakup=True)")
    if sorted(names) != ["AmbientThermodynamics", "Collision", "Condensation"]:
        raise ValueError("run_parcel needs exactly the dynamics AmbientThermodynamics, "
                         f"Condensation and Coalescence, not {sorted(names)}")
    if names != ["AmbientThermodynamics", "Condensation", "Collision"]:
        raise ValueError("run_parcel with Coalescence needs the order AmbientThermodynamics, "
                         f"Condensation, Coalescence, not {names}")
    if isinstance(particulator.dynamics["Collision"], FusedCollision):
        raise ValueError("run_parcel with Coalescence takes PySDM's own dynamic, not "
                         "fuse(Coalescence)")
    if not particulator.dynamics["Collision"].enable:
        raise ValueError("run_parcel needs Coalescence(enable=True)")
    return True


def run_parcel(particulator, steps, products=(), breakup=False):
    """`steps` time steps of a built `Particulator` whose environment is a `Parcel` and whose
    dynamics are exactly `AmbientThermodynamics` and `Condensation`, in ONE `sdm_parcel_run` on the
    particulator's own arrays (include/sdm_parcel.h; anything else: ValueError).  It leaves the
    particulator as `particulator.run(steps)` would: the water masses (marked updated), the
    environment's current values and the previous ones that `sync_parcel_vars` reads next, the
    dynamic's counters, `rh_max` and `success`, and `n_steps`.

    It also serves the dynamics `AmbientThermodynamics`, `Condensation`, `AqueousChemistry`,
    registered in that order (`sdm_parcel_run_chem`, include/sdm_parcel_chem.h): the `moles_*`
    attributes are marked updated (their dependants `conc_*`, `pH`, `dry volume` and `kappa`
    follow), the dynamic's `do_chemistry_flag` is the particulator's own and its
    `environment_mixing_ratios` are written back; what the reference asserts on (a pH solve that
    does not converge, a negative amount, a gas taken beyond what the parcel holds) raises
    afterwards.  Any other set of dynamics is refused.

    Formulae with a ventilation other than Neglect go to `sdm_parcel_run_vent`
    (include/sdm_parcel_vent.h) with the law of `velocity_law_from_pysdm`; the environment's
    current "air density" and "air dynamic viscosity" are the carried pair, read and left as
    `Moist.sync` leaves them.  Not with AqueousChemistry.

    And `AmbientThermodynamics`, `Condensation`, `Coalescence`, registered in that order
    (`sdm_parcel_run_coal`, include/sdm_parcel_coal.h; PySDM files the third under "Collision"):
    the dynamic is mapped by `setup_from_pysdm`, the law by `velocity_law_from_pysdm`; the
    particulator's own permutation (any order, sanitized first), multiplicities, extensive
    attributes (exactly "signed water mass", "dry volume", "kappa times dry volume"), the
    dynamic's counters, `stats_*` and the position of its random stream are read and left as
    `particulator.run(steps)` leaves them; the warnings of `Collision` are issued afterwards.  Any
    other order, a `Breakup` or a `Collision` are refused by name; no `products` with it.

    With `breakup=True` the third dynamic may also be `Collision` or `Breakup`
    (`sdm_parcel_run_collision`, include/sdm_parcel_breakup.h): the dynamic's `breakup_rate` and
    `breakup_rate_deficit` and the positions of its `rnd_opt_proc` and `rnd_opt_frag` streams (one
    position: the two generators share seed and position) are read and left as
    `particulator.run(steps)` leaves them too, and "overflow" is warned about as `Collision` does.

    Observers and PySDM's own product objects are NOT notified per step.  `products` (objects of
    pysdm_amd.products, which carry PySDM's names, arguments and units) are evaluated inside the
    kernel's step loop after every step (`sdm_parcel_run_diag`, include/sdm_parcel_diag.h).
    Returns the profile (host arrays of `steps` values by the names of sdm_parcel_profile), or with
    `products` {product name: array of `steps` values (x bins)}"""
    from . import parcel as _parcel  # pylint: disable=import-outside-toplevel
    from .condensation import CondensationSetup, check_formulae  # pylint: disable=import-outside-toplevel
    from .engine import FLOAT, INT  # pylint: disable=import-outside-toplevel

    env = particulator.environment
    if type(env).__name__ != "Parcel":
        raise ValueError(f"run_parcel needs a Parcel environment, not {type(env).__name__}")
    with_chem = list(particulator.dynamics) == ["AmbientThermodynamics", "Condensation",
                                                "AqueousChemistry"]
    with_coal = _coalescence_asked_for(particulator, breakup)
    if with_coal and len(products):
        raise NotImplementedError("run_parcel with Coalescence: products at output times come "
                                  "from the particulator's own products after the call")
    if not with_chem and not with_coal and sorted(particulator.dynamics) != [
            "AmbientThermodynamics", "Condensation"]:
        raise ValueError("run_parcel needs exactly the dynamics AmbientThermodynamics and "
                         f"Condensation, not {sorted(particulator.dynamics)}")
    if "a_w_ice" in env.variables:
        raise ValueError("run_parcel: mixed_phase=True is not served")
    dynamic = particulator.dynamics["Condensation"]
    if not dynamic.enable or not dynamic.update_thd:
        raise ValueError("run_parcel needs Condensation(enable=True, update_thd=True)")
    steps = int(steps)
    if steps <= 0:
        return None
    formulae, eng = particulator.formulae, particulator.backend.engine
    _parcel.check_hydrostatics(formulae)
    descriptor = check_formulae(formulae)
    ventilated = descriptor.option[_parcel._VENT] != 0  # pylint: disable=protected-access
    if ventilated and with_coal:
        raise ValueError("run_parcel: Coalescence with a ventilation other than Neglect stays on "
                         "particulator.run")
    if ventilated and with_chem:
        raise ValueError("run_parcel: AqueousChemistry with a ventilation other than Neglect "
                         "stays on particulator.run")
    setup = CondensationSetup(
        rtol_x=dynamic.rtol_x, rtol_thd=dynamic.rtol_thd,
        dt_cond_range=tuple(dynamic.dt_cond_range), adaptive=bool(dynamic.adaptive),
        substeps=1, max_iters=int(dynamic.max_iters)) if dynamic.adaptive else CondensationSetup(
            rtol_x=dynamic.rtol_x, rtol_thd=dynamic.rtol_thd,
            dt_cond_range=tuple(dynamic.dt_cond_range), adaptive=False,
            substeps=int(getattr(dynamic, "_Condensation__substeps", 1)),
            max_iters=int(dynamic.max_iters))
    dt = float(particulator.dt)
    cfg = _parcel.parcel_cfg(formulae, setup, dt)

    attrs = particulator.attributes
    idx = getattr(attrs, _PRIVATE + "idx")
    if with_coal:
        attrs.sanitize()
    n_sd = int(len(idx))
    if with_coal:  # any permutation of the live super-droplets; the columns keep their length
        n_live, n_sd = n_sd, int(particulator.n_sd)
    elif n_sd != int(particulator.n_sd) or not np.array_equal(
            eng.download(idx.data)[:n_sd], np.arange(n_sd)):
        raise ValueError("run_parcel needs every super-droplet valid and in row order")
    current, tmp = env._values["current"], env._tmp  # pylint: disable=protected-access
    before = {name: float(eng.download(current[var].data)[0])
              for name, var in _PARCEL_VARS.items()}
    qv_prev_before = float(eng.download(tmp["water_vapour_mixing_ratio"].data)[0])
    state = {name: current[var].data for name, var in _PARCEL_VARS.items()}
    state["qv_prev"] = tmp["water_vapour_mixing_ratio"].data
    state["mass_of_dry_air"] = eng.upload(np.array([env.mass_of_dry_air], dtype=float))
    for name in ("n_substeps", "n_activating", "n_deactivating", "n_ripening"):
        state[name] = dynamic.counters[name].data
    state["RH_max"] = dynamic.rh_max.data
    state["steps_done"] = eng.zeros(1, INT)
    state["failed_step"] = eng.full(1, INT, -1)
    w_mid = np.array([float(env.w((particulator.n_steps + k + 1 / 2) * dt))
                      for k in range(steps)])
    if not np.isfinite(w_mid).all() or (w_mid == 0).any():
        raise ValueError("run_parcel: the updraft must be finite and non-zero at every step's "
                         "mid-point")
    record = {name: eng.full(steps, FLOAT, np.nan) for name in _PARCEL_VARS}
    table = diag = None
    if len(products):
        from .products import RequestTable  # pylint: disable=import-outside-toplevel

        if eng.parcel_diag_library is None:
            raise NotImplementedError(f"engine `{eng.name}` has no parcel-diagnostics library")
        table = RequestTable(products, formulae)
        diag = {name: eng.full(steps * size, FLOAT, np.nan) for name, size in
                (("moment_0", table.n_moments), ("moments", table.n_moments),
                 ("spectrum", table.n_bins), ("dv", 1)) if size > 0}
    chem_call = None
    if with_chem:
        from . import chemistry as _chem  # pylint: disable=import-outside-toplevel

        aqueous = particulator.dynamics["AqueousChemistry"]
        if eng.parcel_chem_library is None:
            raise NotImplementedError(
                f"engine `{eng.name}` has no library for the parcel with aqueous chemistry")
        if descriptor.option[_parcel._SGM] != 0:  # pylint: disable=protected-access
            raise ValueError("run_parcel with AqueousChemistry needs the Constant surface tension")
        chem_setup = _chem.ChemistrySetup(
            aqueous.system_type, aqueous.n_substep,
            ionic_strength_threshold=aqueous.ionic_strength_threshold,
            pH_H_min=aqueous.pH_H_min, pH_H_max=aqueous.pH_H_max, pH_rtol=aqueous.pH_rtol)
        # (the pH attribute's own storage, not its getter: reading it would run a solve)
        acidity = getattr(attrs, _PRIVATE + "attributes")["pH"]
        ratios = [eng.upload(np.ascontiguousarray(aqueous.environment_mixing_ratios[gas],
                                                  dtype=float).reshape(1))
                  for gas in _chem.GASES]
        chem_counters = [eng.zeros(1, INT) for _ in range(3)]
        chem_call = {
            "cfg": chem_setup.cfg(formulae, dt, 0.0),
            "kappa_times_dry_volume": attrs["kappa times dry volume"].data,
            "moles": [attrs[f"moles_{key}"].data for key in _chem.AQUEOUS],
            "pH": acidity.data.data, "do_chemistry_flag": aqueous.do_chemistry_flag.data,
            "mixing_ratios": ratios, "consts": _chem.constants_of(formulae),
            "dry_factor": float(aqueous.dry_molar_mass) / float(aqueous.dry_rho),
            "counters": chem_counters, "profile": None}
    coal_call = None
    if with_coal:  # include/sdm_parcel_coal.h: the particulator's own arrays
        collision = particulator.dynamics["Collision"]
        coal_setup = setup_from_pysdm(collision, formulae)
        _parcel.check_collisions(coal_setup, [n_sd], breakup)
        if eng.parcel_coal_library is None:
            raise NotImplementedError(
                f"engine `{eng.name}` has no library for the parcel with coalescence")
        if breakup and eng.parcel_breakup_library is None:
            raise NotImplementedError(
                f"engine `{eng.name}` has no library for the parcel with breakup")
        keys = list(attrs.get_extensive_attribute_keys())
        wanted = ["signed water mass", "dry volume", "kappa times dry volume"]
        if sorted(keys) != sorted(wanted):
            raise ValueError(f"run_parcel with Coalescence needs exactly the extensive attributes "
                             f"{wanted}, not {keys}")
        stream = collision.rnd_opt_coll.rnd
        if not hasattr(stream, "state_inc") or not hasattr(stream, "offset"):
            raise NotImplementedError("run_parcel with Coalescence needs the random stream of a "
                                      "backend of this package")
        coal_cfg, coal_law, coal_dt_range = _parcel.collision_cfg(
            eng, coal_setup, dt, float(formulae.constants.rho_w),
            velocity_law_from_pysdm(formulae))
        live_count = eng.upload(np.array([n_live], dtype=np.int64))
        coal_events = eng.zeros(1, INT)
        stream_offset = eng.upload(np.array([stream.offset], dtype=np.int64))
        words = np.array(stream.state_inc, dtype=np.uint64)
        coal_call = {
            "cfg": coal_cfg, "idx": idx.data, "n_live": live_count,
            "kappa_times_dry_volume": attrs["kappa times dry volume"].data,
            "collision_rate": collision.collision_rate.data,
            "collision_rate_deficit": collision.collision_rate_deficit.data,
            "coalescence_rate": collision.coalescence_rate.data,
            "stats_n_substep": collision.stats_n_substep.data,
            "stats_dt_min": collision.stats_dt_min.data, "events": coal_events,
            "rng_offset": stream_offset,
            "rng_state_inc": eng.upload(words.view(np.int64).copy()),
            **{name: (coal_law or {}).get(name) for name in ("gk_a", "gk_b", "velocity_params")},
            "fresh_idx": True, "profile": None}
        if breakup and coal_setup.breakup:  # include/sdm_parcel_breakup.h
            streams_b = (collision.rnd_opt_proc.rnd, collision.rnd_opt_frag.rnd)
            if any(not hasattr(s, "state_inc") or not hasattr(s, "offset") for s in streams_b):
                raise NotImplementedError("run_parcel with breakup needs the random streams of a "
                                          "backend of this package")
            if (streams_b[0].offset != streams_b[1].offset
                    or any(tuple(s.state_inc) != tuple(stream.state_inc) for s in streams_b)):
                raise ValueError("run_parcel with breakup: the streams of rnd_opt_proc and "
                                 "rnd_opt_frag must share seed and position")
            stream_offset_b = eng.upload(np.array([streams_b[0].offset], dtype=np.int64))
            coal_call["breakup"] = {"breakup_rate": collision.breakup_rate.data,
                                    "breakup_rate_deficit": collision.breakup_rate_deficit.data,
                                    "rng_offset_breakup": stream_offset_b, "profile": None}
        elif breakup:
            coal_call["breakup"] = {"profile": None}
            streams_b = ()
    vent = None
    if ventilated:  # include/sdm_parcel_vent.h: the law of the formulae, the environment's air
        from .terminal_velocity import make_law  # pylint: disable=import-outside-toplevel

        if eng.parcel_vent_library is None:
            raise NotImplementedError(
                f"engine `{eng.name}` has no library for the ventilated parcel")
        law = make_law(velocity_law_from_pysdm(formulae), eng, formulae.constants)
        out_of_table = eng.zeros(1, INT)
        vent = {**_parcel.vent_law(eng, law), "air_density": current["air density"].data,
                "air_dynamic_viscosity": current["air dynamic viscosity"].data,
                "reynolds_number": eng.empty(n_sd, FLOAT), "out_of_table": out_of_table}
    _parcel.parcel_call(
        eng, formulae, cfg, n_steps=steps, chem=chem_call, vent=vent, coal=coal_call,
        parcel_start=eng.upload(np.array([0, n_sd], dtype=np.int64)),
        water_mass=attrs["signed water mass"].data, multiplicity=attrs["multiplicity"].data,
        dry_volume=attrs["dry volume"].data, kappa=attrs["kappa"].data,
        f_org=attrs["dry volume organic fraction"].data,
        critical_volume=eng.empty(n_sd, FLOAT), state=state, w_mid=eng.upload(w_mid),
        profile=record, descriptor=descriptor,
        requests=None if table is None else table.c_struct(), diag=diag)
    attrs.mark_updated("signed water mass")
    if with_coal:  # what Collision.__call__ and sanitize() leave behind
        n_live = int(eng.download(live_count)[0])
        setattr(attrs, _PRIVATE + "valid_n_sd", n_live)
        idx.length = idx.INT(n_live)
        setattr(attrs, _PRIVATE + "sorted", False)
        attrs.mark_updated("multiplicity")
        for key in attrs.get_extensive_attribute_keys():
            attrs.mark_updated(key)
        stream.offset = int(eng.download(stream_offset)[0])
        for stream_b in (streams_b if breakup else ()):
            stream_b.offset = int(eng.download(stream_offset_b)[0])
        if collision.adaptive:
            eng.fill(collision.dt_left.data, 0.0)
    if with_chem:
        for key in _chem.AQUEOUS:
            attrs.mark_updated(f"moles_{key}")
        for gas, ratio in zip(_chem.GASES, ratios):
            aqueous.environment_mixing_ratios[gas][:] = eng.download(ratio)
        # the dynamic's per-cell constants as its last call left them (the temperature after the
        # last step): the `pH` attribute's next solve reads them
        particulator.backend.chem_recalculate_cell_data(
            equilibrium_consts=aqueous.equilibrium_consts, kinetic_consts=aqueous.kinetic_consts,
            temperature=current["T"])
    done = int(eng.download(state["steps_done"])[0])
    rows = {name: eng.download(array) for name, array in record.items()}
    # what notify() leaves behind: _tmp holds the values before the last step carried out
    if done > 0:
        previous = {name: (rows[name][done - 2] if done >= 2 else before[name])
                    for name in _PARCEL_VARS}
        for name, var in _PARCEL_VARS.items():
            eng.fill(tmp[var].data, float(previous[name]))
        before_previous = (rows["qv"][done - 3] if done >= 3
                           else before["qv"] if done == 2 else qv_prev_before)
        env.delta_liquid_water_mixing_ratio = before_previous - previous["qv"]
        env.mesh.dv = formulae.trivia.volume_of_density_mass(
            (rows["rhod"][done - 1] + previous["rhod"]) / 2, env.mass_of_dry_air)
        env._values["predicted"] = None  # pylint: disable=protected-access
        eng.fill(dynamic.success.data, True)
        particulator.n_steps += done
    if done < steps:
        if ventilated and int(eng.download(out_of_table)[0]):
            # (what the table's `evaluate` raises in particulator.run, before the dynamic ran)
            raise ValueError(f"Radii can be interpolated up to {law.maximum_radius} m: a radius "
                             f"above it stopped the parcel in step {done} of this call")
        eng.fill(dynamic.success.data, False)
        raise RuntimeError("Condensation failed")
    if with_chem:
        _chem.raise_if_counted([int(eng.download(c)[0]) for c in chem_counters])
    if with_coal:
        events = int(eng.download(coal_events)[0])
        if events & abi.PARCEL_COAL_EVENT_BOUND:
            raise RuntimeError("run_parcel with Coalescence: an adaptive time step did not end "
                               "within the bound its own arithmetic sets")
        if events & abi.PARCEL_COAL_EVENT_DT_MIN and float(
                eng.download(collision.stats_dt_min.data)[0]) == coal_dt_range[0]:
            warnings.warn("adaptive time-step reached dt_min")  # collision.py:276-277
        if events >> abi.PARCEL_COAL_OVERFLOW_SHIFT and coal_setup.warn_overflows:
            warnings.warn("overflow")  # (as the reference's backend does with warn_overflows)
    if table is None:
        return rows
    from .products import Rows  # pylint: disable=import-outside-toplevel

    def column(name, width):
        return eng.download(diag[name]).reshape(steps, width) if name in diag \
            else np.empty((steps, 0))

    return table.values(Rows(table, moment_0=column("moment_0", table.n_moments),
                             moments=column("moments", table.n_moments),
                             spectrum=column("spectrum", table.n_bins),
                             dv=eng.download(diag["dv"]), rhod=rows["rhod"]))

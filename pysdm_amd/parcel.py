"""The adiabatic parcel on the library (include/sdm_parcel.h): PySDM's `Parcel` environment with
the dynamics `AmbientThermodynamics` and `Condensation`, for an ensemble of independent parcels.

`ParcelRunner` holds the parcels' state (per parcel: z, rhod, thd, qv, T, p, RH, the previous qv,
the solver's counters; per super-droplet: water mass, multiplicity, dry volume, kappa, f_org and
the critical volume) as engine arrays and runs time steps on one of two routes:

* ``route="fused"``: `sdm_parcel_run` - one library call for `n_steps` steps of all parcels, the
  loop over the steps inside the kernel, nothing read back between the steps;
* ``route="stages"``: the same time step written with the symbols of include/sdm_condensation.h
  (and its `_f` forms): the advance of the parcel's variables in Python floats, then
  `sdm_critical_volume`, `sdm_condensation` and `sdm_temperature_pressure_rh`, per parcel on
  slices of the columns with n_cell = 1.  It is the yardstick of the fused route (the two agree
  bit for bit).

With a ventilation other than Neglect and ``terminal_velocity=`` (a name or a law object of
pysdm_amd.terminal_velocity) every droplet's Reynolds number is formed inside the step
(include/sdm_parcel_vent.h, where the step and the timing of the air density and viscosity it reads
are written out): the fused route calls `sdm_parcel_run_vent`, the stage route adds
`sdm_air_density`, `sdm_air_dynamic_viscosity`, the radius, the law's `evaluate` and
`sdm_reynolds_number`.  The parcels then carry `air_density`, `air_dynamic_viscosity` (state) and
the `reynolds_number` column.

The time step is the one include/sdm_parcel.h writes out (environments/parcel.py:101-153,
environments/impl/moist.py:73-100, dynamics/condensation.py:95-131), with the hydrostatics
ConstantGVapourMixingRatioAndThetaStd; the initial state follows `Parcel.register`
(parcel.py:51-71).  `run` returns the profile and, with `products=` (pysdm_amd/products.py), the
products of the state after every step: the fused route evaluates their request table inside the
kernel's step loop (`sdm_parcel_run_diag`, include/sdm_parcel_diag.h), the stage route with
`sdm_parcel_diagnose` after each step; `diagnose` gives the products of the current state.
"""
import ctypes
import warnings

import numpy as np

from . import abi
from . import chemistry as chem
from . import parcel_ice
from . import terminal_velocity as tv
from .condensation import (CONSTANT_NAMES, OPTION_ORDER, _option_name, check_formulae,
                           condensation_call, critical_volume_call, is_default,
                           temperature_pressure_rh_call)
from .engine import FLOAT, INT
from .products import RequestTable, Rows

HYDROSTATICS = "ConstantGVapourMixingRatioAndThetaStd"
G_STD = 9.80665  # PySDM/physics/constants_defaults.py: g_std (scipy.constants.g)
ROUTES = ("fused", "stages")
_INT_FIELDS = ("n_substeps", "n_activating", "n_deactivating", "n_ripening", "steps_done",
               "failed_step")
_LV = OPTION_ORDER.index("latent_heat_vapourisation")
_SGM = OPTION_ORDER.index("surface_tension")
_VENT = OPTION_ORDER.index("ventilation")
VENT_STATE = ("air_density", "air_dynamic_viscosity")  # what a ventilated parcel carries
CHEM_COUNTERS = ("n_failed", "n_negative", "n_exceeded")
COAL_COUNTERS = ("collision_rate", "collision_rate_deficit", "coalescence_rate")
BREAKUP_COUNTERS = ("breakup_rate", "breakup_rate_deficit")
_COAL_INTS = ("out_of_table", "multiplicity", "idx", "n_live", "stats_n_substep", "events",
              "rng_offset", "rng_offset_breakup") + BREAKUP_COUNTERS
_DIAG_LANES = 256  # the partials of the SUM of include/sdm_parcel_diag.h


def _address(array, dtype):
    """the address of a contiguous engine array of `dtype` (numpy array or torch tensor): what the
    members of ParcelState / ParcelProfile hold (the binding checks only direct arguments)"""
    if array is None:
        return None
    if isinstance(array, np.ndarray):
        if not array.flags["C_CONTIGUOUS"] or array.dtype.type is not dtype:
            raise TypeError(f"parcel: expected a contiguous {np.dtype(dtype).name} array")
        return array.ctypes.data
    if not array.is_contiguous() or str(array.dtype).rsplit(".", 1)[-1] != np.dtype(dtype).name:
        raise TypeError(f"parcel: expected a contiguous {np.dtype(dtype).name} array")
    return array.data_ptr()


def check_hydrostatics(formulae):
    """the parcel's density derivative is ConstantGVapourMixingRatioAndThetaStd.drho_dz (PySDM's
    default); a `Formulae` naming another hydrostatics is refused"""
    value = getattr(formulae, "hydrostatics", None)
    if value is not None and _option_name(value) != HYDROSTATICS:
        raise NotImplementedError(f"parcel supports hydrostatics={HYDROSTATICS!r} only, "
                                  f"not {_option_name(value)!r}")


def parcel_cfg(formulae, setup, dt, steps_per_launch=0):
    """abi.ParcelCfg of a CondensationSetup and a time step"""
    cfg = abi.ParcelCfg()
    cfg.dt = float(dt)
    cfg.g_std = float(getattr(formulae.constants, "g_std", G_STD))
    cfg.rtol_x, cfg.rtol_thd = float(setup.rtol_x), float(setup.rtol_thd)
    cfg.dt_min, cfg.dt_max = float(setup.dt_cond_range[0]), float(setup.dt_cond_range[1])
    cfg.RH_rtol = float(setup.RH_rtol)
    cfg.adaptive, cfg.fuse = int(bool(setup.adaptive)), int(setup.fuse)
    cfg.multiplier, cfg.max_iters = int(setup.multiplier), int(setup.max_iters)
    # dynamics/condensation.py:122-131
    cfg.n_clamp_lo = int(dt / setup.dt_cond_range[1])
    cfg.n_clamp_hi = int(dt / setup.dt_cond_range[0]) if setup.dt_cond_range[0] != 0 else 0
    cfg.steps_per_launch = int(steps_per_launch)
    return cfg


def parcel_call(engine, formulae, cfg, *, n_steps, parcel_start, water_mass, multiplicity,
                dry_volume, kappa, f_org, critical_volume, state, w_mid, profile=None,
                descriptor=None, general=False, requests=None, diag=None, chem=None, vent=None,
                coal=None):
    """one `sdm_parcel_run` call with raw engine arrays: `state` / `profile` are dicts of engine
    arrays by the member names of sdm_parcel_state / sdm_parcel_profile (`profile` may be None or
    lack members), `w_mid` an engine array of n_steps x n_parcel.  PySDM's default formulae go to
    the default kernel unless `general` (the two must agree bit for bit).  With `requests` (an
    abi.ParcelRequests) the call is `sdm_parcel_run_diag`, and `diag` a dict of engine arrays by
    the member names of sdm_parcel_diag (members may be missing).  With `chem` the call is
    `sdm_parcel_run_chem` (include/sdm_parcel_chem.h): a dict with `cfg` (abi.ChemistryCfg),
    `kappa_times_dry_volume`, `moles` (7 columns), `pH`, `do_chemistry_flag`, `mixing_ratios` (6
    arrays of n_parcel), `consts` (62), `dry_factor`, `counters` (3 arrays of n_parcel or None)
    and `profile` (None, or a dict with `mixing_ratio`: 6 arrays, `aq_total`: 7 arrays,
    `n_flagged`, `dv`, each of n_steps x n_parcel; entries may be missing).  With `vent` the call
    is `sdm_parcel_run_vent` (include/sdm_parcel_vent.h; with or without `requests`): a dict by
    the member names of sdm_parcel_vent - the law's part as `vent_law` builds it, and the engine
    arrays `air_density`, `air_dynamic_viscosity` (n_parcel each), `reynolds_number` (n_sd) and
    optionally `out_of_table` (n_parcel, int64); `descriptor` may then be one of
    `condensation.descriptor_of` naming a ventilation a `Formulae` refuses.  With `coal` the call
    is `sdm_parcel_run_coal` (include/sdm_parcel_coal.h): a dict with `cfg` (abi.StepCfg), the
    engine arrays of sdm_parcel_coal_state by their member names (`rng_offset` and
    `rng_state_inc` as int64 arrays holding the unsigned words; the fall-velocity members may be
    missing), `fresh_idx` (default True) and `profile` (None, or a dict by the member names of
    sdm_parcel_coal_profile; entries may be missing); `multiplicity`, `dry_volume` and `kappa`
    are then written.  With `coal["breakup"]` the call is `sdm_parcel_run_collision`
    (include/sdm_parcel_breakup.h): a dict of the engine arrays of sdm_parcel_breakup_state by
    their member names (`rng_offset_breakup` as an int64 array) and `profile` (None, or a dict
    by the member names of sdm_parcel_breakup_profile)"""
    if descriptor is None:
        descriptor = check_formulae(formulae)
    if vent is not None and chem is not None:
        raise NotImplementedError("parcel: chemistry with ventilation is not served")
    n_parcel = engine.size(parcel_start) - 1
    if engine.size(w_mid) != n_steps * n_parcel:
        raise ValueError("parcel: w_mid must hold n_steps x n_parcel values")
    c_state = abi.ParcelState()
    for name in abi.PARCEL_STATE_FIELDS:
        if engine.size(state[name]) != n_parcel:
            raise ValueError(f"parcel: state[{name!r}] must hold n_parcel values")
        setattr(c_state, name, _address(state[name], INT if name in _INT_FIELDS else FLOAT))
    c_profile = None
    if profile is not None:
        c_profile = abi.ParcelProfile()
        for name in abi.PARCEL_PROFILE_FIELDS:
            array = profile.get(name)
            if array is not None and engine.size(array) != n_steps * n_parcel:
                raise ValueError(f"parcel: profile[{name!r}] must hold n_steps x n_parcel values")
            setattr(c_profile, name,
                    _address(array, INT if name.startswith("n_") else FLOAT))
    consts = [float(getattr(formulae.constants, name)) for name in CONSTANT_NAMES]
    args = (cfg, int(n_steps), int(n_parcel), int(engine.size(water_mass)),
            parcel_start, water_mass, multiplicity, dry_volume, kappa, f_org, critical_volume,
            c_state, w_mid, c_profile, consts,
            None if is_default(descriptor) and not general else descriptor)
    if coal is not None:
        if requests is not None or chem is not None or vent is not None:
            raise NotImplementedError("parcel with coalescence: no request table, chemistry or "
                                      "ventilation in the same call")
        coal_args = (args[0], coal["cfg"], *args[1:],
                     _coal_state_struct(engine, coal, n_parcel, int(engine.size(water_mass))),
                     _coal_profile_struct(engine, coal.get("profile"), n_steps * n_parcel),
                     int(bool(coal.get("fresh_idx", True))))
        if coal.get("breakup") is None:
            engine.call_parcel_coal("sdm_parcel_run_coal", *coal_args)
        else:
            engine.call_parcel_breakup(
                "sdm_parcel_run_collision", *coal_args,
                *_breakup_structs(engine, coal["breakup"], n_parcel, n_steps * n_parcel))
        return
    if requests is None and chem is None and vent is None:
        engine.call_parcel("sdm_parcel_run", *args)
        return
    c_diag = None
    if requests is not None:
        sizes = {"moment_0": requests.n_moments, "moments": requests.n_moments,
                 "spectrum": requests.n_bins, "dv": 1}
        c_diag = _diag_struct(engine, diag, sizes, n_steps * n_parcel)
    if vent is not None:
        engine.call_parcel_vent(
            "sdm_parcel_run_vent", *args[:-1], descriptor, requests, c_diag,
            _vent_struct(engine, vent, n_parcel, int(engine.size(water_mass))))
        return
    if chem is None:
        engine.call_parcel_diag("sdm_parcel_run_diag", *args, requests, c_diag)
        return
    engine.call_parcel_chem(
        "sdm_parcel_run_chem", args[0], chem["cfg"], *args[1:], requests, c_diag,
        chem["kappa_times_dry_volume"], chem["moles"], chem["pH"], chem["do_chemistry_flag"],
        chem["mixing_ratios"], chem["consts"], float(chem["dry_factor"]),
        *(chem.get("counters") or (None, None, None)),
        _chem_profile_struct(engine, chem.get("profile"), n_steps * n_parcel))


def vent_law(engine, law):
    """the law's members of sdm_parcel_vent for a law object of pysdm_amd.terminal_velocity: a dict
    of scalars and engine arrays (to be kept alive by the caller for as long as calls use them)"""
    name = tv.law_name(law)
    out = {"velocity_law": abi.VELOCITY_LAWS[name], "velocity_terms": 0, "velocity_params": None,
           "gk_a": None, "gk_b": None, "gk_table_len": 0, "gk_factor": 0.0, "gk_top": 0.0}
    if name == "GunnKinzer1949":
        out.update(gk_a=law.a, gk_b=law.b, gk_table_len=int(law.length),
                   gk_factor=float(law.factor), gk_top=float(law.maximum_radius))
    elif name == "RogersYau":
        out["velocity_params"] = engine.upload(np.array(law.consts, dtype=float))
    else:
        if len(law.powers) > abi.VELOCITY_MAX_TERMS:
            raise ValueError(f"a power series of more than {abi.VELOCITY_MAX_TERMS} terms")
        out["velocity_terms"] = len(law.powers)
        out["velocity_params"] = engine.upload(np.concatenate(
            [np.asarray(law.prefactors, dtype=float), np.asarray(law.powers, dtype=float)]))
    return out


def _vent_struct(engine, vent, n_parcel, n_sd):
    """abi.ParcelVent of a dict by the member names of sdm_parcel_vent"""
    out = abi.ParcelVent()
    law = vent["velocity_law"]
    out.velocity_law = abi.VELOCITY_LAWS[law] if isinstance(law, str) else int(law)
    out.velocity_terms = int(vent.get("velocity_terms", 0))
    out.gk_table_len = int(vent.get("gk_table_len", 0))
    out.gk_factor, out.gk_top = float(vent.get("gk_factor", 0)), float(vent.get("gk_top", 0))
    # (the kernels index these by the counts above: too short an array would be read past its end)
    needs = {"velocity_params": {1: 5, 2: 2 * out.velocity_terms}.get(out.velocity_law, 0),
             "gk_a": out.gk_table_len, "gk_b": out.gk_table_len}
    for name in ("velocity_params", "gk_a", "gk_b"):
        array = vent.get(name)
        if array is not None and engine.size(array) < needs[name]:
            raise ValueError(f"parcel: vent[{name!r}] must hold {needs[name]} values")
        setattr(out, name, _address(array, FLOAT))
    for name, size, dtype in (("air_density", n_parcel, FLOAT),
                              ("air_dynamic_viscosity", n_parcel, FLOAT),
                              ("reynolds_number", n_sd, FLOAT), ("out_of_table", n_parcel, INT)):
        array = vent.get(name)
        if array is not None and engine.size(array) != size:
            raise ValueError(f"parcel: vent[{name!r}] must hold {size} values")
        setattr(out, name, _address(array, dtype))
    return out


def _chem_profile_struct(engine, profile, n_rows):
    """abi.ParcelChemProfile of a dict of engine arrays (None: no record)"""
    if profile is None:
        return None
    out = abi.ParcelChemProfile()

    def address(array, dtype):
        if array is not None and engine.size(array) != n_rows:
            raise ValueError(f"parcel: a chemistry profile member must hold {n_rows} values")
        return _address(array, dtype) or 0

    for g, array in enumerate(profile.get("mixing_ratio") or [None] * 6):
        out.mixing_ratio[g] = address(array, FLOAT)
    for a, array in enumerate(profile.get("aq_total") or [None] * 7):
        out.aq_total[a] = address(array, FLOAT)
    out.n_flagged = address(profile.get("n_flagged"), INT) or None
    out.dv = address(profile.get("dv"), FLOAT) or None
    return out


_COAL_FLOATS = ("kappa_times_dry_volume", "stats_dt_min", "gk_a", "gk_b", "velocity_params", "dv")


def _coal_state_struct(engine, coal, n_parcel, n_sd):
    """abi.ParcelCoalState of a dict of engine arrays by the member names"""
    out = abi.ParcelCoalState()
    sizes = {"idx": n_sd, "kappa_times_dry_volume": n_sd, "rng_state_inc": 4 * n_parcel}
    for name in abi.PARCEL_COAL_STATE_FIELDS:
        array = coal.get(name)
        if name in ("gk_a", "gk_b", "velocity_params"):  # (sized by the cfg's counts)
            setattr(out, name, _address(array, FLOAT))
            continue
        if array is None:
            raise ValueError(f"parcel: coal[{name!r}] is missing")
        if engine.size(array) != sizes.get(name, n_parcel):
            raise ValueError(f"parcel: coal[{name!r}] must hold {sizes.get(name, n_parcel)} "
                             "values")
        setattr(out, name, _address(array, FLOAT if name in _COAL_FLOATS else INT))
    return out


def _coal_profile_struct(engine, profile, n_rows):
    """abi.ParcelCoalProfile of a dict of engine arrays (None: no record)"""
    if profile is None:
        return None
    out = abi.ParcelCoalProfile()
    for name in abi.PARCEL_COAL_PROFILE_FIELDS:
        array = profile.get(name)
        if array is not None and engine.size(array) != n_rows:
            raise ValueError(f"parcel: a coalescence profile member must hold {n_rows} values")
        setattr(out, name, _address(array, FLOAT if name in _COAL_FLOATS else INT))
    return out


def _breakup_structs(engine, breakup, n_parcel, n_rows):
    """(abi.ParcelBreakupState, abi.ParcelBreakupProfile or None) of a dict of engine arrays by
    the member names, and `profile`"""
    state = abi.ParcelBreakupState()
    for name in abi.PARCEL_BREAKUP_STATE_FIELDS:
        array = breakup.get(name)
        if array is not None and engine.size(array) != n_parcel:
            raise ValueError(f"parcel: breakup[{name!r}] must hold {n_parcel} values")
        setattr(state, name, _address(array, INT))
    profile = breakup.get("profile")
    if profile is None:
        return state, None
    record = abi.ParcelBreakupProfile()
    for name in abi.PARCEL_BREAKUP_PROFILE_FIELDS:
        array = profile.get(name)
        if array is not None and engine.size(array) != n_rows:
            raise ValueError(f"parcel: a breakup profile member must hold {n_rows} values")
        setattr(record, name, _address(array, INT))
    return state, record


def diag_sum(multiplicity, values):
    """the SUM of include/sdm_parcel_diag.h of multiplicity * values on the host, add for add"""
    terms = np.asarray(multiplicity).astype(float) * np.asarray(values, dtype=float)
    padded = np.zeros(-(-max(terms.size, 1) // _DIAG_LANES) * _DIAG_LANES)
    padded[:terms.size] = terms  # (+0.0 added to a partial that started at +0.0 changes no bit)
    partial = np.zeros(_DIAG_LANES)
    for chunk in padded.reshape(-1, _DIAG_LANES):
        partial = partial + chunk
    stride = _DIAG_LANES // 2
    while stride >= 1:
        partial[:stride] = partial[:stride] + partial[stride:2 * stride]
        stride //= 2
    return float(partial[0])


def _diag_struct(engine, diag, sizes, n_rows):
    """abi.ParcelDiag of a dict of engine arrays (None: no outputs)"""
    if diag is None:
        return None
    c_diag = abi.ParcelDiag()
    for name in abi.PARCEL_DIAG_FIELDS:
        array = diag.get(name)
        if array is not None and engine.size(array) != n_rows * sizes[name]:
            raise ValueError(f"parcel: diag[{name!r}] must hold {n_rows} x {sizes[name]} values")
        setattr(c_diag, name, _address(array, FLOAT))
    return c_diag


def diagnose_call(engine, formulae, requests, *, parcel_start, water_mass, multiplicity,
                  dry_volume, kappa, f_org, T, diag, descriptor=None, general=False):
    """one `sdm_parcel_diagnose` call with raw engine arrays: the request table on given columns
    at one temperature per parcel; `diag` as in `parcel_call` (without dv)"""
    if descriptor is None:
        descriptor = check_formulae(formulae)
    n_parcel = engine.size(parcel_start) - 1
    if engine.size(T) != n_parcel:
        raise ValueError("parcel: T must hold n_parcel values")
    sizes = {"moment_0": requests.n_moments, "moments": requests.n_moments,
             "spectrum": requests.n_bins, "dv": 0}
    consts = [float(getattr(formulae.constants, name)) for name in CONSTANT_NAMES]
    engine.call_parcel_diag(
        "sdm_parcel_diagnose", int(n_parcel), int(engine.size(water_mass)), parcel_start,
        water_mass, multiplicity, dry_volume, kappa, f_org, T, consts,
        None if is_default(descriptor) and not general else descriptor, requests,
        _diag_struct(engine, {k: v for k, v in diag.items() if k != "dv"}, sizes, n_parcel))


def check_collisions(collisions, counts, breakup=False):
    """what `sdm_parcel_run_coal` - with `breakup`: `sdm_parcel_run_collision` - refuses of a
    `recipe.CollisionSetup` and of the parcels' sizes, refused by name"""
    if collisions.breakup and not breakup:
        raise NotImplementedError("parcel with coalescence: breakup is not served "
                                  "(CollisionSetup.coalescence only) unless asked for with "
                                  "breakup=True (include/sdm_parcel_breakup.h)")
    if collisions.breakup and int(collisions.max_multiplicity) < 1:
        raise ValueError("parcel with breakup: max_multiplicity < 1")
    if collisions.optimized_random:
        raise NotImplementedError("parcel with coalescence: optimized_random is not served")
    if collisions.croupier != "local":
        raise NotImplementedError("parcel with coalescence: the global croupier is not "
                                  "served (a parcel is one cell: croupier='local')")
    most = int(np.max(np.asarray(counts, dtype=np.int64), initial=0))
    if most > abi.PARCEL_COAL_MAX_ROWS:
        raise ValueError(f"parcel with coalescence: a parcel of {most} rows, more than "
                         f"SDM_PARCEL_COAL_MAX_ROWS = {abi.PARCEL_COAL_MAX_ROWS}")


def collision_cfg(engine, collisions, dt, rho_w, terminal_velocity=None):
    """(the `sdm_step_cfg` of a CollisionSetup of coalescence for `sdm_parcel_run_coal` and the
    stage route - the parcel's rows, dv and stream are filled in per parcel -, the law's members
    as `vent_law` builds them or None, the clamped dt_coal_range)"""
    from .physics import constants as physics_constants  # pylint: disable=import-outside-toplevel

    k = physics_constants.namespace()
    desc = collisions.descriptor(k)
    law = None
    dt_range = collisions.clamped_dt_range(dt)
    cfg = abi.StepCfg()
    cfg.n_cell, cfg.n_attr, cfg.mass_attr = 1, 3, 0
    cfg.dt = dt
    cfg.dt_min, cfg.dt_max = dt_range
    cfg.adaptive, cfg.substeps = int(collisions.adaptive), int(collisions.substeps)
    cfg.croupier_local = int(collisions.croupier == "local")
    cfg.optimized_random = int(collisions.optimized_random)
    cfg.enable_breakup = int(collisions.breakup)
    cfg.handle_all_breakups = int(collisions.handle_all_breakups)
    cfg.kernel = desc.get("kernel", 0)
    cfg.ec, cfg.frag = desc.get("ec", 0), desc.get("frag", 0)
    # (the breakup members as CollisionRunner.step_cfg fills them: the stage route's yardstick)
    for name, width in (("kernel_param", 2), ("kernel_berry_params", 13), ("ec_param", 2),
                        ("frag_param", 2), ("berry_params", 13)):
        setattr(cfg, name, (abi.c_f64 * width)(*desc.get(name, (0.0,) * width)))
    cfg.kernel_berry_unit = desc.get("kernel_berry_unit", 1.0)
    cfg.berry_unit = desc.get("berry_unit", 1.0)
    cfg.eb_const = desc.get("eb_const", 0.0)
    cfg.frag_vmin, cfg.frag_nfmax = desc.get("frag_vmin", 0.0), desc.get("frag_nfmax", -1.0)
    cfg.rho_w, cfg.sgm_w = rho_w, k.sgm_w
    cfg.straub_consts = (abi.c_f64 * 6)(k.CM, k.STRAUB_E_D1, k.STRAUB_MU2, k.VEDDER_1987_A,
                                        k.VEDDER_1987_b, k.PI)
    cfg.max_multiplicity = int(collisions.max_multiplicity)
    if desc["needs_gk"]:
        name = tv.law_name(terminal_velocity or "GunnKinzer1949")
        if name not in engine.fused_velocity_laws:
            raise NotImplementedError(
                f"the fused collision step of engine `{engine.name}` does not evaluate the "
                f"terminal-velocity law {name!r} (it has "
                f"{', '.join(engine.fused_velocity_laws)})")
        law = vent_law(engine, tv.make_law(terminal_velocity or "GunnKinzer1949", engine, k))
        cfg.velocity_law = law["velocity_law"]
        cfg.velocity_terms = law["velocity_terms"]
        cfg.gk_table_len = law["gk_table_len"]
        cfg.gk_factor = law["gk_factor"]
    return cfg, law, dt_range


class ParcelRunner:  # pylint: disable=too-many-instance-attributes
    """an ensemble of adiabatic parcels; see the module's docstring.

    `counts[c]` rows of the per-droplet arrays (`multiplicity`, `water_mass`, `dry_volume`,
    `kappa`, `f_org`), in order, belong to parcel c.  `T0, p0, qv0, w, mass_of_dry_air, z0` are
    scalars or arrays of n_parcel; `w` may be a callable of time, or a list of n_parcel numbers
    and callables.  `steps_per_launch` (fused route): 0 for the library's default."""

    def __init__(self, engine, formulae, setup, *, dt, T0, p0, qv0, w, mass_of_dry_air, z0=0,
                 counts, multiplicity, water_mass, dry_volume, kappa, f_org=None, route="fused",
                 steps_per_launch=0, general=False, chemistry=None, mole_fractions=None,
                 dry_rho=None, dry_molar_mass=None, initial_moles=None, molar_mass=None,
                 terminal_velocity=None, descriptor=None, collisions=None, seed=None,
                 breakup=False, freezing=None, deposition=None, ice_order="freezing_first",
                 ice_seed=None, freezing_temperature=None, immersed_surface_area=None):
        """`terminal_velocity`: a name or a law object of pysdm_amd.terminal_velocity, needed
        (and read) with a ventilation other than Neglect, and by the collision kernels that take
        a fall velocity (the Gunn-Kinzer table if not given).  `descriptor`: one of
        `condensation.descriptor_of` instead of the formulae's own (a ventilation a `Formulae`
        refuses travels so).  `collisions`: a `recipe.CollisionSetup` of coalescence as the third
        dynamic (include/sdm_parcel_coal.h); `seed`: an int, or one per parcel (default: the
        setup's), each parcel drawing from its own NumPy-PCG64 stream.  `breakup=True`: the
        third dynamic is `Collision` / `Breakup` (include/sdm_parcel_breakup.h) - `collisions` may
        then be a set-up with breakup (CollisionSetup.collision, .breakup_only; without the keyword
        such a set-up is refused); a set-up of coalescence runs as it does without the keyword.
        `freezing` (a `freezing.FreezingSetup`) and / or `deposition` (True, or a dict with `sum`:
        "ordered" / "blocked"): the mixed-phase parcel (include/sdm_parcel_ice.h, pysdm_amd/
        parcel_ice.py) - `formulae` then name MixedPhaseSpheres, `water_mass` is the signed water
        mass, `ice_order` is "freezing_first" or "deposition_first", `ice_seed` an int or one per
        parcel (default: the formulae's), `freezing_temperature` / `immersed_surface_area` the
        per-row columns the set-up reads; `run` then returns (profile, ice profile)"""
        if route not in ROUTES:
            raise ValueError(f"route must be one of {ROUTES}, not {route!r}")
        check_hydrostatics(formulae)
        self.engine, self.formulae, self.setup = engine, formulae, setup
        self.mixed_phase = freezing is not None or bool(deposition)
        if self.mixed_phase:
            if descriptor is not None or chemistry is not None or collisions is not None:
                raise NotImplementedError(
                    "mixed-phase parcel: no descriptor=, chemistry or collisions in the same run")
            descriptor = parcel_ice.descriptor(formulae)
            if descriptor.option[_VENT] != 0 or terminal_velocity is not None:
                raise NotImplementedError("mixed-phase parcel: ventilated ice is not served")
        self.descriptor = check_formulae(formulae) if descriptor is None else descriptor
        self.ventilated = self.descriptor.option[_VENT] != 0
        self.terminal_velocity = None
        if route == "fused" and engine.parcel_library is None:
            raise NotImplementedError(
                f"engine `{engine.name}` has no parcel library: route='fused' is not "
                "available on it (route='stages' is)")
        if self.ventilated and collisions is not None:
            raise NotImplementedError(
                "parcel with coalescence: a ventilation other than Neglect is not served")
        if self.ventilated:
            if terminal_velocity is None:
                raise NotImplementedError(
                    "a parcel with a ventilation other than Neglect needs a fall velocity per "
                    "droplet per step: pass terminal_velocity=")
            if chemistry is not None:
                raise NotImplementedError(
                    "parcel with chemistry: a ventilation other than Neglect is not served")
            if route == "fused" and engine.parcel_vent_library is None:
                raise NotImplementedError(
                    f"engine `{engine.name}` has no library for the ventilated parcel: "
                    "route='fused' is not available on it (route='stages' is)")
            self.terminal_velocity = tv.make_law(terminal_velocity, engine, formulae.constants)
        if setup.dt_cond_range[0] == 0:
            raise NotImplementedError("dt_cond_range[0] == 0")
        self.chemistry = chemistry
        if chemistry is not None:
            if self.descriptor.option[_SGM] != 0:
                raise NotImplementedError(
                    "parcel with chemistry: a surface tension other than Constant is not served "
                    "(the organic fraction would have to follow the dry volume)")
            if mole_fractions is None or dry_rho is None or dry_molar_mass is None:
                raise ValueError("parcel with chemistry needs mole_fractions, dry_rho and "
                                 "dry_molar_mass")
            if route == "fused" and engine.parcel_chem_library is None:
                raise NotImplementedError(
                    f"engine `{engine.name}` has no library for the parcel with aqueous "
                    "chemistry: route='fused' is not available on it (route='stages' is)")
            if engine.chemistry_library is None:
                raise NotImplementedError(f"engine `{engine.name}` has no chemistry library")
        self.collisions = collisions
        self.breakup = bool(breakup)
        if self.breakup and collisions is None:
            raise ValueError("breakup=True needs collisions=")
        if collisions is not None:
            self._check_collisions(collisions, route, counts)
        self.route, self.general = route, bool(general)
        self.ice = None
        self.dt = float(dt)
        self.cfg = parcel_cfg(formulae, setup, self.dt, steps_per_launch)
        counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        if counts.size == 0 or (counts <= 0).any():
            raise ValueError("every parcel needs at least one super-droplet")
        self.n_parcel = n_parcel = int(counts.size)
        self.parcel_start_host = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        self.n_sd = n_sd = int(self.parcel_start_host[-1])
        const = formulae.constants

        def per_parcel(value, name):
            out = np.broadcast_to(np.asarray(value, dtype=float), (n_parcel,)).copy()
            if not np.isfinite(out).all():
                raise ValueError(f"{name} must be finite")
            return out

        def column(value, name, dtype):
            out = np.ascontiguousarray(value, dtype=dtype).reshape(-1)
            if out.size != n_sd:
                raise ValueError(f"{name} must hold sum(counts) = {n_sd} values")
            return engine.upload(out)

        self.w = self._updrafts(w)
        T0, p0, qv0 = per_parcel(T0, "T0"), per_parcel(p0, "p0"), per_parcel(qv0, "qv0")
        # Parcel.register, parcel.py:51-71 (trivia.p_d, rhod_of_pd_T, th_std)
        pd0 = p0 * (1 - 1 / (1 + const.eps / qv0))
        rhod0 = pd0 / const.Rd / T0
        thd0 = T0 * np.power(const.p1000 / pd0, const.Rd_over_c_pd)
        up = engine.upload
        self.state = {
            "z": up(per_parcel(z0, "z0")), "rhod": up(rhod0), "thd": up(thd0), "qv": up(qv0),
            "T": engine.empty(n_parcel, FLOAT), "p": engine.empty(n_parcel, FLOAT),
            "RH": engine.empty(n_parcel, FLOAT), "qv_prev": up(qv0.copy()),
            "mass_of_dry_air": up(per_parcel(mass_of_dry_air, "mass_of_dry_air")),
            "n_substeps": engine.full(n_parcel, INT, -1 if setup.adaptive else setup.substeps),
            "n_activating": engine.full(n_parcel, INT, -1),
            "n_deactivating": engine.full(n_parcel, INT, -1),
            "n_ripening": engine.full(n_parcel, INT, -1),
            "RH_max": engine.full(n_parcel, FLOAT, np.nan),
            "steps_done": engine.zeros(n_parcel, INT),
            "failed_step": engine.full(n_parcel, INT, -1),
        }
        temperature_pressure_rh_call(engine, formulae, self.state["rhod"], self.state["thd"],
                                     self.state["qv"], self.state["T"], self.state["p"],
                                     self.state["RH"], n_parcel, mixed_phase=self.mixed_phase)
        self.parcel_start = up(self.parcel_start_host)
        self.multiplicity = column(multiplicity, "multiplicity", np.int64)
        self.water_mass = column(water_mass, "water_mass", float)
        self.dry_volume = column(dry_volume, "dry_volume", float)
        self.kappa = column(np.broadcast_to(np.asarray(kappa, dtype=float), (n_sd,)), "kappa",
                            float)
        self.f_org = column(np.zeros(n_sd) if f_org is None else f_org, "f_org", float)
        self.critical_volume = engine.full(n_sd, FLOAT, np.nan)
        if self.ventilated:  # Parcel.register -> Moist.sync: the air of the initial state
            self.state.update({name: engine.empty(n_parcel, FLOAT) for name in VENT_STATE})
            self._sync_air(self.state["air_density"], self.state["air_dynamic_viscosity"],
                           self.state["rhod"], self.state["qv"], self.state["T"], n_parcel)
            self.reynolds_number = engine.full(n_sd, FLOAT, np.nan)
            self.out_of_table = engine.zeros(n_parcel, INT)
            self._vent_law = vent_law(engine, self.terminal_velocity)
        if self.mixed_phase:
            self.ice = parcel_ice.IceParcel(
                self, freezing=freezing, deposition=deposition, order=ice_order, seed=ice_seed,
                freezing_temperature=freezing_temperature,
                immersed_surface_area=immersed_surface_area)
        if chemistry is not None:
            self._init_chemistry(mole_fractions, dry_rho, dry_molar_mass, initial_moles,
                                 molar_mass, np.ascontiguousarray(dry_volume, dtype=float),
                                 np.broadcast_to(np.asarray(kappa, dtype=float), (n_sd,)))
        if collisions is not None:
            self._init_collisions(collisions, seed, terminal_velocity,
                                  np.ascontiguousarray(dry_volume, dtype=float),
                                  np.broadcast_to(np.asarray(kappa, dtype=float), (n_sd,)))
        self.last_chem_profile = None
        self.last_coal_profile = None
        self.last_ice_profile = None
        self.n_steps = 0  # time steps asked for so far: the clock of w(t)
        self.last_profile = None
        self.last_products = None
        self.last_rows = None
        self.diag_fill = np.nan  # what the rows of steps a failed parcel did not carry out hold
        self._reported = set()

    def _init_chemistry(self, mole_fractions, dry_rho, dry_molar_mass, initial_moles, molar_mass,
                        dry_volume, kappa):
        """the columns of the third dynamic: ammonium bisulphate (moles_S_VI = moles_N_mIII =
        vdry * dry_rho / dry_molar_mass, the others 0) unless `initial_moles` ({key: column})
        says otherwise, pH = pH_w, the flag clear, mixing ratios from the mole fractions"""
        eng, formulae, n_sd, n_parcel = self.engine, self.formulae, self.n_sd, self.n_parcel
        chem.check_formulae(formulae, molar_mass)
        self.dry_factor = float(dry_molar_mass) / float(dry_rho)
        self.chem_cfg = self.chemistry.cfg(formulae, self.dt, 0.0)  # (dv: per step)
        self.chem_consts = chem.constants_of(formulae, molar_mass)
        salt = dry_volume * float(dry_rho) / float(dry_molar_mass)
        unknown = set(initial_moles or {}) - set(chem.AQUEOUS)
        if unknown:
            raise ValueError(f"initial_moles of {sorted(unknown)}: the keys are {chem.AQUEOUS}")
        self.moles = []
        for key in chem.AQUEOUS:
            column = salt if key in ("S_VI", "N_mIII") else np.zeros(n_sd)
            if initial_moles and key in initial_moles:
                column = np.broadcast_to(np.asarray(initial_moles[key], dtype=float), (n_sd,))
            self.moles.append(eng.upload(np.ascontiguousarray(column, dtype=float).copy()))
        self.kappa_times_dry_volume = eng.upload(np.ascontiguousarray(kappa * dry_volume))
        self.pH = eng.full(n_sd, FLOAT, float(chem._constant(formulae, "pH_w")))  # pylint: disable=protected-access
        self.do_chemistry_flag = eng.zeros(n_sd, np.uint8)
        ratios = chem.mixing_ratios_of(mole_fractions, formulae, molar_mass)
        self.mixing_ratios = [eng.upload(np.broadcast_to(np.asarray(ratios[g], dtype=float),
                                                         (n_parcel,)).copy())
                              for g in chem.GASES]
        self.chem_counters = [eng.zeros(n_parcel, INT) for _ in CHEM_COUNTERS]

    def _chem_record(self, n_rows):
        eng = self.engine
        return {"mixing_ratio": [eng.full(n_rows, FLOAT, np.nan) for _ in chem.GASES],
                "aq_total": [eng.full(n_rows, FLOAT, np.nan) for _ in chem.AQUEOUS],
                "n_flagged": eng.full(n_rows, INT, -1), "dv": eng.full(n_rows, FLOAT, np.nan)}

    def _chem_call(self, record):
        return {"cfg": self.chem_cfg, "kappa_times_dry_volume": self.kappa_times_dry_volume,
                "moles": self.moles, "pH": self.pH, "do_chemistry_flag": self.do_chemistry_flag,
                "mixing_ratios": self.mixing_ratios, "consts": self.chem_consts,
                "dry_factor": self.dry_factor, "counters": self.chem_counters, "profile": record}

    # ---- coalescence (include/sdm_parcel_coal.h) ------------------------------------------------
    def _check_collisions(self, collisions, route, counts):
        """what the library refuses is refused here by name, on either route, before anything
        runs (a ventilated descriptor: by __init__ already)"""
        eng = self.engine
        if self.chemistry is not None:
            raise NotImplementedError(
                "parcel with coalescence: aqueous chemistry in the same run is not served")
        check_collisions(collisions, counts, self.breakup)
        if route == "fused" and eng.parcel_coal_library is None:
            raise NotImplementedError(
                f"engine `{eng.name}` has no library for the parcel with coalescence: "
                "route='fused' is not available on it (route='stages' is)")
        if route == "fused" and self.breakup and eng.parcel_breakup_library is None:
            raise NotImplementedError(
                f"engine `{eng.name}` has no library for the parcel with breakup: "
                "route='fused' is not available on it (route='stages' is)")

    def _init_collisions(self, collisions, seed, terminal_velocity, dry_volume, kappa):
        """the arrays of the third dynamic and its `sdm_step_cfg`: the identity permutation, all
        rows live, kappa times dry volume, the counters of `CollisionRunner` per parcel, one
        stream per parcel at position 0"""
        eng, n_parcel, n_sd = self.engine, self.n_parcel, self.n_sd
        self.coal_cfg, self._coal_law, self.coal_dt_range = collision_cfg(
            eng, collisions, self.dt, float(self.formulae.constants.rho_w), terminal_velocity)
        seeds = np.broadcast_to(np.asarray(collisions.seed if seed is None else seed),
                                (n_parcel,))
        words = np.array([abi.pcg64_state_inc(int(s)) for s in seeds], dtype=np.uint64)
        self._seed_words = words
        self.rng_state_inc = eng.upload(words.reshape(-1).view(np.int64).copy())
        self.rng_offset = eng.zeros(n_parcel, INT)
        self.idx = eng.upload(np.arange(n_sd, dtype=np.int64))
        self.n_live = eng.upload(np.diff(self.parcel_start_host).astype(np.int64))
        self.kappa_times_dry_volume = eng.upload(np.ascontiguousarray(kappa * dry_volume))
        self.coal_counters = {name: eng.zeros(n_parcel, INT) for name in COAL_COUNTERS}
        self.stats_n_substep = eng.full(n_parcel, INT,
                                        0 if collisions.adaptive else collisions.substeps)
        self.stats_dt_min = eng.full(n_parcel, FLOAT, np.nan)
        self.coal_events = eng.zeros(n_parcel, INT)
        self._fresh_idx = True
        if self.breakup:  # include/sdm_parcel_breakup.h: the proc / frag stream at position 0
            self.breakup_counters = {name: eng.zeros(n_parcel, INT) for name in BREAKUP_COUNTERS}
            self.rng_offset_breakup = eng.zeros(n_parcel, INT)

    def _coal_columns(self, get=lambda array: array):
        """the columns coalescence adds to a snapshot, by name (`get` applied to every array)"""
        out = {"multiplicity": get(self.multiplicity), "dry_volume": get(self.dry_volume),
               "kappa": get(self.kappa),
               "kappa_times_dry_volume": get(self.kappa_times_dry_volume),
               "idx": get(self.idx), "n_live": get(self.n_live),
               "stats_n_substep": get(self.stats_n_substep),
               "stats_dt_min": get(self.stats_dt_min), "events": get(self.coal_events),
               "rng_offset": get(self.rng_offset)}
        out.update({name: get(array) for name, array in self.coal_counters.items()})
        if self.breakup:
            out.update({name: get(array) for name, array in self.breakup_counters.items()})
            out["rng_offset_breakup"] = get(self.rng_offset_breakup)
        return out

    @property
    def with_breakup(self):
        """the collisions are a set-up with breakup (asked for with breakup=True)"""
        return self.breakup and bool(self.collisions.breakup)

    def _coal_record(self, n_rows):
        """the record of the call: the members of sdm_parcel_coal_profile and, with breakup, of
        sdm_parcel_breakup_profile (the two sets of names are disjoint)"""
        eng = self.engine
        out = {name: eng.full(n_rows, FLOAT, np.nan) if name == "dv"
               else eng.full(n_rows, INT, -1) for name in abi.PARCEL_COAL_PROFILE_FIELDS}
        if self.with_breakup:
            out.update({name: eng.full(n_rows, INT, -1)
                        for name in abi.PARCEL_BREAKUP_PROFILE_FIELDS})
        return out

    def _coal_call(self, record):
        law = self._coal_law or {}
        breakup = None
        if self.breakup:
            breakup = {**self.breakup_counters, "rng_offset_breakup": self.rng_offset_breakup,
                       "profile": ({name: record[name]
                                    for name in abi.PARCEL_BREAKUP_PROFILE_FIELDS}
                                   if self.with_breakup else None)}
            record = {name: record[name] for name in abi.PARCEL_COAL_PROFILE_FIELDS}
        return {"cfg": self.coal_cfg, "breakup": breakup, "idx": self.idx, "n_live": self.n_live,
                "kappa_times_dry_volume": self.kappa_times_dry_volume, **self.coal_counters,
                "stats_n_substep": self.stats_n_substep, "stats_dt_min": self.stats_dt_min,
                "events": self.coal_events, "rng_offset": self.rng_offset,
                "rng_state_inc": self.rng_state_inc, "gk_a": law.get("gk_a"),
                "gk_b": law.get("gk_b"), "velocity_params": law.get("velocity_params"),
                "fresh_idx": self._fresh_idx, "profile": record}

    def _coal_warnings(self):
        """the events of the last call as the warnings `CollisionRunner` issues"""
        eng = self.engine
        events = eng.download(self.coal_events)
        if (events & abi.PARCEL_COAL_EVENT_BOUND).any():
            eng.assign(self.coal_events, eng.upload(events & ~abi.PARCEL_COAL_EVENT_BOUND))
            raise RuntimeError("parcel with coalescence: an adaptive time step did not end "
                               "within the bound its own arithmetic sets, in parcels "
                               f"{np.flatnonzero(events & abi.PARCEL_COAL_EVENT_BOUND).tolist()}")
        overflows = events >> abi.PARCEL_COAL_OVERFLOW_SHIFT
        if (events & abi.PARCEL_COAL_EVENT_DT_MIN).any():
            # the reference's condition (collision.py:276-277; a NaN entry, the initial state,
            # silences it)
            if np.min(eng.download(self.stats_dt_min)) == self.coal_dt_range[0]:
                warnings.warn("adaptive time-step reached dt_min")
        if (overflows > 0).any() and self.collisions.warn_overflows:
            warnings.warn("overflow")
        if events.any():
            eng.fill(self.coal_events, 0)

    def _live_rows(self):
        """(rows of every parcel's live positions in position order, their parcel_start)"""
        idx = self.engine.download(self.idx)
        n_live = self.engine.download(self.n_live)
        starts = self.parcel_start_host
        rows = np.concatenate([idx[starts[c]:starts[c] + n_live[c]]
                               for c in range(self.n_parcel)])
        return rows.astype(np.int64), np.concatenate(([0], np.cumsum(n_live))).astype(np.int64)

    def _run_stages_coal(self, w_mid, record, coal_record):  # pylint: disable=too-many-locals,too-many-statements
        """the time step of include/sdm_parcel_coal.h with the stage symbols, parcel after
        parcel: the stage step of `_run_stages` over the parcel's slice with its permutation and
        live count, `sdm_collision_step` with n_cell = 1 and the step's dv on that slice, the
        division of point 3.  With a set-up with breakup (include/sdm_parcel_breakup.h) the
        collision step gets the parcel's breakup counters and the position of its proc / frag
        stream.  The yardstick of the fused route"""
        eng, const, cfg, setup = self.engine, self.formulae.constants, self.cfg, self.setup
        host = {name: eng.download(array) for name, array in self.state.items()}
        rows = {name: (eng.download(array) if array is not None else None)
                for name, array in (record or {}).items()}
        coal_rows = {name: eng.download(array) for name, array in coal_record.items()}
        idx_host, n_live = eng.download(self.idx), eng.download(self.n_live)
        offsets, events = eng.download(self.rng_offset), eng.download(self.coal_events)
        offsets_b = eng.download(self.rng_offset_breakup) if self.with_breakup else None
        one = {name: eng.empty(1, FLOAT) for name in
               ("rhod", "thd", "qv", "prhod", "pthd", "pqv", "T", "p", "RH", "RH_max", "lv")}
        counters = {name: eng.empty(1, INT) for name in
                    ("n_substeps", "n_activating", "n_deactivating", "n_ripening")}
        success = eng.zeros(1, np.uint8)
        zero = eng.zeros(1, INT)
        most = int(np.diff(self.parcel_start_host).max())
        v_wet, backup, v_cr = (eng.empty(most, FLOAT) for _ in range(3))
        cell = eng.zeros(most, INT)
        block, spare = eng.empty(3 * most, FLOAT), eng.empty(most, INT)
        dt_left = eng.empty(1, FLOAT)
        dt_range = (setup.dt_cond_range[0], min(setup.dt_cond_range[1], self.dt))
        n_parcel = self.n_parcel
        law = self._coal_law or {}
        result = abi.StepResult()

        def address(array):
            return None if array is None else abi.c_ptr(
                array.data_ptr() if hasattr(array, "data_ptr") else array.ctypes.data)

        for c in range(n_parcel):
            if host["failed_step"][c] >= 0:
                continue
            r0, r1 = (int(v) for v in self.parcel_start_host[c:c + 2])
            n_rows = r1 - r0
            mass = self.water_mass[r0:r1]
            for k in range(w_mid.shape[0]):
                live = int(n_live[c])
                rel_host = (idx_host[r0:r0 + live] - r0).astype(np.int64)
                rel = eng.upload(rel_host)
                cell_start = eng.upload(np.array([0, live], dtype=np.int64))
                T, p = float(host["T"][c]), float(host["p"][c])
                rhod, thd, qv = (float(host[v][c]) for v in ("rhod", "thd", "qv"))
                w, dt = float(w_mid[k, c]), self.dt
                delta = float(host["qv_prev"][c]) - qv
                qv_mid = qv - delta / 2
                lv = self._latent_heat(T, one["lv"])
                Rq = const.Rv / (1 / qv_mid + 1) + const.Rd / (1 + qv_mid)
                cp = const.c_pv / (1 / qv_mid + 1) + const.c_pd / (1 + qv_mid)
                rho = p / Rq / T
                dql_dz = delta / w / dt
                drho_dz = (cfg.g_std / T * rho * (Rq / cp - 1)
                           - p * lv / cp / (T * T) * dql_dz) / Rq
                z = float(host["z"][c]) + dt * w
                prhod = rhod + dt * (w * drho_dz)
                dv = float(host["mass_of_dry_air"][c]) / ((prhod + rhod) / 2)
                for name, value in (("rhod", rhod), ("thd", thd), ("qv", qv), ("prhod", prhod),
                                    ("pthd", thd), ("pqv", qv), ("T", T)):
                    eng.fill(one[name], value)
                eng.fill(counters["n_substeps"], int(host["n_substeps"][c]))
                eng.call("sdm_volume_of_water_mass", v_wet[:n_rows], mass, n_rows,
                         float(const.rho_w))
                eng.assign(backup[:n_rows], mass)
                # the critical volume of the live rows only (the others are not written)
                critical_volume_call(eng, self.formulae, v_cr[:n_rows], self.kappa[r0:r1],
                                     self.f_org[r0:r1], self.dry_volume[r0:r1], v_wet[:n_rows],
                                     one["T"], cell[:n_rows], n_rows)
                self.critical_volume[r0:r1][rel] = v_cr[:n_rows][rel]
                condensation_call(
                    eng, formulae=self.formulae, n_sd=n_rows, n_cell=1, cell_start=cell_start,
                    water_mass=mass, v_cr=self.critical_volume[r0:r1],
                    multiplicity=self.multiplicity[r0:r1], vdry=self.dry_volume[r0:r1],
                    idx=rel, rhod=one["rhod"], thd=one["thd"],
                    water_vapour_mixing_ratio=one["qv"], dv=dv, prhod=one["prhod"],
                    pthd=one["pthd"], predicted_water_vapour_mixing_ratio=one["pqv"],
                    kappa=self.kappa[r0:r1], f_org=self.f_org[r0:r1], rtol_x=setup.rtol_x,
                    rtol_thd=setup.rtol_thd, timestep=dt, counters=counters, cell_order=zero,
                    RH_max=one["RH_max"], success=success, reynolds_number=None,
                    air_density=None, air_dynamic_viscosity=None, dt_range=dt_range,
                    adaptive=setup.adaptive, fuse=setup.fuse, multiplier=setup.multiplier,
                    RH_rtol=setup.RH_rtol, max_iters=setup.max_iters, general=self.general,
                    descriptor=self.descriptor)
                if not eng.download(success)[0]:
                    eng.assign(mass, backup[:n_rows])
                    host["failed_step"][c] = host["steps_done"][c]
                    break
                temperature_pressure_rh_call(eng, self.formulae, one["prhod"], one["pthd"],
                                             one["pqv"], one["T"], one["p"], one["RH"], 1)
                n_sub = int(eng.download(counters["n_substeps"])[0])
                if setup.adaptive:  # dynamics/condensation.py:122-131
                    n_sub = min(max(n_sub, int(cfg.n_clamp_lo)), int(cfg.n_clamp_hi))
                host["qv_prev"][c] = qv
                host["z"][c], host["rhod"][c] = z, prhod
                host["thd"][c] = eng.download(one["pthd"])[0]
                host["qv"][c] = eng.download(one["pqv"])[0]
                for name in ("T", "p", "RH", "RH_max"):
                    host[name][c] = eng.download(one[name])[0]
                host["n_substeps"][c] = n_sub
                for name in ("n_activating", "n_deactivating", "n_ripening"):
                    host[name][c] = eng.download(counters[name])[0]
                host["steps_done"][c] += 1
                for name, row in rows.items():
                    if row is not None:
                        row[k * n_parcel + c] = host[name][c]
                # ---- point 2: the parcel as one cell of sdm_collision_step -----------------------
                at = k * n_parcel + c
                new_live, n_collision_sub = live, 0
                tracked = {name: self.coal_counters[name]
                           for name in ("coalescence_rate", "collision_rate_deficit")}
                if self.with_breakup:
                    tracked.update(self.breakup_counters)
                    coal_rows["n_overflow"][at] = 0
                before = {name: int(eng.download(array[c:c + 1])[0])
                          for name, array in tracked.items()}
                if n_rows >= 2:
                    columns = (mass, self.dry_volume[r0:r1], self.kappa_times_dry_volume[r0:r1])
                    for a, column in enumerate(columns):
                        eng.assign(block[a * n_rows:(a + 1) * n_rows], column)
                    perm = eng.upload(np.concatenate(
                        [rel_host, np.full(n_rows - live, n_rows, dtype=np.int64)]))
                    ctl = eng.upload(np.array([live, live, 1, 1, 0, 0, 0, 0], dtype=np.int64))
                    step_cfg = abi.StepCfg.from_buffer_copy(self.coal_cfg)
                    step_cfg.n_sd, step_cfg.dv = n_rows, dv
                    step_cfg.rng_state_inc = (abi.c_u64 * 4)(*(int(v) for v in
                                                               self._seed_words[c]))
                    state = abi.StepState()
                    for name, array in (
                            ("idx", perm), ("tmp_idx", spare[:n_rows]),
                            ("multiplicity", self.multiplicity[r0:r1]),
                            ("attributes", block[:3 * n_rows]), ("cell_id", cell[:n_rows]),
                            ("cell_idx", zero), ("cell_start", cell_start),
                            ("dt_left", dt_left), ("stats_dt_min", self.stats_dt_min[c:c + 1]),
                            ("stats_n_substep", self.stats_n_substep[c:c + 1]),
                            ("collision_rate", self.coal_counters["collision_rate"][c:c + 1]),
                            ("collision_rate_deficit",
                             self.coal_counters["collision_rate_deficit"][c:c + 1]),
                            ("coalescence_rate",
                             self.coal_counters["coalescence_rate"][c:c + 1]),
                            ("gk_a", law.get("gk_a")), ("gk_b", law.get("gk_b")),
                            ("velocity_params", law.get("velocity_params")), ("ctl", ctl)):
                        setattr(state, name, address(array))
                    state.known_valid = -1
                    state.rng_offset = int(offsets[c])
                    if self.with_breakup:
                        for name, array in self.breakup_counters.items():
                            setattr(state, name, address(array[c:c + 1]))
                        state.rng_offset_breakup = int(offsets_b[c])
                    eng.call("sdm_collision_step", step_cfg, state, result, 1 | 2)
                    words = list(result.ctl)
                    if int(words[7]) & 0xff:
                        raise RuntimeError("libsdm_hip: device-side failure in the fused "
                                           f"collision step: code {int(words[7]) & 0xff}")
                    now = eng.download(spare[:n_rows] if result.idx_swapped else perm)
                    new_live = int(result.valid_n_sd)
                    n_collision_sub = int(result.n_substeps)
                    idx_host[r0:r0 + new_live] = r0 + now[:new_live]
                    for a, column in enumerate(columns):
                        eng.assign(column, block[a * n_rows:(a + 1) * n_rows])
                    offsets[c] = int(result.rng_offset)
                    if self.with_breakup:
                        offsets_b[c] = int(result.rng_offset_breakup)
                        coal_rows["n_overflow"][at] = int(words[4])
                    n_live[c] = new_live
                    if int(words[7]) & 0x100:
                        events[c] |= abi.PARCEL_COAL_EVENT_DT_MIN
                    if int(words[4]) > 0:
                        events[c] += int(words[4]) << abi.PARCEL_COAL_OVERFLOW_SHIFT
                # ---- point 3 -------------------------------------------------------------------------
                alive = eng.upload((idx_host[r0:r0 + new_live] - r0).astype(np.int64))
                self.kappa[r0:r1][alive] = (self.kappa_times_dry_volume[r0:r1][alive]
                                            / self.dry_volume[r0:r1][alive])
                coal_rows["n_live"][at] = new_live
                coal_rows["n_substeps"][at] = n_collision_sub
                for name, was in before.items():
                    coal_rows[name][at] = int(eng.download(tracked[name][c:c + 1])[0]) - was
                coal_rows["dv"][at] = dv
        for name, value in coal_rows.items():
            eng.assign(coal_record[name], eng.upload(value))
        for name, value in (("idx", idx_host), ("n_live", n_live), ("rng_offset", offsets),
                            ("coal_events", events), ("rng_offset_breakup", offsets_b)):
            if value is not None:
                eng.assign(getattr(self, name), eng.upload(value))
        for name, array in self.state.items():
            eng.assign(array, eng.upload(host[name]))
        for name, row in rows.items():
            if row is not None:
                eng.assign(record[name], eng.upload(row))

    # ---- construction from a spectrum ---------------------------------------------------------
    @classmethod
    def from_spectrum(cls, engine, formulae, setup, *, dt, T0, p0, qv0, w, mass_of_dry_air,
                      spectrum, kappa, n_sd, n_parcel=1, z0=0, f_org=None,
                      sampling="constant_multiplicity", **kwargs):
        """`n_parcel` parcels of `n_sd` super-droplets each, sampled from the dry-radius `spectrum`
        (per kg of dry air) and brought to Koehler equilibrium with each parcel's initial air by
        `initialisation.wet_aerosol`; multiplicity = discretise(n_per_kg * mass_of_dry_air), what
        `Parcel.init_attributes` callers pass as n_in_dv"""
        from . import initialisation  # pylint: disable=import-outside-toplevel
        from .condensation import AmbientColumns  # pylint: disable=import-outside-toplevel

        const = formulae.constants
        broadcast = lambda v: np.broadcast_to(np.asarray(v, dtype=float), (n_parcel,))  # noqa: E731
        T0b, p0b, qv0b, mass = broadcast(T0), broadcast(p0), broadcast(qv0), broadcast(
            mass_of_dry_air)
        pd0 = p0b * (1 - 1 / (1 + const.eps / qv0b))
        ambient = AmbientColumns(engine, formulae, rhod=pd0 / const.Rd / T0b,
                                 thd=T0b * np.power(const.p1000 / pd0, const.Rd_over_c_pd),
                                 qv=qv0b)
        cells = np.repeat(np.arange(n_parcel, dtype=np.int64), n_sd)
        sampler = initialisation.SAMPLERS[sampling] if isinstance(sampling, str) else sampling

        def tiled(spec, _):  # every parcel gets the same n_sd bins of the spectrum
            r_dry, n_per_kg = sampler(spec, n_sd)
            return np.tile(r_dry, n_parcel), np.tile(n_per_kg, n_parcel)

        forg = None if f_org is None else np.broadcast_to(np.asarray(f_org, dtype=float),
                                                          (n_parcel * n_sd,)).copy()
        drops = initialisation.wet_aerosol(engine, formulae, ambient, spectrum=spectrum,
                                           kappa=kappa, n_sd=n_parcel * n_sd, cell_id=cells,
                                           f_org=forg, sampling=tiled)
        multiplicity = initialisation.discretise_multiplicities(drops["n_per_kg"] * mass[cells])
        return cls(engine, formulae, setup, dt=dt, T0=T0, p0=p0, qv0=qv0, w=w,
                   mass_of_dry_air=mass_of_dry_air, z0=z0, counts=np.full(n_parcel, n_sd),
                   multiplicity=multiplicity, water_mass=drops["water_mass"],
                   dry_volume=drops["dry_volume"], kappa=drops["kappa"], f_org=forg, **kwargs)

    # ---- updrafts -------------------------------------------------------------------------------
    def _updrafts(self, w):
        if callable(w):
            return [w] * self.n_parcel
        if isinstance(w, (list, tuple)) and any(callable(item) for item in w):
            if len(w) != self.n_parcel:
                raise ValueError("w must hold one entry per parcel")
            return [item if callable(item) else (lambda _, value=float(item): value)
                    for item in w]
        values = np.broadcast_to(np.asarray(w, dtype=float), (self.n_parcel,))
        return [(lambda _, value=float(value): value) for value in values]

    def w_mid(self, n_steps):
        """w((k + 1/2) dt) of the next `n_steps` steps (parcel.py:109), n_steps x n_parcel"""
        out = np.empty((n_steps, self.n_parcel))
        for k in range(n_steps):
            t = (self.n_steps + k + 1 / 2) * self.dt
            for c, w in enumerate(self.w):
                out[k, c] = w(t)
        if not np.isfinite(out).all() or (out == 0).any():
            raise ValueError("parcel: the updraft must be finite and non-zero at every step's "
                             "mid-point (the step divides by it)")
        return out

    # ---- running ----------------------------------------------------------------------------------
    def _table(self, products):
        if self.engine.parcel_diag_library is None:
            raise NotImplementedError(f"engine `{self.engine.name}` has no parcel-diagnostics "
                                      "library: products are not available on it")
        return products if isinstance(products, RequestTable) else RequestTable(products,
                                                                                self.formulae)

    def _diag_arrays(self, table, n_rows, dv=True):
        """engine arrays for `n_rows` rows of the table's outputs, prefilled with `diag_fill`
        (NaN): rows of steps a failed parcel did not carry out stay so"""
        eng = self.engine
        sizes = {"moment_0": table.n_moments, "moments": table.n_moments,
                 "spectrum": table.n_bins, "dv": 1 if dv else 0}
        return {name: eng.full(n_rows * size, FLOAT, self.diag_fill) for name, size in sizes.items()
                if size > 0}

    def _rows(self, table, diag, shape, rhod, dv=None):
        down = self.engine.download

        def get(name, width):
            if name not in diag:  # (no such requests, or no steps)
                return np.full((*shape, width), np.nan)
            return down(diag[name]).reshape(*shape, width)

        return Rows(table, moment_0=get("moment_0", table.n_moments),
                    moments=get("moments", table.n_moments),
                    spectrum=get("spectrum", table.n_bins),
                    dv=down(diag["dv"]).reshape(shape) if dv is None else dv, rhod=rhod)

    def diagnose(self, products, dv=None):
        """the products of the current state, {name: array of n_parcel (x n_bins)}: the request
        table on the runner's columns at the parcels' temperatures (`sdm_parcel_diagnose`).  `dv`
        defaults to mass_of_dry_air / rhod, `mesh.dv` of a parcel that has not moved yet (after a
        step PySDM's mesh.dv is the step's mid-point volume, which `run` reports)"""
        table = self._table(products)
        diag = self._diag_arrays(table, self.n_parcel, dv=False)
        columns = {"parcel_start": self.parcel_start, "water_mass": self.water_mass,
                   "multiplicity": self.multiplicity, "dry_volume": self.dry_volume,
                   "kappa": self.kappa, "f_org": self.f_org}
        if self.collisions is not None:
            # every parcel's live rows in position order, gathered (rows that died hold no drop)
            rows, starts = self._live_rows()
            rows = self.engine.upload(rows)
            columns = {name: array if name == "parcel_start" else array[rows]
                       for name, array in columns.items()}
            columns["parcel_start"] = self.engine.upload(starts)
        diagnose_call(self.engine, self.formulae, table.c_struct(), **columns,
                      T=self.state["T"], diag=diag, descriptor=self.descriptor,
                      general=self.general)
        rhod = self.engine.download(self.state["rhod"])
        if dv is None:
            dv = self.engine.download(self.state["mass_of_dry_air"]) / rhod
        rows = self._rows(table, diag, (self.n_parcel,), rhod,
                          dv=np.broadcast_to(np.asarray(dv, dtype=float), (self.n_parcel,)))
        self.last_rows = rows
        return table.values(rows)

    def run(self, n_steps, profile=True, products=()):
        """`n_steps` further time steps of every parcel that has not failed; returns the profile
        (host arrays of n_steps x n_parcel by the names of sdm_parcel_profile; entries of steps a
        failed parcel did not carry out are NaN / -1) or None.  With `products` (a sequence of
        pysdm_amd.products objects, or a RequestTable) it returns (profile, {product name: array
        of n_steps x n_parcel (x n_bins)}): the products of the state after every step (NaN for
        steps a failed parcel did not carry out); the evaluated table itself is kept in
        `last_rows`.  With chemistry the chemistry profile ({"mixing_ratio": 6 x n_steps x
        n_parcel, "aq_total": 7 x ..., "n_flagged", "dv"}, kept in `last_chem_profile`) comes
        second: (profile, chemistry profile) or (profile, chemistry profile, products).  Raises
        RuntimeError("Condensation failed", parcel, step) after the call for the first parcel whose
        solver failed in it: the other parcels' state stays valid (and the profile is kept in
        `last_profile`); a failed parcel is skipped from then on.  A ventilated parcel stopped by
        the range of the Gunn-Kinzer table (a radius above its top) is such a parcel too, but
        raises the ValueError of `GunnKinzerTable.evaluate`"""
        n_steps = int(n_steps)
        if n_steps < 0:
            raise ValueError("n_steps must not be negative")
        eng, n_parcel = self.engine, self.n_parcel
        record = None
        if self.collisions is not None and (isinstance(products, RequestTable) or len(products)):
            raise NotImplementedError(
                "parcel with coalescence: products at output times come from `run(k); "
                "diagnose(products)` (the per-step request table is not part of "
                "sdm_parcel_run_coal)")
        table = self._table(products) if isinstance(products, RequestTable) or len(products) \
            else None
        diag = None
        chem_record = None
        if n_steps > 0 and self.chemistry is not None:
            chem_record = self._chem_record(n_steps * n_parcel)
        coal_record = None
        if n_steps > 0 and self.collisions is not None:
            coal_record = self._coal_record(n_steps * n_parcel)
        if n_steps > 0:
            w_mid = self.w_mid(n_steps)
            if table is not None:
                diag = self._diag_arrays(table, n_steps * n_parcel)
                if not profile:  # (the specific products divide by the step's rhod)
                    record = {"rhod": eng.full(n_steps * n_parcel, FLOAT, np.nan)}
            if profile:
                record = {name: eng.full(n_steps * n_parcel, INT, -1) if name.startswith("n_")
                          else eng.full(n_steps * n_parcel, FLOAT, np.nan)
                          for name in abi.PARCEL_PROFILE_FIELDS}
            if self.ice is not None:
                if table is not None:
                    raise NotImplementedError(
                        "mixed-phase parcel: the only products are those of the ice profile")
                ice_record = self.ice.record(eng, n_steps * n_parcel)
                if self.route == "fused":
                    self.ice.run_fused(self, n_steps, w_mid, record, ice_record)
                else:
                    self.ice.run_stages(self, w_mid, record, ice_record)
            elif self.route == "fused":
                parcel_call(eng, self.formulae, self.cfg, n_steps=n_steps,
                            parcel_start=self.parcel_start, water_mass=self.water_mass,
                            multiplicity=self.multiplicity, dry_volume=self.dry_volume,
                            kappa=self.kappa, f_org=self.f_org,
                            critical_volume=self.critical_volume, state=self.state,
                            w_mid=eng.upload(w_mid.reshape(-1)), profile=record,
                            descriptor=self.descriptor, general=self.general,
                            requests=None if table is None else table.c_struct(), diag=diag,
                            chem=None if self.chemistry is None else self._chem_call(chem_record),
                            vent=self._vent_call() if self.ventilated else None,
                            coal=None if self.collisions is None
                            else self._coal_call(coal_record))
            elif self.collisions is not None:
                self._run_stages_coal(w_mid, record, coal_record)
            else:
                self._run_stages(w_mid, record, table, diag, chem_record)
            self.n_steps += n_steps
            self._fresh_idx = False
        out = None
        if record is not None:
            out = {name: eng.download(array).reshape(n_steps, n_parcel)
                   for name, array in record.items()}
        values = None
        if table is not None:
            shape = (n_steps, n_parcel)
            rhod = out["rhod"] if n_steps > 0 else np.empty(shape)
            self.last_rows = self._rows(table, diag or {"dv": eng.empty(0, FLOAT)}, shape, rhod)
            values = table.values(self.last_rows)
            if not profile:
                out = None
        self.last_profile, self.last_products = out, values
        chem_out = None
        if self.chemistry is not None:
            shape = (n_steps, n_parcel)
            get = lambda a: eng.download(a).reshape(shape)  # noqa: E731
            if chem_record is None:
                chem_record = {"mixing_ratio": [eng.empty(0, FLOAT)] * 6,
                               "aq_total": [eng.empty(0, FLOAT)] * 7,
                               "n_flagged": eng.empty(0, INT), "dv": eng.empty(0, FLOAT)}
            chem_out = {"mixing_ratio": np.stack([get(a) for a in chem_record["mixing_ratio"]]),
                        "aq_total": np.stack([get(a) for a in chem_record["aq_total"]]),
                        "n_flagged": get(chem_record["n_flagged"]), "dv": get(chem_record["dv"])}
            self.last_chem_profile = chem_out
        coal_out = None
        if self.collisions is not None:
            if coal_record is None:
                coal_record = {name: eng.empty(0, FLOAT if name == "dv" else INT)
                               for name in abi.PARCEL_COAL_PROFILE_FIELDS + (
                                   abi.PARCEL_BREAKUP_PROFILE_FIELDS if self.with_breakup
                                   else ())}
            coal_out = {name: eng.download(array).reshape(n_steps, n_parcel)
                        for name, array in coal_record.items()}
            self.last_coal_profile = coal_out
            self._coal_warnings()
        ice_out = None
        if self.ice is not None:
            if n_steps > 0:
                ice_out = {name: eng.download(array).reshape(n_steps, n_parcel)
                           for name, array in ice_record.items()}
            self.last_ice_profile = ice_out
        failed = eng.download(self.state["failed_step"])
        for parcel in np.flatnonzero(failed >= 0):
            if int(parcel) not in self._reported:
                self._reported.update(int(p) for p in np.flatnonzero(failed >= 0))
                if self.ventilated and eng.download(self.out_of_table)[parcel]:
                    self._raise_out_of_table(int(parcel))
                raise RuntimeError("Condensation failed", int(parcel), int(failed[parcel]))
        if self.chemistry is not None:
            return (out, chem_out) if table is None else (out, chem_out, values)
        if self.collisions is not None:
            return out, coal_out
        if self.ice is not None:
            return out, ice_out
        return out if table is None else (out, values)

    # ---- ventilation (include/sdm_parcel_vent.h) ---------------------------------------------------
    def _sync_air(self, air_density, air_dynamic_viscosity, rhod, qv, T, n):
        """what Moist.sync leaves in the environment's "air density" and "air dynamic viscosity"
        (moist.py:73-100), with the stage symbols"""
        eng = self.engine
        consts = [float(getattr(self.formulae.constants, name)) for name in CONSTANT_NAMES]
        eng.call_condensation("sdm_air_density", air_density, rhod, qv, n)
        eng.call_condensation("sdm_air_dynamic_viscosity", air_dynamic_viscosity, T, n, consts)

    def _radius(self, out, mass, n):
        """attributes/physics/radius.py of water masses, with the symbols `Population.radius`
        launches"""
        eng, const = self.engine, self.formulae.constants
        eng.call("sdm_volume_of_water_mass", out, mass, n, float(const.rho_w))
        eng.call("sdm_elementwise_f64", 2, out, out, None, 1 / float(const.PI_4_3), n)
        eng.call("sdm_elementwise_f64", 4, out, out, None, 1 / 3, n)

    def _largest_radius(self, radius, n):
        return self.engine.scalar_out("sdm_reduce_f64", ctypes.c_double, 1, radius, n)

    def _vent_call(self):
        return {**self._vent_law, "air_density": self.state["air_density"],
                "air_dynamic_viscosity": self.state["air_dynamic_viscosity"],
                "reynolds_number": self.reynolds_number, "out_of_table": self.out_of_table}

    def _raise_out_of_table(self, parcel):
        """what GunnKinzerTable.evaluate raises for the radii that stopped `parcel` (its water
        masses are those of before the step)"""
        r0, r1 = (int(v) for v in self.parcel_start_host[parcel:parcel + 2])
        radius = self.engine.empty(r1 - r0, FLOAT)
        self._radius(radius, self.water_mass[r0:r1], r1 - r0)
        raise ValueError(f"Radii can be interpolated up to {self.terminal_velocity.maximum_radius}"
                         f" m (max value of {self._largest_radius(radius, r1 - r0)} m within "
                         "input data)")

    def _latent_heat(self, T, scratch):
        """formulae.latent_heat_vapourisation.lv(T) in the library's arithmetic: Kirchhoff and
        Constant are plain doubles; Lowe2019's power goes through `sdm_elementwise_f64` (the
        library's pow, which the kernels evaluate), one element"""
        const = self.formulae.constants
        choice = self.descriptor.option[_LV]
        if choice == 1:
            return const.l_tri
        if choice == 2:
            eng = self.engine
            eng.fill(scratch, const.T_tri / T)
            eng.call("sdm_elementwise_f64", 4, scratch, scratch, None,
                     float(const.l_l19_a + const.l_l19_b * T), 1)
            return const.l_tri * float(eng.download(scratch)[0])
        return const.l_tri + (const.c_pv - const.c_pw) * (T - const.T_tri)

    def _run_stages(self, w_mid, record, table=None, diag=None, chem_record=None):  # pylint: disable=too-many-locals,too-many-statements
        """the time step of include/sdm_parcel.h with the stage symbols, parcel after parcel; the
        products' table with `sdm_parcel_diagnose` on the parcel's slice after each step"""
        eng, const, cfg, setup = self.engine, self.formulae.constants, self.cfg, self.setup
        diag_rows = {name: eng.download(array) for name, array in (diag or {}).items()}
        if table is not None:
            requests = table.c_struct()
            one_diag = self._diag_arrays(table, 1, dv=False)
            widths = {"moment_0": table.n_moments, "moments": table.n_moments,
                      "spectrum": table.n_bins}
        host = {name: eng.download(array) for name, array in self.state.items()}
        rows = {name: (eng.download(array) if array is not None else None)
                for name, array in (record or {}).items()}
        one = {name: eng.empty(1, FLOAT) for name in
               ("rhod", "thd", "qv", "prhod", "pthd", "pqv", "T", "p", "RH", "RH_max", "lv")}
        counters = {name: eng.empty(1, INT) for name in
                    ("n_substeps", "n_activating", "n_deactivating", "n_ripening")}
        success = eng.zeros(1, np.uint8)
        zero = eng.zeros(1, INT)
        most = int(np.diff(self.parcel_start_host).max())
        v_wet, backup = eng.empty(most, FLOAT), eng.empty(most, FLOAT)
        cell = eng.zeros(most, INT)
        identity = eng.upload(np.arange(most, dtype=np.int64))
        dt_range = (setup.dt_cond_range[0], min(setup.dt_cond_range[1], self.dt))
        n_parcel = self.n_parcel
        vent = self.ventilated
        if vent:  # include/sdm_parcel_vent.h
            air = {name: eng.empty(1, FLOAT) for name in
                   ("rho", "eta", "new_rho", "new_eta", "T", "p", "RH")}
            radius, velocity = eng.empty(most, FLOAT), eng.empty(most, FLOAT)
            law = self.terminal_velocity
            ranged = tv.law_name(law) == "GunnKinzer1949"  # (the closed forms have no range)
            stopped = eng.download(self.out_of_table)
        with_chem = self.chemistry is not None
        if with_chem:
            chem_cfg = abi.ChemistryCfg.from_buffer_copy(self.chem_cfg)
            chem_cfg.timestep = self.dt
            counts = eng.zeros(3, INT)
            chem_rows = {name: ([eng.download(a) for a in value] if isinstance(value, list)
                                else eng.download(value)) for name, value in chem_record.items()}
        for c in range(n_parcel):
            if host["failed_step"][c] >= 0:
                continue
            r0, r1 = (int(v) for v in self.parcel_start_host[c:c + 2])
            n = r1 - r0
            cell_start = eng.upload(np.array([0, n], dtype=np.int64))
            mass = self.water_mass[r0:r1]
            for k in range(w_mid.shape[0]):
                T, p = float(host["T"][c]), float(host["p"][c])
                rhod, thd, qv = (float(host[v][c]) for v in ("rhod", "thd", "qv"))
                w, dt = float(w_mid[k, c]), self.dt
                delta = float(host["qv_prev"][c]) - qv
                qv_mid = qv - delta / 2
                lv = self._latent_heat(T, one["lv"])
                Rq = const.Rv / (1 / qv_mid + 1) + const.Rd / (1 + qv_mid)
                cp = const.c_pv / (1 / qv_mid + 1) + const.c_pd / (1 + qv_mid)
                rho = p / Rq / T
                dql_dz = delta / w / dt
                drho_dz = (cfg.g_std / T * rho * (Rq / cp - 1)
                           - p * lv / cp / (T * T) * dql_dz) / Rq
                z = float(host["z"][c]) + dt * w
                prhod = rhod + dt * (w * drho_dz)
                dv = float(host["mass_of_dry_air"][c]) / ((prhod + rhod) / 2)
                for name, value in (("rhod", rhod), ("thd", thd), ("qv", qv), ("prhod", prhod),
                                    ("pthd", thd), ("pqv", qv), ("T", T)):
                    eng.fill(one[name], value)
                eng.fill(counters["n_substeps"], int(host["n_substeps"][c]))
                if vent:
                    # Moist.sync of this step: the pair the NEXT step reads, from the advanced
                    # rhod and the thd and qv of before this step's condensation
                    temperature_pressure_rh_call(eng, self.formulae, one["prhod"], one["thd"],
                                                 one["qv"], air["T"], air["p"], air["RH"], 1)
                    self._sync_air(air["new_rho"], air["new_eta"], one["prhod"], one["qv"],
                                   air["T"], 1)
                    self._radius(radius[:n], mass, n)
                    if ranged and self._largest_radius(radius[:n], n) > law.maximum_radius:
                        host["failed_step"][c] = host["steps_done"][c]
                        stopped[c] = 1
                        break
                    law.evaluate(eng, velocity[:n], radius[:n], n,
                                 *((False,) if ranged else ()))  # (check_range: done above)
                    eng.fill(air["rho"], float(host["air_density"][c]))
                    eng.fill(air["eta"], float(host["air_dynamic_viscosity"][c]))
                    eng.call_condensation("sdm_reynolds_number", self.reynolds_number[r0:r1],
                                          cell[:n], air["eta"], air["rho"], radius[:n],
                                          velocity[:n], n)
                eng.call("sdm_volume_of_water_mass", v_wet[:n], mass, n, float(const.rho_w))
                eng.assign(backup[:n], mass)
                critical_volume_call(eng, self.formulae, self.critical_volume[r0:r1],
                                     self.kappa[r0:r1], self.f_org[r0:r1],
                                     self.dry_volume[r0:r1], v_wet[:n], one["T"], cell[:n], n)
                condensation_call(
                    eng, formulae=self.formulae, n_sd=n, n_cell=1, cell_start=cell_start,
                    water_mass=mass, v_cr=self.critical_volume[r0:r1],
                    multiplicity=self.multiplicity[r0:r1], vdry=self.dry_volume[r0:r1],
                    idx=identity[:n], rhod=one["rhod"], thd=one["thd"],
                    water_vapour_mixing_ratio=one["qv"], dv=dv, prhod=one["prhod"],
                    pthd=one["pthd"], predicted_water_vapour_mixing_ratio=one["pqv"],
                    kappa=self.kappa[r0:r1], f_org=self.f_org[r0:r1], rtol_x=setup.rtol_x,
                    rtol_thd=setup.rtol_thd, timestep=dt, counters=counters, cell_order=zero,
                    RH_max=one["RH_max"], success=success,
                    reynolds_number=self.reynolds_number[r0:r1] if vent else None,
                    air_density=air["rho"] if vent else None,
                    air_dynamic_viscosity=air["eta"] if vent else None, dt_range=dt_range,
                    adaptive=setup.adaptive, fuse=setup.fuse, multiplier=setup.multiplier,
                    RH_rtol=setup.RH_rtol, max_iters=setup.max_iters, general=self.general,
                    descriptor=self.descriptor)
                if not eng.download(success)[0]:
                    eng.assign(mass, backup[:n])
                    host["failed_step"][c] = host["steps_done"][c]
                    break
                temperature_pressure_rh_call(eng, self.formulae, one["prhod"], one["pthd"],
                                             one["pqv"], one["T"], one["p"], one["RH"], 1)
                n_sub = int(eng.download(counters["n_substeps"])[0])
                if setup.adaptive:  # dynamics/condensation.py:122-131
                    n_sub = min(max(n_sub, int(cfg.n_clamp_lo)), int(cfg.n_clamp_hi))
                host["qv_prev"][c] = qv
                host["z"][c], host["rhod"][c] = z, prhod
                host["thd"][c] = eng.download(one["pthd"])[0]
                host["qv"][c] = eng.download(one["pqv"])[0]
                for name in ("T", "p", "RH", "RH_max"):
                    host[name][c] = eng.download(one[name])[0]
                host["n_substeps"][c] = n_sub
                for name in ("n_activating", "n_deactivating", "n_ripening"):
                    host[name][c] = eng.download(counters[name])[0]
                host["steps_done"][c] += 1
                if vent:
                    host["air_density"][c] = eng.download(air["new_rho"])[0]
                    host["air_dynamic_viscosity"][c] = eng.download(air["new_eta"])[0]
                for name, row in rows.items():
                    if row is not None:
                        row[k * n_parcel + c] = host[name][c]
                if with_chem:  # points 2-5 of include/sdm_parcel_chem.h with the stage symbols
                    at = k * n_parcel + c
                    chem_cfg.cell_volume = dv
                    ratios = [mr[c:c + 1] for mr in self.mixing_ratios]
                    eng.call("sdm_volume_of_water_mass", v_wet[:n], mass, n, float(const.rho_w))
                    eng.call_chemistry(
                        "sdm_chemistry_step", chem_cfg, n, 1, identity[:n], cell_start, cell[:n],
                        self.multiplicity[r0:r1], v_wet[:n], [m[r0:r1] for m in self.moles],
                        self.pH[r0:r1], self.do_chemistry_flag[r0:r1], one["T"], one["p"],
                        one["prhod"], ratios, counts, self.chem_consts)
                    for counter, count in zip(self.chem_counters, eng.download(counts)):
                        counter[c:c + 1] += int(count)
                    sulphate = self.moles[chem.AQUEOUS.index("S_VI")][r0:r1]
                    eng.assign(self.dry_volume[r0:r1], sulphate * self.dry_factor)
                    eng.assign(self.kappa[r0:r1],
                               self.kappa_times_dry_volume[r0:r1] / self.dry_volume[r0:r1])
                    mult = eng.download(self.multiplicity[r0:r1])
                    for g in range(6):
                        chem_rows["mixing_ratio"][g][at] = eng.download(ratios[g])[0]
                    for a in range(7):
                        chem_rows["aq_total"][a][at] = diag_sum(
                            mult, eng.download(self.moles[a][r0:r1]))
                    chem_rows["n_flagged"][at] = int(np.count_nonzero(
                        eng.download(self.do_chemistry_flag[r0:r1])))
                    chem_rows["dv"][at] = dv
                if table is not None:
                    at = k * n_parcel + c
                    diagnose_call(eng, self.formulae, requests, parcel_start=cell_start,
                                  water_mass=mass, multiplicity=self.multiplicity[r0:r1],
                                  dry_volume=self.dry_volume[r0:r1], kappa=self.kappa[r0:r1],
                                  f_org=self.f_org[r0:r1], T=one["T"], diag=one_diag,
                                  descriptor=self.descriptor, general=self.general)
                    diag_rows["dv"][at] = dv
                    for name, array in one_diag.items():
                        width = widths[name]
                        diag_rows[name][at * width:(at + 1) * width] = eng.download(array)
        for name, row in diag_rows.items():
            eng.assign(diag[name], eng.upload(row))
        if with_chem:
            for name, value in chem_rows.items():
                for dst, src in (zip(chem_record[name], value) if isinstance(value, list)
                                 else ((chem_record[name], value),)):
                    eng.assign(dst, eng.upload(src))
        for name, array in self.state.items():
            eng.assign(array, eng.upload(host[name]))
        if vent:
            eng.assign(self.out_of_table, eng.upload(stopped))
        for name, row in rows.items():
            if row is not None:
                eng.assign(record[name], eng.upload(row))

    # ---- state --------------------------------------------------------------------------------------
    def snapshot(self):
        """host copies of everything a later `restore` needs: the parcels' state arrays, the
        per-droplet water masses and critical volumes, and the clock of w(t); with chemistry also
        the dry volumes, kappa, the seven amounts, pH, the flag, the mixing ratios and the three
        counters"""
        down = self.engine.download
        out = {name: down(array) for name, array in self.state.items()}
        out["water_mass"] = down(self.water_mass)
        out["critical_volume"] = down(self.critical_volume)
        out["n_steps"] = self.n_steps
        if self.ventilated:  # (the carried air pair is among the state arrays)
            out["reynolds_number"] = down(self.reynolds_number)
            out["out_of_table"] = down(self.out_of_table)
        if self.chemistry is not None:
            out.update(self._chem_columns(down))
        if self.ice is not None:  # (the carried pair is among the state arrays)
            out.update(self.ice.columns(down))
        if self.collisions is not None:
            out.update(self._coal_columns(down))
            # (positions past a parcel's live ones hold nothing that is defined)
            position = np.arange(self.n_sd) - np.repeat(self.parcel_start_host[:-1],
                                                        np.diff(self.parcel_start_host))
            out["idx"] = np.where(position < np.repeat(out["n_live"],
                                                       np.diff(self.parcel_start_host)),
                                  out["idx"], -1)
        return out

    def _chem_columns(self, get=lambda array: array):
        """the columns chemistry adds to a snapshot, by name (`get` applied to every array)"""
        out = {"dry_volume": get(self.dry_volume), "kappa": get(self.kappa), "pH": get(self.pH),
               "do_chemistry_flag": get(self.do_chemistry_flag)}
        out.update({f"moles_{key}": get(array) for key, array in zip(chem.AQUEOUS, self.moles)})
        out.update({f"mixing_ratio_{gas}": get(array)
                    for gas, array in zip(chem.GASES, self.mixing_ratios)})
        out.update({name: get(array) for name, array in zip(CHEM_COUNTERS, self.chem_counters)})
        return out

    def restore(self, state):
        """sets the state to a given one (a `snapshot`, or any dict with some of its entries):
        qv_prev, the counters, steps_done and failed_step included.  Where rhod, thd or qv are given
        without T, p and RH, these are recomputed from them (`sdm_temperature_pressure_rh`)"""
        eng = self.engine
        for name, value in state.items():
            if name == "n_steps":
                self.n_steps = int(value)
                continue
            columns = {"water_mass": self.water_mass, "critical_volume": self.critical_volume}
            if self.ventilated:
                columns.update(reynolds_number=self.reynolds_number,
                               out_of_table=self.out_of_table)
            if self.chemistry is not None:
                columns.update(self._chem_columns())
            if self.ice is not None:
                columns.update(self.ice.columns())
            if self.collisions is not None:
                columns.update(self._coal_columns())
                if name in ("idx", "n_live"):
                    self._fresh_idx = True
            target = columns.get(name, self.state.get(name))
            if target is None:
                raise KeyError(name)
            dtype = INT if name in _INT_FIELDS + CHEM_COUNTERS + COAL_COUNTERS + _COAL_INTS else \
                np.uint8 if name == "do_chemistry_flag" else FLOAT
            value = np.ascontiguousarray(np.broadcast_to(
                np.asarray(value, dtype=dtype), (eng.size(target),)))
            eng.assign(target, eng.upload(value))
        if {"rhod", "thd", "qv"} & set(state) and not {"T", "p", "RH"} & set(state):
            temperature_pressure_rh_call(eng, self.formulae, self.state["rhod"],
                                         self.state["thd"], self.state["qv"], self.state["T"],
                                         self.state["p"], self.state["RH"], self.n_parcel,
                                         mixed_phase=self.mixed_phase)
        failed = eng.download(self.state["failed_step"])
        self._reported = {int(p) for p in np.flatnonzero(failed >= 0)}

"""The mixed-phase parcel on the library (include/sdm_parcel_ice.h, where the time step and the
timing of what the ice passes read are written out): what `ParcelRunner(freezing=...,
deposition=...)` adds to the adiabatic parcel.

PySDM's `Parcel(mixed_phase=True)` with the dynamics `AmbientThermodynamics`, `Condensation`, then
`Freezing` and / or `VapourDepositionOnIce` in either order.  `route="fused"` is one
`sdm_parcel_run_ice` call: the ice passes run inside the kernel's step loop.  `route="stages"` is
the yardstick: per parcel and step it chains the stage symbols `sdm_temperature_pressure_rh(_f)`,
`sdm_a_w_ice`, `sdm_critical_volume(_f)` (copied back for the liquid rows only),
`sdm_condensation(_f)`, `sdm_freezing_step` and `sdm_deposition` on the parcel's slice, with
several read-backs per step.

The particle shape is MixedPhaseSpheres (the mass column is the signed water mass); the options
the condensation solver reads must be PySDM's defaults but the diffusion coordinate, which the
deposition shares ("WaterMass" goes through the general kernel).  Every parcel draws from its own
NumPy-PCG64 stream (`ice_seed`: an int, or one per parcel).
"""
import numpy as np

from . import abi
from . import deposition as dep
from . import freezing as frz
from .condensation import (condensation_call, constants_of, critical_volume_call, descriptor_of,
                           temperature_pressure_rh_call)
from .engine import FLOAT, INT

STATE = ("a_w_ice", "RH_ice")                      # per parcel, carried from step to step
COUNTERS = ("rng_offset", "n_exceeded")            # per parcel, int64
COLUMNS = ("freezing_temperature", "immersed_surface_area", "temperature_of_last_freezing")
_PROFILE_INTS = ("n_ice", "n_exceeded")


def _name(value):
    return value if isinstance(value, str) else getattr(value, "__name__", type(value).__name__)


def descriptor(formulae):
    """the condensation descriptor of mixed-phase formulae: PySDM's defaults (checked) with the
    formulae's diffusion coordinate"""
    constants_of(formulae, mixed_phase=True)
    return descriptor_of({"diffusion_coordinate": _name(formulae.diffusion_coordinate)},
                         formulae.constants)


class IceParcel:  # pylint: disable=too-many-instance-attributes
    """the ice part of a `ParcelRunner`: configuration, the carried state, the per-row columns"""

    def __init__(self, runner, *, freezing, deposition, order, seed, freezing_temperature,
                 immersed_surface_area):
        eng, formulae = runner.engine, runner.formulae
        n_parcel, n_sd = runner.n_parcel, runner.n_sd
        if freezing is None and not deposition:
            raise ValueError("a mixed-phase parcel needs freezing= or deposition=")
        if order not in abi.PARCEL_ICE_ORDERS:
            raise NotImplementedError(
                f"ice_order={order!r}: one of {sorted(abi.PARCEL_ICE_ORDERS)}")
        if runner.route == "fused" and eng.parcel_ice_library is None:
            raise NotImplementedError(
                f"engine `{eng.name}` has no library for the mixed-phase parcel: route='fused' "
                "is not available on it (route='stages' is)")
        self.setup = freezing
        self.deposition = bool(deposition)
        self.sum = deposition.get("sum", "ordered") if isinstance(deposition, dict) else "ordered"
        self.order = order
        frz.check_formulae(formulae)
        cfg = self.cfg = abi.ParcelIceCfg()
        cfg.order = abi.PARCEL_ICE_ORDERS[order]
        self.stochastic = 0
        if freezing is not None:
            cfg.freezing = 1
            cfg.singular, cfg.thaw = int(freezing.singular), int(freezing.thaw)
            cfg.immersion_freezing = int(freezing.immersion_freezing)
            cfg.homogeneous_freezing = int(freezing.homogeneous_freezing)
            time_dependent = freezing.immersion_freezing and not freezing.singular
            cfg.j_het = frz.j_het_code(formulae) if time_dependent else 0
            cfg.j_hom = frz.j_hom_code(formulae) if freezing.homogeneous_freezing else 0
            self.stochastic = freezing.n_stochastic_passes
        if self.deposition:
            one = dep.deposition_cfg(formulae, runner.dt, 1.0, self.sum)
            cfg.deposition = 1
            cfg.coordinate, cfg.capacity = one.coordinate, one.capacity
            cfg.kinetics, cfg.sum = one.kinetics, one.sum
        self.frz_consts = frz.constants_of(formulae)
        self.dep_consts = dep.constants_of(formulae)

        def column(values, what, needed):
            if not needed:
                return None
            if values is None:
                raise ValueError(f"this Freezing setup needs `{what}`")
            out = np.ascontiguousarray(values, dtype=float).reshape(-1)
            if out.size != n_sd:
                raise ValueError(f"{what} must hold sum(counts) = {n_sd} values")
            return eng.upload(out)

        on = freezing is not None and freezing.immersion_freezing
        self.freezing_temperature = column(freezing_temperature, "freezing_temperature",
                                           on and freezing.singular)
        self.immersed_surface_area = column(immersed_surface_area, "immersed_surface_area",
                                            on and not freezing.singular)
        self.temperature_of_last_freezing = (
            eng.full(n_sd, FLOAT, np.nan)
            if freezing is not None and freezing.record_freezing_temperature else None)
        seeds = np.broadcast_to(np.asarray(formulae.seed if seed is None else seed), (n_parcel,))
        self.seed_words = np.array([abi.pcg64_state_inc(int(s)) for s in seeds], dtype=np.uint64)
        self.rng_state_inc = eng.upload(self.seed_words.reshape(-1).view(np.int64).copy())
        self.rng_offset = eng.zeros(n_parcel, INT)
        self.n_exceeded = eng.zeros(n_parcel, INT)
        # Parcel.register -> Moist.sync: the pair of the initial state
        state = runner.state
        state.update({name: eng.empty(n_parcel, FLOAT) for name in STATE})
        eng.call_freezing("sdm_a_w_ice", state["T"], state["p"], state["RH"], state["qv"],
                          state["a_w_ice"], state["RH_ice"], n_parcel, self.frz_consts)
        self.last_profile = None

    # ---- what a snapshot carries ------------------------------------------------------------
    def columns(self, get=lambda array: array):
        out = {"rng_offset": get(self.rng_offset), "n_exceeded": get(self.n_exceeded)}
        if self.temperature_of_last_freezing is not None:
            out["temperature_of_last_freezing"] = get(self.temperature_of_last_freezing)
        return out

    def record(self, engine, n_rows):
        return {name: engine.full(n_rows, INT, -1) if name in _PROFILE_INTS
                else engine.full(n_rows, FLOAT, np.nan) for name in abi.PARCEL_ICE_PROFILE_FIELDS}

    # ---- route="fused" --------------------------------------------------------------------------
    def run_fused(self, runner, n_steps, w_mid, record, ice_record):
        from .parcel import CONSTANT_NAMES, _INT_FIELDS, _address  # pylint: disable=import-outside-toplevel

        eng, n_parcel = runner.engine, runner.n_parcel
        c_state = abi.ParcelState()
        for name in abi.PARCEL_STATE_FIELDS:
            setattr(c_state, name,
                    _address(runner.state[name], INT if name in _INT_FIELDS else FLOAT))
        c_profile = None
        if record is not None:
            c_profile = abi.ParcelProfile()
            for name in abi.PARCEL_PROFILE_FIELDS:
                setattr(c_profile, name, _address(record.get(name),
                                                  INT if name.startswith("n_") else FLOAT))
        ice_state = abi.ParcelIceState()
        ice_state.a_w_ice = _address(runner.state["a_w_ice"], FLOAT)
        ice_state.RH_ice = _address(runner.state["RH_ice"], FLOAT)
        ice_state.rng_offset = _address(self.rng_offset, INT)
        ice_state.rng_state_inc = _address(self.rng_state_inc, INT)
        ice_state.n_exceeded = _address(self.n_exceeded, INT)
        for name in COLUMNS:
            setattr(ice_state, name, _address(getattr(self, name), FLOAT))
        ice_profile = abi.ParcelIceProfile()
        for name in abi.PARCEL_ICE_PROFILE_FIELDS:
            array = ice_record[name]
            if eng.size(array) != n_steps * n_parcel:
                raise ValueError(f"parcel: ice profile[{name!r}] must hold n_steps x n_parcel")
            setattr(ice_profile, name, _address(array, INT if name in _PROFILE_INTS else FLOAT))
        consts = [float(getattr(runner.formulae.constants, name)) for name in CONSTANT_NAMES]
        default = not any(runner.descriptor.option) and not runner.general
        eng.call_parcel_ice(
            "sdm_parcel_run_ice", runner.cfg, self.cfg, int(n_steps), n_parcel, runner.n_sd,
            runner.parcel_start, runner.water_mass, runner.multiplicity, runner.dry_volume,
            runner.kappa, runner.f_org, runner.critical_volume, c_state,
            eng.upload(w_mid.reshape(-1)), c_profile, consts,
            None if default else runner.descriptor, ice_state, ice_profile, self.frz_consts,
            self.dep_consts)

    # ---- route="stages" -------------------------------------------------------------------------
    def run_stages(self, runner, w_mid, record, ice_record):  # pylint: disable=too-many-locals,too-many-statements
        """the time step of include/sdm_parcel_ice.h with the stage symbols, parcel after parcel"""
        from .parcel import diag_sum  # pylint: disable=import-outside-toplevel

        eng, formulae = runner.engine, runner.formulae
        const, cfg, setup = formulae.constants, runner.cfg, runner.setup
        host = {name: eng.download(array) for name, array in runner.state.items()}
        rows = {name: eng.download(array) for name, array in (record or {}).items()}
        ice_rows = {name: eng.download(array) for name, array in ice_record.items()}
        offsets = eng.download(self.rng_offset).view(np.uint64)
        n_exceeded = eng.download(self.n_exceeded)
        one = {name: eng.empty(1, FLOAT) for name in
               ("rhod", "thd", "qv", "prhod", "pthd", "pqv", "T", "p", "RH", "RH_max", "lv",
                "sync_T", "sync_p", "sync_RH", "new_a_w_ice", "new_RH_ice", "a_w_ice", "RH_ice",
                "cur_T", "cur_p", "cur_RH")}
        counters = {name: eng.empty(1, INT) for name in
                    ("n_substeps", "n_activating", "n_deactivating", "n_ripening")}
        success, zero, exceeded = eng.zeros(1, np.uint8), eng.zeros(1, INT), eng.zeros(1, INT)
        most = int(np.diff(runner.parcel_start_host).max())
        v_wet, backup, v_cr = (eng.empty(most, FLOAT) for _ in range(3))
        cell = eng.zeros(most, INT)
        identity = eng.upload(np.arange(most, dtype=np.int64))
        dt_range = (setup.dt_cond_range[0], min(setup.dt_cond_range[1], runner.dt))
        n_parcel, dt = runner.n_parcel, runner.dt
        frz_cfg = None
        if self.setup is not None:
            frz_cfg = frz.freezing_cfg(self.setup, formulae, dt, 0)
        dep_cfg = dep.deposition_cfg(formulae, dt, 1.0, self.sum) if self.deposition else None
        passes = ("freezing", "deposition") if self.order == "freezing_first" else (
            "deposition", "freezing")
        for c in range(n_parcel):
            if host["failed_step"][c] >= 0:
                continue
            r0, r1 = (int(v) for v in runner.parcel_start_host[c:c + 2])
            n = r1 - r0
            cell_start = eng.upload(np.array([0, n], dtype=np.int64))
            mass = runner.water_mass[r0:r1]
            mult = runner.multiplicity[r0:r1]
            if frz_cfg is not None:
                frz_cfg.rng_state_inc[:] = [int(word) for word in self.seed_words[c]]
            for k in range(w_mid.shape[0]):
                T, p, RH = (float(host[v][c]) for v in ("T", "p", "RH"))
                rhod, thd, qv = (float(host[v][c]) for v in ("rhod", "thd", "qv"))
                w = float(w_mid[k, c])
                delta = float(host["qv_prev"][c]) - qv
                qv_mid = qv - delta / 2
                lv = runner._latent_heat(T, one["lv"])  # pylint: disable=protected-access
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
                                    ("pthd", thd), ("pqv", qv), ("T", T), ("cur_T", T),
                                    ("cur_p", p), ("cur_RH", RH),
                                    ("a_w_ice", float(host["a_w_ice"][c])),
                                    ("RH_ice", float(host["RH_ice"][c]))):
                    eng.fill(one[name], value)
                eng.fill(counters["n_substeps"], int(host["n_substeps"][c]))
                # Moist.sync of this step: the pair the NEXT step reads
                temperature_pressure_rh_call(eng, formulae, one["prhod"], one["thd"], one["qv"],
                                             one["sync_T"], one["sync_p"], one["sync_RH"], 1,
                                             mixed_phase=True)
                eng.call_freezing("sdm_a_w_ice", one["sync_T"], one["sync_p"], one["sync_RH"],
                                  one["qv"], one["new_a_w_ice"], one["new_RH_ice"], 1,
                                  self.frz_consts)
                # the critical volume, copied back for the liquid rows only
                eng.call("sdm_volume_of_water_mass", v_wet[:n], mass, n, float(const.rho_w))
                eng.assign(backup[:n], mass)
                critical_volume_call(eng, formulae, v_cr[:n], runner.kappa[r0:r1],
                                     runner.f_org[r0:r1], runner.dry_volume[r0:r1], v_wet[:n],
                                     one["T"], cell[:n], n, mixed_phase=True)
                liquid = eng.download(mass) > 0
                eng.assign(runner.critical_volume[r0:r1], eng.upload(np.where(
                    liquid, eng.download(v_cr[:n]), eng.download(runner.critical_volume[r0:r1]))))
                condensation_call(
                    eng, formulae=formulae, n_sd=n, n_cell=1, cell_start=cell_start,
                    water_mass=mass, v_cr=runner.critical_volume[r0:r1], multiplicity=mult,
                    vdry=runner.dry_volume[r0:r1], idx=identity[:n], rhod=one["rhod"],
                    thd=one["thd"], water_vapour_mixing_ratio=one["qv"], dv=dv,
                    prhod=one["prhod"], pthd=one["pthd"],
                    predicted_water_vapour_mixing_ratio=one["pqv"], kappa=runner.kappa[r0:r1],
                    f_org=runner.f_org[r0:r1], rtol_x=setup.rtol_x, rtol_thd=setup.rtol_thd,
                    timestep=dt, counters=counters, cell_order=zero, RH_max=one["RH_max"],
                    success=success, reynolds_number=None, air_density=None,
                    air_dynamic_viscosity=None, dt_range=dt_range, adaptive=setup.adaptive,
                    fuse=setup.fuse, multiplier=setup.multiplier, RH_rtol=setup.RH_rtol,
                    max_iters=setup.max_iters, general=runner.general,
                    descriptor=runner.descriptor)
                if not eng.download(success)[0]:
                    eng.assign(mass, backup[:n])
                    host["failed_step"][c] = host["steps_done"][c]
                    break
                # T, p, RH of the state after the condensation alone
                temperature_pressure_rh_call(eng, formulae, one["prhod"], one["pthd"],
                                             one["pqv"], one["T"], one["p"], one["RH"], 1,
                                             mixed_phase=True)
                step_exceeded = 0
                for which in passes:
                    if which == "freezing" and frz_cfg is not None:
                        last = self.temperature_of_last_freezing
                        eng.call_freezing(
                            "sdm_freezing_step", frz_cfg, int(offsets[c]), n, 1, mass,
                            None if self.freezing_temperature is None
                            else self.freezing_temperature[r0:r1],
                            None if self.immersed_surface_area is None
                            else self.immersed_surface_area[r0:r1], None, cell[:n],
                            None if last is None else last[r0:r1], one["cur_T"], one["cur_RH"],
                            one["a_w_ice"], one["RH_ice"], self.frz_consts)
                        offsets[c] += np.uint64(n * self.stochastic)
                    elif which == "deposition" and dep_cfg is not None:
                        dep_cfg.cell_volume = dv
                        eng.call_deposition(
                            "sdm_deposition", dep_cfg, n, 1, mult, mass, cell[:n], one["cur_T"],
                            one["cur_p"], one["cur_RH"], one["a_w_ice"], one["qv"], one["rhod"],
                            one["thd"], one["pqv"], one["pthd"], exceeded, self.dep_consts)
                        step_exceeded = int(eng.download(exceeded)[0])
                n_exceeded[c] += step_exceeded
                n_sub = int(eng.download(counters["n_substeps"])[0])
                if setup.adaptive:  # dynamics/condensation.py:122-131
                    n_sub = min(max(n_sub, int(cfg.n_clamp_lo)), int(cfg.n_clamp_hi))
                host["qv_prev"][c] = qv
                host["z"][c], host["rhod"][c] = z, prhod
                host["thd"][c] = eng.download(one["pthd"])[0]
                host["qv"][c] = eng.download(one["pqv"])[0]
                for name in ("T", "p", "RH", "RH_max"):
                    host[name][c] = eng.download(one[name])[0]
                host["a_w_ice"][c] = eng.download(one["new_a_w_ice"])[0]
                host["RH_ice"][c] = eng.download(one["new_RH_ice"])[0]
                host["n_substeps"][c] = n_sub
                for name in ("n_activating", "n_deactivating", "n_ripening"):
                    host[name][c] = eng.download(counters[name])[0]
                host["steps_done"][c] += 1
                at = k * n_parcel + c
                for name, row in rows.items():
                    row[at] = host[name][c]
                m_now, mult_host = eng.download(mass), eng.download(mult)
                ice = m_now < 0
                ice_rows["a_w_ice"][at] = host["a_w_ice"][c]
                ice_rows["RH_ice"][at] = host["RH_ice"][c]
                ice_rows["n_ice"][at] = int(mult_host[ice].sum())
                ice_rows["ice_mass"][at] = diag_sum(mult_host, np.where(ice, -m_now, 0.0))
                ice_rows["n_exceeded"][at] = step_exceeded
                ice_rows["dv"][at] = dv
        for name, array in runner.state.items():
            eng.assign(array, eng.upload(host[name]))
        eng.assign(self.rng_offset, eng.upload(offsets.view(np.int64)))
        eng.assign(self.n_exceeded, eng.upload(n_exceeded))
        for name, row in rows.items():
            eng.assign(record[name], eng.upload(row))
        for name, row in ice_rows.items():
            eng.assign(ice_record[name], eng.upload(row))

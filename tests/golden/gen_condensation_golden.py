#!/usr/bin/env python3
"""Generates the condensation goldens (tests/golden/cond_*.npz) by RUNNING THE REFERENCE (PySDM at
/root/reference) in its pure-Python mode, with the same no-JIT import as gen_golden.py (the
stand-ins of tests/golden/standins put in front of it).  Run as:

    PYTHONDONTWRITEBYTECODE=1 CI=1 python3 -B tests/golden/gen_condensation_golden.py

Written:
  cond_parcel_a1.npz / cond_parcel_a0.npz  a `Parcel` ascent with `AmbientThermodynamics()` +
      `Condensation(adaptive=...)` on a lognormal aerosol; every `backend.condensation` call is
      recorded: its arguments (state and ambient values in) and what the reference left behind
      (water mass, predicted thd / water vapour mixing ratio, counters, RH_max, success out).
  cond_box.npz  a 4 x 4-cell box with different rhod / thd / qv per cell and prescribed predicted
      values (cell_order, empty cells, per-cell n_substeps), a few calls in a row.
  cond_ambient.npz  elementwise cases of the six ambient methods.
"""
# pylint: disable=wrong-import-position,import-error,too-many-locals,protected-access
import os
import sys

os.environ.setdefault("CI", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "standins"), "/root/reference"]

import numpy as np

from PySDM import Builder, Formulae
from PySDM.backends import CPU
from PySDM.dynamics import AmbientThermodynamics, Condensation
from PySDM.environments import Parcel
from PySDM.initialisation import spectra
from PySDM.initialisation.sampling.spectral_sampling import ConstantMultiplicity
from PySDM.physics import si

OUT = HERE
STATE_IN = ("water_mass", "v_cr")
CONSTANT_IN = ("multiplicity", "vdry", "kappa", "f_org", "idx", "cell_start_arg", "cell_id",
               "reynolds_number")
CELL_IN = ("rhod", "thd", "water_vapour_mixing_ratio", "prhod", "pthd",
           "predicted_water_vapour_mixing_ratio", "air_density", "air_dynamic_viscosity")
COUNTERS = ("n_substeps", "n_activating", "n_deactivating", "n_ripening")


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


def _host(value):
    while hasattr(value, "data") and not isinstance(value, np.ndarray):
        value = value.data  # attribute -> Storage -> ndarray
    return np.array(value, copy=True)


class Recorder:
    """wraps `backend.condensation` / `make_condensation_solver` and keeps every call"""

    def __init__(self, backend):
        self.calls = []
        self.solver_args = None
        inner_make, inner = backend.make_condensation_solver, backend.condensation

        def make(timestep, n_cell, **kwargs):
            self.solver_args = dict(timestep=timestep, n_cell=n_cell, **kwargs)
            return inner_make(timestep, n_cell, **kwargs)

        def condensation(**kwargs):
            before = {k: _host(kwargs[k]) for k in STATE_IN + CONSTANT_IN + CELL_IN}
            before.update({f"in_{k}": _host(kwargs["counters"][k]) for k in COUNTERS})
            before.update(dv=float(kwargs["dv"]), timestep=float(kwargs["timestep"]),
                          rtol_x=float(kwargs["rtol_x"]), rtol_thd=float(kwargs["rtol_thd"]),
                          cell_order=np.asarray(kwargs["cell_order"], dtype=np.int64))
            inner(**kwargs)
            after = {f"out_{k}": _host(kwargs["counters"][k]) for k in COUNTERS}
            after.update(out_water_mass=_host(kwargs["water_mass"]),
                         out_pthd=_host(kwargs["pthd"]),
                         out_predicted_water_vapour_mixing_ratio=_host(
                             kwargs["predicted_water_vapour_mixing_ratio"]),
                         out_RH_max=_host(kwargs["RH_max"]),
                         out_success=_host(kwargs["success"]).astype(np.int64))
            self.calls.append({**before, **after})

        backend.make_condensation_solver = make
        backend.condensation = condensation


def _pack(recorder, extra):
    calls = recorder.calls
    arrays = dict(extra)
    for key in CONSTANT_IN:  # the parcel run never changes these: stored once
        for call in calls:
            np.testing.assert_array_equal(call[key], calls[0][key])
        arrays[key] = calls[0][key]
    varying = [k for k in calls[0] if k not in CONSTANT_IN]
    for key in varying:
        arrays[f"calls/{key}"] = np.stack([np.asarray(c[key]) for c in calls])
    for key in ("dt_range",):
        arrays[f"solver/{key}"] = np.asarray(recorder.solver_args[key], dtype=float)
    for key in ("adaptive", "fuse", "multiplier", "max_iters"):
        arrays[f"solver/{key}"] = np.asarray(int(recorder.solver_args[key]))
    arrays["solver/RH_rtol"] = np.asarray(float(recorder.solver_args["RH_rtol"]))
    arrays["solver/timestep"] = np.asarray(float(recorder.solver_args["timestep"]))
    arrays["n_calls"] = np.asarray(len(calls))
    return arrays


PARCEL = dict(n_sd=192, n_steps=40, dt=1 * si.s, mass_of_dry_air=1 * si.kg, p0=1000 * si.hPa,
              qv0=12 * si.g / si.kg, T0=290 * si.K, w=5 * si.m / si.s, kappa=1.28,
              spectrum=(60 / si.cm ** 3, 0.04 * si.um, 1.4))


def parcel(adaptive):
    cfg = PARCEL
    formulae = Formulae()
    backend = CPU(formulae)
    recorder = Recorder(backend)
    env = Parcel(dt=cfg["dt"], mass_of_dry_air=cfg["mass_of_dry_air"], p0=cfg["p0"],
                 initial_water_vapour_mixing_ratio=cfg["qv0"], T0=cfg["T0"], w=cfg["w"])
    builder = Builder(n_sd=cfg["n_sd"], backend=backend, environment=env)
    builder.add_dynamic(AmbientThermodynamics())
    builder.add_dynamic(Condensation(adaptive=adaptive))
    norm, mode, sigma = cfg["spectrum"]
    spectrum = spectra.Lognormal(norm_factor=norm, m_mode=mode, s_geom=sigma)
    r_dry, n_per_volume = ConstantMultiplicity(spectrum).sample(cfg["n_sd"])
    attributes = builder.particulator.environment.init_attributes(
        n_in_dv=n_per_volume * builder.particulator.environment.mesh.dv, kappa=cfg["kappa"],
        r_dry=r_dry)
    particulator = builder.build(attributes=attributes, products=())
    initial = {k: np.asarray(v) for k, v in attributes.items()}
    for _ in range(cfg["n_steps"]):
        particulator.run(steps=1)
    arrays = _pack(recorder, {f"init/{k}": v for k, v in initial.items()})
    arrays.update({f"parcel/{k}": np.asarray(v, dtype=float)
                   for k, v in cfg.items() if k != "spectrum"})
    arrays["parcel/spectrum"] = np.asarray(cfg["spectrum"], dtype=float)
    act = arrays["calls/out_n_activating"]
    assert act.max() > 0, "no activation recorded"
    print(f"parcel adaptive={adaptive}: n_activating max {act.max()}, n_substeps "
          f"{arrays['calls/out_n_substeps'].ravel().tolist()}")
    save(f"cond_parcel_a{int(adaptive)}", **arrays)


def box():
    """4 x 4 cells, prescribed ambient state and predictions, calls straight on the backend"""
    rng = np.random.default_rng(20261016)
    formulae = Formulae()
    backend = CPU(formulae)
    n_cell, dt = 16, 2.0
    counts = rng.integers(1, 40, n_cell)
    counts[[3, 10]] = 0  # empty cells
    n_sd = int(counts.sum())
    cell_id = np.repeat(np.arange(n_cell), counts)
    perm = rng.permutation(n_sd)
    cell_id = cell_id[perm]
    idx = np.argsort(cell_id, kind="stable").astype(np.int64)
    cell_start = np.zeros(n_cell + 1, dtype=np.int64)
    cell_start[1:] = np.cumsum(np.bincount(cell_id, minlength=n_cell))
    const = formulae.constants
    r_dry = np.exp(rng.uniform(np.log(0.01e-6), np.log(0.5e-6), n_sd))
    vdry = const.PI_4_3 * r_dry ** 3
    kappa = rng.uniform(0.2, 1.3, n_sd)
    f_org = np.zeros(n_sd)
    multiplicity = rng.integers(1, 10 ** 9, n_sd).astype(np.int64)
    multiplicity[5] = 0
    r_wet = r_dry * rng.uniform(1.5, 20, n_sd)
    r_wet[rng.uniform(size=n_sd) < 0.1] *= 50
    water_mass = const.rho_w * const.PI_4_3 * r_wet ** 3
    water_mass[7] = 0.0
    water_mass[11] = -water_mass[11]
    rhod = rng.uniform(1.0, 1.2, n_cell)
    thd = rng.uniform(285, 300, n_cell)
    qv = rng.uniform(0.006, 0.014, n_cell)
    # saturate: RH close to 1 in every cell, so that growth / evaporation both appear
    T = formulae.state_variable_triplet.T(rhod, thd)
    p = formulae.state_variable_triplet.p(rhod, T, qv)
    pvs = formulae.saturation_vapour_pressure.pvs_water(T)
    target_rh = rng.uniform(0.97, 1.01, n_cell)
    pv = target_rh * pvs
    qv = const.eps * pv / (p - pv)
    prhod = rhod * (1 + rng.uniform(-2e-4, 0, n_cell))
    pthd = thd + rng.uniform(-0.05, 0.05, n_cell) * 10.0 ** rng.integers(0, 3, n_cell)
    pqv = qv * (1 + rng.uniform(-5e-4, 5e-4, n_cell) * 10.0 ** rng.integers(0, 3, n_cell))
    air_density = rhod * (1 + qv)
    eta = formulae.air_dynamic_viscosity.eta_air(T)
    v_cr = np.empty(n_sd)
    for i in range(n_sd):
        T_i = T[cell_id[i]]
        v_cr[i] = formulae.trivia.volume(formulae.hygroscopicity.r_cr(
            kappa[i], vdry[i] / const.PI_4_3, T_i, const.sgm_w))
    S = backend.Storage
    calls = []
    for adaptive in (True, False):
        solver_args = dict(dt_range=(1e-4, dt), adaptive=adaptive, fuse=32, multiplier=2,
                           RH_rtol=1e-7, max_iters=16)
        solver = backend.make_condensation_solver(dt, n_cell, **solver_args)
        st = {k: S.from_ndarray(np.array(v)) for k, v in dict(
            water_mass=water_mass, v_cr=v_cr, multiplicity=multiplicity, vdry=vdry,
            kappa=kappa, f_org=f_org, idx=idx, cell_start_arg=cell_start, cell_id=cell_id,
            reynolds_number=np.zeros(n_sd), rhod=rhod, thd=thd, water_vapour_mixing_ratio=qv,
            prhod=prhod, pthd=pthd.copy(), predicted_water_vapour_mixing_ratio=pqv.copy(),
            air_density=air_density, air_dynamic_viscosity=eta).items()}
        counters = {k: S.from_ndarray(np.full(n_cell, -1 if adaptive or k != "n_substeps"
                                              else 3, dtype=np.int64)) for k in COUNTERS}
        RH_max = S.from_ndarray(np.full(n_cell, np.nan))
        success = S.from_ndarray(np.zeros(n_cell, dtype=bool))
        for _ in range(3):
            cell_order = np.argsort(counters["n_substeps"].to_ndarray())
            rec = {k: _host(st[k]) for k in STATE_IN + CONSTANT_IN + CELL_IN}
            rec.update({f"in_{k}": _host(counters[k]) for k in COUNTERS})
            rec.update(cell_order=cell_order.astype(np.int64), adaptive=int(adaptive))
            backend.condensation(
                solver=solver, n_cell=n_cell, cell_start_arg=st["cell_start_arg"],
                water_mass=st["water_mass"], multiplicity=st["multiplicity"], vdry=st["vdry"],
                idx=st["idx"], rhod=st["rhod"], thd=st["thd"],
                water_vapour_mixing_ratio=st["water_vapour_mixing_ratio"], dv=1e6,
                prhod=st["prhod"], pthd=st["pthd"],
                predicted_water_vapour_mixing_ratio=st["predicted_water_vapour_mixing_ratio"],
                kappa=st["kappa"], f_org=st["f_org"], rtol_x=1e-6, rtol_thd=1e-9,
                v_cr=st["v_cr"], timestep=dt, counters=counters, cell_order=cell_order,
                RH_max=RH_max, success=success, cell_id=st["cell_id"],
                reynolds_number=st["reynolds_number"], air_density=st["air_density"],
                air_dynamic_viscosity=st["air_dynamic_viscosity"])
            rec.update({f"out_{k}": _host(counters[k]) for k in COUNTERS})
            rec.update(out_water_mass=_host(st["water_mass"]), out_pthd=_host(st["pthd"]),
                       out_predicted_water_vapour_mixing_ratio=_host(
                           st["predicted_water_vapour_mixing_ratio"]),
                       out_RH_max=_host(RH_max), out_success=_host(success).astype(np.int64))
            calls.append(rec)
            # the next call starts where this one ended: predictions become the state
            st["thd"] = S.from_ndarray(_host(st["pthd"]))
            st["water_vapour_mixing_ratio"] = S.from_ndarray(
                _host(st["predicted_water_vapour_mixing_ratio"]))
            st["pthd"] = S.from_ndarray(_host(st["pthd"]) + 0.02)
            st["predicted_water_vapour_mixing_ratio"] = S.from_ndarray(
                _host(st["predicted_water_vapour_mixing_ratio"]) * (1 - 1e-4))
    arrays = {f"calls/{k}": np.stack([np.asarray(c[k]) for c in calls]) for k in calls[0]}
    arrays.update(n_calls=np.asarray(len(calls)), timestep=np.asarray(dt), dv=np.asarray(1e6),
                  n_cell=np.asarray(n_cell), rtol_x=np.asarray(1e-6),
                  rtol_thd=np.asarray(1e-9), dt_range=np.asarray((1e-4, dt)),
                  fuse=np.asarray(32), multiplier=np.asarray(2), RH_rtol=np.asarray(1e-7),
                  max_iters=np.asarray(16))
    print("box n_substeps", arrays["calls/out_n_substeps"].tolist())
    print("box success", arrays["calls/out_success"].tolist())
    save("cond_box", **arrays)


def ambient():
    rng = np.random.default_rng(7)
    formulae = Formulae()
    backend = CPU(formulae)
    S = backend.Storage
    n = 33
    rhod = rng.uniform(0.6, 1.3, n)
    thd = rng.uniform(270, 320, n)
    qv = rng.uniform(1e-4, 0.02, n)
    T, p, RH = (S.from_ndarray(np.zeros(n)) for _ in range(3))
    backend.temperature_pressure_rh(rhod=S.from_ndarray(rhod), thd=S.from_ndarray(thd),
                                    water_vapour_mixing_ratio=S.from_ndarray(qv), T=T, p=p, RH=RH)
    rho = S.from_ndarray(np.zeros(n))
    backend.air_density(output=rho, rhod=S.from_ndarray(rhod),
                        water_vapour_mixing_ratio=S.from_ndarray(qv))
    eta = S.from_ndarray(np.zeros(n))
    backend.air_dynamic_viscosity(output=eta, temperature=T)
    m = 57
    cell = rng.integers(0, n, m).astype(np.int64)
    kappa = rng.uniform(0.1, 1.3, m)
    f_org = np.zeros(m)
    v_dry = formulae.trivia.volume(np.exp(rng.uniform(np.log(1e-8), np.log(1e-6), m)))
    v_wet = v_dry * rng.uniform(2, 1000, m)
    v_cr = S.from_ndarray(np.zeros(m))
    backend.critical_volume(v_cr=v_cr, kappa=S.from_ndarray(kappa), f_org=S.from_ndarray(f_org),
                            v_dry=S.from_ndarray(v_dry), v_wet=S.from_ndarray(v_wet), T=T,
                            cell=S.from_ndarray(cell))
    radius = np.exp(rng.uniform(np.log(1e-7), np.log(1e-3), m))
    velocity = rng.uniform(0, 9, m)
    re = S.from_ndarray(np.zeros(m))
    backend.reynolds_number(output=re, cell_id=S.from_ndarray(cell), dynamic_viscosity=eta,
                            density=rho, radius=S.from_ndarray(radius),
                            velocity_wrt_air=S.from_ndarray(velocity))
    y0 = rng.uniform(-5, 5, 9)
    y = S.from_ndarray(y0.copy())
    backend.explicit_euler(y, 0.7, 1.3)
    save("cond_ambient", rhod=rhod, thd=thd, qv=qv, T=_host(T), p=_host(p), RH=_host(RH),
         air_density=_host(rho), air_dynamic_viscosity=_host(eta), cell=cell, kappa=kappa,
         f_org=f_org, v_dry=v_dry, v_wet=v_wet, v_cr=_host(v_cr), radius=radius,
         velocity_wrt_air=velocity, reynolds_number=_host(re), euler_y0=y0,
         euler_dt=np.asarray(0.7), euler_dy_dt=np.asarray(1.3), euler_y=_host(y))


if __name__ == "__main__":
    what = sys.argv[1:] or ["ambient", "box", "parcel"]
    if "ambient" in what:
        ambient()
    if "box" in what:
        box()
    if "parcel" in what:
        parcel(adaptive=True)
        parcel(adaptive=False)

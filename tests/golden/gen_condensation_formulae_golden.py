#!/usr/bin/env python3
"""Generates the goldens of condensation with non-default formulae (tests/golden/condf_*.npz) by
RUNNING THE REFERENCE (PySDM, its tree named by the environment variable PYSDM_REFERENCE) in its
pure-Python mode, with the same no-JIT import as gen_condensation_golden.py (the stand-ins of
tests/golden/standins put in front of it).  Run as:

    PYSDM_REFERENCE=<tree> PYTHONDONTWRITEBYTECODE=1 CI=1 \\
        python3 -B tests/golden/gen_condensation_formulae_golden.py [set ...]

Written (the sets and their formulae are tests/condensation_formulae_cases.py `SETS`):
  condf_<set>.npz  an 8-cell box (two cells empty) with different rhod / thd / qv per cell near
      saturation by the set's own saturation vapour pressure, prescribed predictions, f_org spread
      over [0, 1] with exact 0 and 1, Reynolds numbers from 0 to a few hundred; one adaptive and
      one fixed `backend.condensation` call, each recorded with its arguments and with what the
      reference left behind.  One set per non-default choice (the other options at their defaults)
      and three combined sets.  `hygroscopicity="KappaKoehler"` gets kappa >= 1 and wetter droplets:
      with kappa < 1 the full kappa-Koehler RH_eq has a pole at r^3 = rd^3 (1 - kappa) between
      x_insane and x_old, brackets fail and the adaptivity runs to dt_min.
  condf_bracket_fail.npz  one cell, a handful of droplets, KappaKoehler with kappa < 1 and a coarse
      dt_min: the bracket search fails and success is 0.
  condf_parcel_lowe2019.npz  a short `Parcel` ascent with the Lowe-2019 set and f_org > 0, every
      `backend.condensation` call recorded (as cond_parcel_a1.npz is).
  condf_ambient.npz  elementwise `temperature_pressure_rh` per saturation vapour pressure and
      `critical_volume` per surface tension and hygroscopicity.
"""
# pylint: disable=wrong-import-position,import-error,too-many-locals,protected-access
import os
import sys

os.environ.setdefault("CI", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.join(HERE, "standins"),
                os.environ["PYSDM_REFERENCE"]]

import numpy as np

from PySDM import Builder, Formulae
from PySDM.backends import CPU
from PySDM.dynamics import AmbientThermodynamics, Condensation
from PySDM.environments import Parcel
from PySDM.initialisation import spectra
from PySDM.initialisation.sampling.spectral_sampling import ConstantMultiplicity
from PySDM.physics import si

from tests.condensation_formulae_cases import (CONSTANTS, PVS_CHOICES, SETS, SGM_CHOICES,
                                               HYGRO_CHOICES)
from tests.golden.gen_condensation_golden import (CELL_IN, CONSTANT_IN, COUNTERS, STATE_IN,
                                                  Recorder, _host, _pack, save)


def formulae_of(options):
    return Formulae(constants=dict(CONSTANTS), **options)


def box_state(rng, formulae, *, n_cell, counts, kappa_range, wet_range):
    """the box's state: per-droplet columns, per-cell ambient state and predictions"""
    const = formulae.constants
    n_sd = int(counts.sum())
    cell_id = np.repeat(np.arange(n_cell), counts)[rng.permutation(n_sd)]
    idx = np.argsort(cell_id, kind="stable").astype(np.int64)
    cell_start = np.zeros(n_cell + 1, dtype=np.int64)
    cell_start[1:] = np.cumsum(np.bincount(cell_id, minlength=n_cell))
    r_dry = np.exp(rng.uniform(np.log(0.02e-6), np.log(0.4e-6), n_sd))
    vdry = const.PI_4_3 * r_dry ** 3
    kappa = rng.uniform(*kappa_range, n_sd)
    f_org = rng.uniform(0, 1, n_sd)
    f_org[:4] = (0.0, 1.0, 0.0, 1.0)
    multiplicity = rng.integers(1, 10 ** 9, n_sd).astype(np.int64)
    r_wet = r_dry * rng.uniform(*wet_range, n_sd)
    big = rng.uniform(size=n_sd) < 0.15
    r_wet[big] *= 50
    water_mass = const.rho_w * const.PI_4_3 * r_wet ** 3
    if n_sd > 12:
        multiplicity[5] = 0
        water_mass[7] = 0.0
        water_mass[11] = -water_mass[11]
    reynolds = np.where(big, rng.uniform(1, 400, n_sd), rng.uniform(0, 2, n_sd))
    reynolds[:3] = 0.0
    rhod = rng.uniform(1.0, 1.2, n_cell)
    thd = rng.uniform(285, 300, n_cell)
    qv = rng.uniform(0.006, 0.014, n_cell)
    T = formulae.state_variable_triplet.T(rhod, thd)
    target_rh = rng.uniform(0.985, 1.006, n_cell)
    for _ in range(30):  # fixed point: p depends on qv
        p = formulae.state_variable_triplet.p(rhod, T, qv)
        pv = target_rh * formulae.saturation_vapour_pressure.pvs_water(T)
        qv = const.eps * pv / (p - pv)
    prhod = rhod * (1 + rng.uniform(-2e-4, 0, n_cell))
    pthd = thd + rng.uniform(-0.05, 0.05, n_cell) * 10.0 ** rng.integers(0, 3, n_cell)
    pqv = qv * (1 + rng.uniform(-5e-4, 5e-4, n_cell) * 10.0 ** rng.integers(0, 3, n_cell))
    return dict(water_mass=water_mass, multiplicity=multiplicity, vdry=vdry, kappa=kappa,
                f_org=f_org, idx=idx, cell_start_arg=cell_start, cell_id=cell_id,
                reynolds_number=reynolds, rhod=rhod, thd=thd, water_vapour_mixing_ratio=qv,
                prhod=prhod, pthd=pthd, predicted_water_vapour_mixing_ratio=pqv,
                air_density=rhod * (1 + qv),
                air_dynamic_viscosity=formulae.air_dynamic_viscosity.eta_air(T)), T


def record_calls(backend, state, T, *, n_cell, dt, dt_range, modes, max_iters=16):
    """`backend.condensation` once per entry of `modes` (adaptive or not), each from the same
    state; v_cr from `backend.critical_volume` (the set's surface tension and hygroscopicity)"""
    S = backend.Storage
    v_cr = S.from_ndarray(np.zeros(state["vdry"].shape[0]))
    volume = np.abs(state["water_mass"]) / backend.formulae.constants.rho_w
    backend.critical_volume(v_cr=v_cr, kappa=S.from_ndarray(state["kappa"]),
                            f_org=S.from_ndarray(state["f_org"]),
                            v_dry=S.from_ndarray(state["vdry"]), v_wet=S.from_ndarray(volume),
                            T=S.from_ndarray(T), cell=S.from_ndarray(state["cell_id"]))
    state = dict(state, v_cr=_host(v_cr))
    calls = []
    for adaptive in modes:
        solver = backend.make_condensation_solver(
            dt, n_cell, dt_range=dt_range, adaptive=adaptive, fuse=32, multiplier=2,
            RH_rtol=1e-7, max_iters=max_iters)
        st = {k: S.from_ndarray(np.array(v)) for k, v in state.items()}
        counters = {k: S.from_ndarray(np.full(n_cell, -1 if adaptive or k != "n_substeps" else 3,
                                              dtype=np.int64)) for k in COUNTERS}
        RH_max = S.from_ndarray(np.full(n_cell, np.nan))
        success = S.from_ndarray(np.zeros(n_cell, dtype=bool))
        cell_order = np.argsort(state["rhod"]).astype(np.int64)
        rec = {k: _host(st[k]) for k in STATE_IN + CONSTANT_IN + CELL_IN}
        rec.update({f"in_{k}": _host(counters[k]) for k in COUNTERS})
        rec.update(cell_order=cell_order, adaptive=int(adaptive))
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
    arrays = {f"calls/{k}": np.stack([np.asarray(c[k]) for c in calls]) for k in calls[0]}
    arrays.update(n_calls=np.asarray(len(calls)), timestep=np.asarray(dt), dv=np.asarray(1e6),
                  n_cell=np.asarray(n_cell), rtol_x=np.asarray(1e-6), rtol_thd=np.asarray(1e-9),
                  dt_range=np.asarray(dt_range), fuse=np.asarray(32), multiplier=np.asarray(2),
                  RH_rtol=np.asarray(1e-7), max_iters=np.asarray(max_iters))
    return arrays


def box(name):
    cfg = SETS[name]
    rng = np.random.default_rng(cfg["seed"])
    formulae = formulae_of(cfg["options"])
    backend = CPU(formulae)
    n_cell = 8
    counts = rng.integers(6, 26, n_cell)
    counts[[2, 6]] = 0  # empty cells
    wet = cfg.get("wet_range", (1.5, 20))
    state, T = box_state(rng, formulae, n_cell=n_cell, counts=counts,
                         kappa_range=cfg.get("kappa_range", (0.2, 1.3)), wet_range=wet)
    arrays = record_calls(backend, state, T, n_cell=n_cell, dt=2.0, dt_range=(1e-4, 2.0),
                          modes=(True, False))
    print(name, "n_substeps", arrays["calls/out_n_substeps"].tolist(), "success",
          arrays["calls/out_success"].tolist())
    save(f"condf_{name}", **arrays)


def bracket_fail():
    """one cell, six droplets, KappaKoehler with kappa < 1, dt_min = dt / 2: no bracket"""
    rng = np.random.default_rng(11)
    formulae = formulae_of({"hygroscopicity": "KappaKoehler"})
    backend = CPU(formulae)
    state, T = box_state(rng, formulae, n_cell=1, counts=np.asarray([6]),
                         kappa_range=(0.2, 0.6), wet_range=(1.5, 4))
    arrays = record_calls(backend, state, T, n_cell=1, dt=1.0, dt_range=(0.5, 1.0),
                          modes=(True,))
    print("bracket_fail success", arrays["calls/out_success"].tolist(), "n_substeps",
          arrays["calls/out_n_substeps"].tolist())
    assert not arrays["calls/out_success"].any(), "the bracket did not fail"
    save("condf_bracket_fail", **arrays)


PARCEL = dict(n_sd=48, n_steps=12, dt=2 * si.s, mass_of_dry_air=1 * si.kg, p0=1000 * si.hPa,
              qv0=12 * si.g / si.kg, T0=290 * si.K, w=2 * si.m / si.s, kappa=0.6, f_org=0.3,
              spectrum=(200 / si.cm ** 3, 0.05 * si.um, 1.5))


def parcel():
    cfg = PARCEL
    formulae = formulae_of(SETS["lowe2019"]["options"])
    backend = CPU(formulae)
    recorder = Recorder(backend)
    env = Parcel(dt=cfg["dt"], mass_of_dry_air=cfg["mass_of_dry_air"], p0=cfg["p0"],
                 initial_water_vapour_mixing_ratio=cfg["qv0"], T0=cfg["T0"], w=cfg["w"])
    builder = Builder(n_sd=cfg["n_sd"], backend=backend, environment=env)
    builder.add_dynamic(AmbientThermodynamics())
    builder.add_dynamic(Condensation())
    norm, mode, sigma = cfg["spectrum"]
    spectrum = spectra.Lognormal(norm_factor=norm, m_mode=mode, s_geom=sigma)
    r_dry, n_per_volume = ConstantMultiplicity(spectrum).sample(cfg["n_sd"])
    attributes = builder.particulator.environment.init_attributes(
        n_in_dv=n_per_volume * builder.particulator.environment.mesh.dv, kappa=cfg["kappa"],
        r_dry=r_dry)
    attributes["dry volume organic"] = cfg["f_org"] * attributes["dry volume"]
    particulator = builder.build(attributes=attributes, products=())
    initial = {k: np.asarray(v) for k, v in attributes.items()}
    for _ in range(cfg["n_steps"]):
        particulator.run(steps=1)
    arrays = _pack(recorder, {f"init/{k}": v for k, v in initial.items()})
    arrays.update({f"parcel/{k}": np.asarray(v, dtype=float)
                   for k, v in cfg.items() if k != "spectrum"})
    arrays["parcel/spectrum"] = np.asarray(cfg["spectrum"], dtype=float)
    print("parcel n_substeps", arrays["calls/out_n_substeps"].ravel().tolist(), "n_activating",
          arrays["calls/out_n_activating"].ravel().tolist())
    save("condf_parcel_lowe2019", **arrays)


def ambient():
    rng = np.random.default_rng(7)
    n, m = 33, 57
    rhod = rng.uniform(0.6, 1.3, n)
    thd = rng.uniform(270, 320, n)
    qv = rng.uniform(1e-4, 0.02, n)
    cell = rng.integers(0, n, m).astype(np.int64)
    kappa = rng.uniform(0.1, 1.3, m)
    f_org = rng.uniform(0, 1, m)
    f_org[:4] = (0.0, 1.0, 0.0, 1.0)
    arrays = dict(rhod=rhod, thd=thd, qv=qv, cell=cell, kappa=kappa, f_org=f_org)
    for choice in PVS_CHOICES:
        backend = CPU(formulae_of({"saturation_vapour_pressure": choice}))
        S = backend.Storage
        T, p, RH = (S.from_ndarray(np.zeros(n)) for _ in range(3))
        backend.temperature_pressure_rh(
            rhod=S.from_ndarray(rhod), thd=S.from_ndarray(thd),
            water_vapour_mixing_ratio=S.from_ndarray(qv), T=T, p=p, RH=RH)
        arrays.update({f"T/{choice}": _host(T), f"p/{choice}": _host(p),
                       f"RH/{choice}": _host(RH)})
    T = arrays[f"T/{PVS_CHOICES[0]}"]
    v_dry = 4 / 3 * np.pi * np.exp(rng.uniform(np.log(1e-8), np.log(1e-6), m)) ** 3
    v_wet = v_dry * rng.uniform(2, 1000, m)
    arrays.update(v_dry=v_dry, v_wet=v_wet, T=T)
    for sgm in SGM_CHOICES:
        for hygro in HYGRO_CHOICES:
            backend = CPU(formulae_of({"surface_tension": sgm, "hygroscopicity": hygro}))
            S = backend.Storage
            v_cr = S.from_ndarray(np.zeros(m))
            backend.critical_volume(
                v_cr=v_cr, kappa=S.from_ndarray(kappa), f_org=S.from_ndarray(f_org),
                v_dry=S.from_ndarray(v_dry), v_wet=S.from_ndarray(v_wet), T=S.from_ndarray(T),
                cell=S.from_ndarray(cell))
            arrays[f"v_cr/{sgm}/{hygro}"] = _host(v_cr)
    save("condf_ambient", **arrays)


if __name__ == "__main__":
    what = sys.argv[1:] or ["ambient", "bracket_fail", "parcel", *SETS]
    for item in what:
        if item in SETS:
            box(item)
        else:
            {"ambient": ambient, "bracket_fail": bracket_fail, "parcel": parcel}[item]()

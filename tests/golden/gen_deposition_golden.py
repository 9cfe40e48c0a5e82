#!/usr/bin/env python3
"""Generates the deposition goldens (tests/golden/dep_*.npz) by RUNNING THE REFERENCE (PySDM at
/root/reference) in its pure-Python mode, with the same no-JIT import as gen_freezing_golden.py
(the stand-ins of tests/golden/standins put in front of it).  Run as:

    PYTHONDONTWRITEBYTECODE=1 CI=1 python3 -B tests/golden/gen_deposition_golden.py

Every call is `CPU(formulae).deposition(...)` itself.  Written:
  dep_methods.npz  one seeded state of 1000 rows over 7 cells - S_ice above 1 (cells 0, 5), below
      1 (cells 1, 6), exactly 1 (cell 2: RH = a_w_ice), a cell without ice (3) and an empty cell
      (4); ~60 % of the rows ice, ~5 % of multiplicity 0, masses log-uniform in 1e-16 .. 1e-8 kg,
      predicted columns that differ from the current ones - and one call for every combination of
      diffusion_coordinate x diffusion_ice_capacity x diffusion_ice_kinetics: inputs, the call's
      time step, and the outputs (masses, both predicted columns).
  dep_steps.npz  the default formulae, 256 rows over 3 cells, 20 consecutive calls; between calls
      the predicted values become current and T, p, RH, a_w_ice are recomputed with the reference
      backend's own `temperature_pressure_rh` and `a_w_ice`.  The state and T, p, RH, a_w_ice
      before the first call; masses and ambient columns after every call.

Asserted (dep_methods: a seed is tried after another until all hold):
  1. the reference's assertion (-delta_rv_i > current_vapour_mixing_ratio) never fires;
  2. in the logarithm cases every row has |ln(m_new / m)| <= 1 (the time step of a case is 0.8 /
     the largest relative growth rate, to 3 digits), so that the comparison tolerance is not eaten
     by an amplifying exp;
  3. in the WaterMass cases between 1 and 20 rows change sign (the time step is chosen between
     the 8th and 9th largest relative sublimation rate), so that path is recorded but does not
     dominate;
  4. in every cell with contributing rows |increment| >= 1e-6 |predicted| for both columns, so
     the sums are not compared on noise;
  dep_steps: the assertion never fires and at least one cell crosses between growth and
     sublimation during the run.
"""
# pylint: disable=wrong-import-position,import-error,too-many-locals
import itertools
import os
import sys

os.environ.setdefault("CI", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "standins"), "/root/reference"]

import numpy as np

from PySDM import Formulae
from PySDM.backends import CPU

OUT = HERE
COORDINATES = ("WaterMassLogarithm", "WaterMass")
CAPACITIES = ("Spherical", "Columnar")
KINETICS = ("Standard", "Neglect")
ARGUMENTS = ("T", "p", "RH", "a_w_ice", "qv", "rhod", "thd")


class Retry(Exception):
    pass


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


def formulae_for(coordinate="WaterMassLogarithm", capacity="Spherical", kinetics="Standard"):
    return Formulae(particle_shape_and_density="MixedPhaseSpheres",
                    diffusion_coordinate=coordinate, diffusion_ice_capacity=capacity,
                    diffusion_ice_kinetics=kinetics)


def ambient_of(formulae, T, p, S_ice):
    """a physically consistent cell: RH, a_w_ice, qv, rhod, thd of (T, p, S_ice)"""
    const = formulae.constants
    pvs_w = formulae.saturation_vapour_pressure.pvs_water(T)
    pvs_i = formulae.saturation_vapour_pressure.pvs_ice(T)
    pv = S_ice * pvs_i
    RH = pv / pvs_w
    a_w_ice = pvs_i / pvs_w
    qv = const.eps * pv / (p - pv)
    rhod = (p - pv) / const.Rd / T
    thd = T * np.power(const.p1000 / (p - pv), const.Rd_over_c_pd)
    return dict(T=T, p=p, RH=RH, a_w_ice=a_w_ice, qv=qv, rhod=rhod, thd=thd)


def call(formulae, state, masses, ambient, predicted, dt, dv):
    """one reference call; returns (masses, pqv, pthd) - Retry if the reference asserts"""
    backend = CPU(formulae)
    S = backend.Storage
    m = S.from_ndarray(masses.copy())
    pqv, pthd = S.from_ndarray(predicted[0].copy()), S.from_ndarray(predicted[1].copy())
    n_sd = masses.shape[0]
    try:
        backend.deposition(
            multiplicity=S.from_ndarray(state["multiplicity"].copy()), signed_water_mass=m,
            current_temperature=S.from_ndarray(ambient["T"].copy()),
            current_total_pressure=S.from_ndarray(ambient["p"].copy()),
            current_relative_humidity=S.from_ndarray(ambient["RH"].copy()),
            current_water_activity=S.from_ndarray(ambient["a_w_ice"].copy()),
            current_vapour_mixing_ratio=S.from_ndarray(ambient["qv"].copy()),
            current_dry_air_density=S.from_ndarray(ambient["rhod"].copy()),
            current_dry_potential_temperature=S.from_ndarray(ambient["thd"].copy()),
            cell_volume=dv, time_step=dt, cell_id=S.from_ndarray(state["cell_id"].copy()),
            reynolds_number=S.from_ndarray(np.zeros(n_sd)),
            schmidt_number=S.from_ndarray(np.zeros(ambient["T"].shape[0])),
            predicted_vapour_mixing_ratio=pqv, predicted_dry_potential_temperature=pthd)
    except AssertionError as fired:
        raise Retry("the reference's assertion fired") from fired
    return m.to_ndarray(), pqv.to_ndarray(), pthd.to_ndarray()


def three_digits(x):
    return float(f"{x:.3g}")


# ---- dep_methods ---------------------------------------------------------------------------------
N_SD, N_CELL, DV = 1000, 7, 1.0
CELL_T = np.array([253.0, 248.0, 258.0, 263.0, 250.0, 238.0, 266.0])
CELL_P = np.array([70e3, 60e3, 75e3, 80e3, 65e3, 45e3, 85e3])
CELL_S = np.array([1.04, 0.95, 1.0, 1.1, 1.0, 1.12, 0.9])


def methods(seed):
    rng = np.random.default_rng(seed)
    plain = formulae_for()
    ambient = ambient_of(plain, CELL_T, CELL_P, CELL_S)
    ambient["RH"][2] = ambient["a_w_ice"][2]  # S_ice == 1 exactly
    assert ambient["RH"][2] / ambient["a_w_ice"][2] == 1
    cell = rng.choice([0, 1, 2, 3, 5, 6], N_SD).astype(np.int64)  # cell 4 stays empty
    mass = np.exp(rng.uniform(np.log(1e-16), np.log(1e-8), N_SD))
    ice = (rng.uniform(size=N_SD) < 0.6 / (5 / 6)) & (cell != 3)  # cell 3: liquid only
    mass[ice] *= -1
    multiplicity = np.exp(rng.uniform(np.log(1e5), np.log(2e7), N_SD)).astype(np.int64)
    multiplicity[rng.uniform(size=N_SD) < 0.05] = 0
    state = dict(multiplicity=multiplicity, cell_id=cell)
    predicted = (ambient["qv"] * (1 + 1e-3 * rng.uniform(-1, 1, N_CELL)),
                 ambient["thd"] + 0.1 * rng.uniform(-1, 1, N_CELL))
    contributing = ice & np.isin(cell, [0, 1, 5, 6])
    print(f"seed {seed}: {ice.mean():.3f} ice, {(multiplicity == 0).mean():.3f} multiplicity 0")
    arrays = {f"cell/{k}": ambient[k] for k in ARGUMENTS}
    arrays.update(cell_id=cell, signed_water_mass=mass, multiplicity=multiplicity,
                  predicted_qv=predicted[0], predicted_thd=predicted[1],
                  cell_volume=np.asarray(DV), seed=np.asarray(seed))
    for number, (coordinate, capacity, kinetics) in enumerate(
            itertools.product(COORDINATES, CAPACITIES, KINETICS)):
        # the relative rates dm_dt / m of this capacity x kinetics, from a probe call with a tiny
        # time step in the untransformed coordinate
        probe_dt = 1e-7
        probe, _, _ = call(formulae_for("WaterMass", capacity, kinetics), state, mass, ambient,
                           predicted, probe_dt, DV)
        rate = (probe[contributing] - mass[contributing]) / mass[contributing] / probe_dt
        if coordinate == "WaterMassLogarithm":
            dt = three_digits(0.8 / np.abs(rate).max())
        else:
            sublimation = np.sort(-rate[rate < 0])[::-1]
            dt = three_digits(2 / (sublimation[7] + sublimation[8]))
        formulae = formulae_for(coordinate, capacity, kinetics)
        out_mass, out_qv, out_thd = call(formulae, state, mass, ambient, predicted, dt, DV)
        what = f"{coordinate} {capacity} {kinetics} dt={dt}"
        changed = out_mass != mass
        np.testing.assert_array_equal(changed[~contributing], False)
        if coordinate == "WaterMassLogarithm":
            worst = np.abs(np.log(out_mass[contributing] / mass[contributing])).max()
            print(f"{what}: max |ln(m_new / m)| = {worst:.3f}")
            if not worst <= 1:
                raise Retry(what)
            assert (out_mass[ice] < 0).all()
        else:
            n_flipped = int((out_mass[ice] > 0).sum())
            print(f"{what}: {n_flipped} rows change sign")
            if not 1 <= n_flipped <= 20:
                raise Retry(what)
        for c in range(N_CELL):
            touched = c in (0, 1, 5, 6)
            for got, before in ((out_qv, predicted[0]), (out_thd, predicted[1])):
                if touched:
                    if not abs(got[c] - before[c]) >= 1e-6 * abs(before[c]):
                        raise Retry(f"{what}: cell {c}: increment {got[c] - before[c]!r}")
                else:
                    assert got[c] == before[c]
        arrays[f"calls/{number}/coordinate"] = np.asarray(coordinate)
        arrays[f"calls/{number}/capacity"] = np.asarray(capacity)
        arrays[f"calls/{number}/kinetics"] = np.asarray(kinetics)
        arrays[f"calls/{number}/time_step"] = np.asarray(dt)
        arrays[f"calls/{number}/out_signed_water_mass"] = out_mass
        arrays[f"calls/{number}/out_predicted_qv"] = out_qv
        arrays[f"calls/{number}/out_predicted_thd"] = out_thd
    arrays["n_calls"] = np.asarray(8)
    save("dep_methods", **arrays)


# ---- dep_steps -----------------------------------------------------------------------------------
STEPS_N_SD, STEPS_N_CELL, N_STEPS, STEPS_DT, STEPS_DV = 256, 3, 20, 1.0, 1.0
# time step over the relaxation time of the cell's vapour: > 1 overshoots (the cell then
# alternates between growth and sublimation), < 1 relaxes from one side
STEPS_DT_OVER_TAU = np.array([1.4, 0.3, 0.15])


def refresh(backend, rhod, thd, qv):
    """T, p, RH, a_w_ice of the state, by the reference backend's own methods"""
    S = backend.Storage
    n = rhod.shape[0]
    T, p, RH, a_w_ice, RH_ice = (S.from_ndarray(np.zeros(n)) for _ in range(5))
    s_qv = S.from_ndarray(qv.copy())
    backend.temperature_pressure_rh(rhod=S.from_ndarray(rhod.copy()),
                                    thd=S.from_ndarray(thd.copy()),
                                    water_vapour_mixing_ratio=s_qv, T=T, p=p, RH=RH)
    backend.a_w_ice(T=T, p=p, RH=RH, water_vapour_mixing_ratio=s_qv, a_w_ice=a_w_ice,
                    RH_ice=RH_ice)
    return dict(T=T.to_ndarray(), p=p.to_ndarray(), RH=RH.to_ndarray(),
                a_w_ice=a_w_ice.to_ndarray(), qv=qv.copy(), rhod=rhod.copy(), thd=thd.copy())


def steps(seed):
    rng = np.random.default_rng(seed)
    formulae = formulae_for()
    backend = CPU(formulae)
    start = ambient_of(formulae, np.array([250.0, 245.0, 260.0]), np.array([60e3, 50e3, 80e3]),
                       np.array([1.08, 1.15, 0.9]))
    rhod, thd, qv = start["rhod"], start["thd"], start["qv"]
    cell = rng.integers(0, STEPS_N_CELL, STEPS_N_SD).astype(np.int64)
    mass = np.exp(rng.uniform(np.log(1e-12), np.log(1e-9), STEPS_N_SD))
    ice = rng.uniform(size=STEPS_N_SD) < 0.6
    mass[ice] *= -1
    multiplicity = np.exp(rng.uniform(np.log(1e3), np.log(1e4), STEPS_N_SD))
    # scale each cell's multiplicities to its dt / tau, measured by a probe call
    ambient = refresh(backend, rhod, thd, qv)
    probe_dt = 1e-6
    state = dict(multiplicity=np.ceil(multiplicity).astype(np.int64), cell_id=cell)
    _, probe_qv, _ = call(formulae, state, mass, ambient, (qv, thd), probe_dt, STEPS_DV)
    S_ice = ambient["RH"] / ambient["a_w_ice"]
    one_over_tau = -(probe_qv - qv) / probe_dt / (qv * (1 - 1 / S_ice))
    multiplicity *= (STEPS_DT_OVER_TAU / (STEPS_DT * one_over_tau))[cell]
    state["multiplicity"] = np.ceil(multiplicity).astype(np.int64)
    arrays = dict(cell_id=cell, signed_water_mass=mass, multiplicity=state["multiplicity"],
                  rhod=rhod, thd=thd, qv=qv, dt=np.asarray(STEPS_DT), dv=np.asarray(STEPS_DV),
                  n_steps=np.asarray(N_STEPS), seed=np.asarray(seed))
    arrays.update({k: ambient[k] for k in ("T", "p", "RH", "a_w_ice")})  # before the first call
    history = {k: [] for k in ("signed_water_mass", "qv", "thd", "T", "p", "RH", "a_w_ice")}
    signs = []
    for _ in range(N_STEPS):
        ambient = refresh(backend, rhod, thd, qv)
        signs.append(np.sign(ambient["RH"] / ambient["a_w_ice"] - 1))
        mass, qv, thd = call(formulae, state, mass, ambient, (qv, thd), STEPS_DT, STEPS_DV)
        after = refresh(backend, rhod, thd, qv)
        history["signed_water_mass"].append(mass)
        for key in ("qv", "thd", "T", "p", "RH", "a_w_ice"):
            history[key].append(after[key])
    signs = np.stack(signs)
    crossing = ((signs[1:] * signs[:-1]) < 0).any(axis=0)
    print("S_ice - 1 by step:\n", np.stack(history["RH"]) / np.stack(history["a_w_ice"]) - 1)
    print("cells that cross between growth and sublimation:", np.flatnonzero(crossing))
    if not crossing.any():
        raise Retry("no cell crosses")
    assert (mass[ice] < 0).all()
    arrays.update({f"steps/{k}": np.stack(v) for k, v in history.items()})
    save("dep_steps", **arrays)


def _retrying(function, first_seed):
    for seed in range(first_seed, first_seed + 50):
        try:
            return function(seed)
        except Retry as refused:
            print(f"seed {seed} refused: {refused}")
    raise RuntimeError("no seed satisfies the generator's conditions")


if __name__ == "__main__":
    what = sys.argv[1:] or ["methods", "steps"]
    if "methods" in what:
        _retrying(methods, 20261017)
    if "steps" in what:
        _retrying(steps, 20261117)

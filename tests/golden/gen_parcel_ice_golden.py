#!/usr/bin/env python3
"""Generates tests/golden/parcel_ice_runs.npz by RUNNING THE REFERENCE (PySDM, at $PYSDM_REFERENCE)
in its pure-Python mode, with the same no-JIT import as gen_parcel_golden.py.  Run as:

    PYSDM_REFERENCE=<PySDM checkout> PYTHONDONTWRITEBYTECODE=1 CI=1 \
        python3 -B tests/golden/gen_parcel_ice_golden.py

Three short ascents of `Parcel(mixed_phase=True)` with 48 super-droplets of 5 - 15 um (a quarter of
them ice at the start), steps of 0.1 s:
  a  AmbientThermodynamics, Condensation, Freezing(singular=True), VapourDepositionOnIce; 30 steps
  b  AmbientThermodynamics, Condensation, VapourDepositionOnIce, Freezing(singular=False,
     immersion_freezing=False, homogeneous_freezing=True) with a constant rate, at 237 K; 30 steps
  c  AmbientThermodynamics, Condensation, Freezing(singular=False, thaw=True) with ABIFM, a
     sinusoidal w(t); 40 steps
For each run <r> the file holds
  <r>/profile/<q>   after every step: z, rhod, thd, qv, T, p, RH, RH_max, a_w_ice, RH_ice (the
                    environment's values as the reference leaves them), n_ice (the multiplicities
                    of the rows with a negative signed water mass) and the solver's n_substeps
  <r>/init/<a>      multiplicity, water_mass (signed), dry_volume, kappa, and freezing_temperature
                    or immersed_surface_area where the run reads them
  <r>/final/water_mass, <r>/final/rng_offset (uniforms the Freezing dynamic has drawn)
  <r>/cfg/<k>       dt, T0, p0, qv0, mass_of_dry_air, z0, n_steps, seed; <r>/w_mid
and the same from two more runs with T0 replaced by nextafter(T0, +-inf), as <r>_up/...,
<r>_down/....  spread/<r>/<q> is the worst relative difference of <q> between the three runs.  The
generator asserts that the three runs of each ascent freeze the same rows at the same steps.
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
from PySDM.dynamics import (AmbientThermodynamics, Condensation, Freezing,
                            VapourDepositionOnIce)
from PySDM.environments import Parcel
from PySDM.physics import si

from tests.golden.gen_condensation_golden import _host, save

FLOATS = ("z", "rhod", "thd", "qv", "T", "p", "RH", "RH_max", "a_w_ice", "RH_ice")
ENV = {"z": "z", "rhod": "rhod", "thd": "thd", "qv": "water_vapour_mixing_ratio", "T": "T",
       "p": "p", "RH": "RH", "a_w_ice": "a_w_ice", "RH_ice": "RH_ice"}
N_SD, DT, SEED = 48, 0.1 * si.s, 44

RUNS = {
    "a": dict(T0=258.0, n_steps=30, w=2.0, order=("freezing", "deposition"),
              freezing=dict(singular=True), options={}, constants={}),
    "b": dict(T0=237.2, n_steps=30, w=2.0, order=("deposition", "freezing"),
              freezing=dict(singular=False, immersion_freezing=False, homogeneous_freezing=True),
              options=dict(homogeneous_ice_nucleation_rate="Constant"),
              constants=dict(J_HOM=1e14)),
    "c": dict(T0=246.0, n_steps=40, w=lambda t: 3.0 * np.sin(np.pi * t / 4.0) + 1.0,
              order=("freezing",), freezing=dict(singular=False, thaw=True),
              options=dict(heterogeneous_ice_nucleation_rate="ABIFM"),
              constants=dict(ABIFM_M=54.48, ABIFM_C=-10.67)),
}
P0, MASS_OF_DRY_AIR = 60000.0, 1.0


def _first(storage):
    return np.asarray(_host(storage)).reshape(-1)[0]


def ascent(cfg, T0):
    """one run of the reference; {key: array} without the run's prefix"""
    formulae = Formulae(particle_shape_and_density="MixedPhaseSpheres", seed=SEED,
                        constants=dict(cfg["constants"]), **cfg["options"])
    const = formulae.constants
    pvs = formulae.saturation_vapour_pressure.pvs_water(T0)
    qv0 = const.eps * 1.002 * pvs / (P0 - 1.002 * pvs)
    w = cfg["w"] if callable(cfg["w"]) else (lambda t, value=cfg["w"]: value)
    env = Parcel(dt=DT, mass_of_dry_air=MASS_OF_DRY_AIR, p0=P0,
                 initial_water_vapour_mixing_ratio=qv0, T0=T0, w=w, mixed_phase=True)
    builder = Builder(n_sd=N_SD, backend=CPU(formulae), environment=env)
    builder.add_dynamic(AmbientThermodynamics())
    builder.add_dynamic(Condensation())
    for which in cfg["order"]:
        builder.add_dynamic(Freezing(**cfg["freezing"]) if which == "freezing"
                            else VapourDepositionOnIce())
    rng = np.random.default_rng(7)
    r_dry = np.exp(rng.uniform(np.log(2e-8), np.log(2e-7), N_SD))
    r_wet = rng.uniform(5e-6, 15e-6, N_SD)
    mass = const.rho_w * 4 / 3 * np.pi * r_wet ** 3
    frozen = rng.uniform(size=N_SD) < 0.25
    attributes = {
        "multiplicity": np.full(N_SD, 40000, dtype=np.int64),
        "dry volume": 4 / 3 * np.pi * r_dry ** 3,
        "kappa times dry volume": 0.6 * 4 / 3 * np.pi * r_dry ** 3,
        "signed water mass": np.where(frozen, -mass * const.rho_i / const.rho_w, mass),
    }
    out = {}
    if cfg["freezing"].get("immersion_freezing", True):
        if cfg["freezing"]["singular"]:
            attributes["freezing temperature"] = T0 + rng.uniform(-0.12, 0.01, N_SD)
            out["init/freezing_temperature"] = attributes["freezing temperature"]
        else:
            attributes["immersed surface area"] = 1.5e-7 * rng.uniform(0.5, 2.0, N_SD)
            out["init/immersed_surface_area"] = attributes["immersed surface area"]
    particulator = builder.build(attributes=attributes, products=())
    environment, attr = particulator.environment, particulator.attributes
    condensation = particulator.dynamics["Condensation"]
    out.update({"init/multiplicity": _host(attr["multiplicity"]).astype(np.int64),
                "init/water_mass": _host(attr["signed water mass"]),
                "init/dry_volume": _host(attr["dry volume"]), "init/kappa": _host(attr["kappa"])})
    rows = {name: [] for name in FLOATS + ("n_ice", "n_substeps")}
    w_mid, signs = [], []
    for step in range(cfg["n_steps"]):
        w_mid.append(float(environment.w((step + 1 / 2) * DT)))
        particulator.run(steps=1)
        for name, var in ENV.items():
            rows[name].append(float(_first(environment[var])))
        rows["RH_max"].append(float(_first(condensation.rh_max)))
        rows["n_substeps"].append(int(_first(condensation.counters["n_substeps"])))
        m = _host(attr["signed water mass"])
        rows["n_ice"].append(int(_host(attr["multiplicity"])[m < 0].sum()))
        signs.append(m < 0)
        assert bool(_first(condensation.success))
    for name in FLOATS:
        out[f"profile/{name}"] = np.asarray(rows[name], dtype=float)
    for name in ("n_ice", "n_substeps"):
        out[f"profile/{name}"] = np.asarray(rows[name], dtype=np.int64)
    out["signs"] = np.asarray(signs)
    out["final/water_mass"] = _host(attr["signed water mass"])
    freezing = particulator.dynamics.get("Freezing")
    drawn = 0
    if freezing is not None and getattr(freezing, "rng", None) is not None:
        passes = int(not cfg["freezing"]["singular"]
                     and cfg["freezing"].get("immersion_freezing", True)) + int(
                         cfg["freezing"].get("homogeneous_freezing", False))
        drawn = passes * N_SD * cfg["n_steps"]
    out["final/rng_offset"] = np.asarray(drawn, dtype=np.int64)
    out["w_mid"] = np.asarray(w_mid, dtype=float)
    for key, value in (("dt", DT), ("p0", P0), ("qv0", qv0), ("T0", T0), ("z0", 0.0),
                       ("mass_of_dry_air", MASS_OF_DRY_AIR), ("n_steps", cfg["n_steps"]),
                       ("seed", SEED)):
        out[f"cfg/{key}"] = np.asarray(float(value))
    return out


def main():
    arrays = {}
    for run, cfg in RUNS.items():
        T0 = float(cfg["T0"])
        trio = {"": ascent(cfg, T0), "_up": ascent(cfg, np.nextafter(T0, np.inf)),
                "_down": ascent(cfg, np.nextafter(T0, -np.inf))}
        base = trio[""]
        for suffix, result in trio.items():
            assert np.array_equal(result["signs"], base["signs"]), \
                f"run {run}{suffix} does not freeze the same rows at the same steps"
            arrays.update({f"{run}{suffix}/{key}": value for key, value in result.items()
                           if key != "signs"})
        for name, key in [(q, f"profile/{q}") for q in FLOATS] + [("water_mass",
                                                                   "final/water_mass")]:
            worst = 0.0
            for x in trio.values():
                for y in trio.values():
                    worst = max(worst, float(np.max(np.abs(x[key] - y[key])
                                                    / np.abs(base[key]))))
            arrays[f"spread/{run}/{name}"] = np.asarray(worst)
        liquid = base["init/water_mass"] > 0
        newly = float(np.mean(base["final/water_mass"][liquid] < 0))
        print(run, "n_ice", base["profile/n_ice"].tolist(), "frozen of the liquid", newly,
              "RH", base["profile/RH"][[0, -1]], "RH_ice", base["profile/RH_ice"][[0, -1]],
              "spread", {q: float(arrays[f"spread/{run}/{q}"]) for q in ("thd", "RH", "water_mass")})
        assert 0.1 < newly < 0.9, f"run {run}: {newly} of the liquid rows froze"
    save("parcel_ice_runs", **arrays)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates tests/golden/parcel_runs.npz by RUNNING THE REFERENCE (PySDM, at $PYSDM_REFERENCE) in
its pure-Python mode, with the same no-JIT import as gen_condensation_golden.py (the stand-ins of
tests/golden/standins put in front of it).  Run as:

    PYSDM_REFERENCE=<PySDM checkout> PYTHONDONTWRITEBYTECODE=1 CI=1 \
        python3 -B tests/golden/gen_parcel_golden.py

Three short `Parcel` ascents with `AmbientThermodynamics()` + `Condensation()`:
  a  the configuration of cond_parcel_a1.npz (192 super-droplets, 40 steps of 1 s, w = 5 m/s)
  b  a sinusoidal w(t) that turns into a descent, so that droplets deactivate (asserted here)
  c  the Lowe-2019 set with f_org > 0 (the configuration of condf_parcel_lowe2019.npz)
For each run <r> the file holds
  <r>/profile/<q>   the state after every step: z, rhod, thd, qv, T, p, RH, RH_max and the four
                    counters n_substeps, n_activating, n_deactivating, n_ripening
  <r>/init/<a>      the initial attributes: multiplicity, water_mass, dry_volume, kappa, f_org
  <r>/final/water_mass
  <r>/cfg/<k>       dt, T0, p0, qv0, mass_of_dry_air, z0, n_steps; <r>/w_mid: the updraft of
                    every step (at its mid-point, as Parcel evaluates it)
and the same from two more runs of the reference with T0 replaced by nextafter(T0, +-inf), as
<r>_up/... and <r>_down/....  spread/<r>/<q> is the worst relative difference of quantity <q>
(water_mass: the final masses) between the three runs: the reference's own sensitivity to one
rounding of its input, measured on the reference alone.  The tests' bounds rest on it.
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

from tests.condensation_formulae_cases import CONSTANTS, SETS
from tests.golden.gen_condensation_formulae_golden import PARCEL as PARCEL_LOWE2019
from tests.golden.gen_condensation_golden import PARCEL as PARCEL_A1
from tests.golden.gen_condensation_golden import _host, save

FLOATS = ("z", "rhod", "thd", "qv", "T", "p", "RH", "RH_max")
COUNTERS = ("n_substeps", "n_activating", "n_deactivating", "n_ripening")
ENV = {"z": "z", "rhod": "rhod", "thd": "thd", "qv": "water_vapour_mixing_ratio", "T": "T",
       "p": "p", "RH": "RH"}

B_AMPLITUDE, B_QUARTER_PERIOD = 10 * si.m / si.s, 40 * si.s
RUNS = {
    "a": dict(PARCEL_A1, options={}, f_org=None),
    "b": dict(PARCEL_A1, n_sd=64, n_steps=60, dt=2 * si.s, options={}, f_org=None,
              w=lambda t: B_AMPLITUDE * np.cos(np.pi / 2 * t / B_QUARTER_PERIOD)),
    "c": dict(PARCEL_LOWE2019, options=SETS["lowe2019"]["options"]),
}


def _first(storage):
    return np.asarray(_host(storage)).reshape(-1)[0]


def ascent(cfg, T0):
    """one run of the reference; {key: array} without the run's prefix"""
    formulae = Formulae(constants=dict(CONSTANTS), **cfg["options"]) if cfg["options"] \
        else Formulae()
    backend = CPU(formulae)
    env = Parcel(dt=cfg["dt"], mass_of_dry_air=cfg["mass_of_dry_air"], p0=cfg["p0"],
                 initial_water_vapour_mixing_ratio=cfg["qv0"], T0=T0, w=cfg["w"])
    builder = Builder(n_sd=cfg["n_sd"], backend=backend, environment=env)
    builder.add_dynamic(AmbientThermodynamics())
    builder.add_dynamic(Condensation())
    norm, mode, sigma = cfg["spectrum"]
    spectrum = spectra.Lognormal(norm_factor=norm, m_mode=mode, s_geom=sigma)
    r_dry, n_per_volume = ConstantMultiplicity(spectrum).sample(cfg["n_sd"])
    environment = builder.particulator.environment
    attributes = environment.init_attributes(n_in_dv=n_per_volume * environment.mesh.dv,
                                             kappa=cfg["kappa"], r_dry=r_dry)
    if cfg["f_org"] is not None:
        attributes["dry volume organic"] = cfg["f_org"] * attributes["dry volume"]
    particulator = builder.build(attributes=attributes, products=())
    attr = particulator.attributes
    condensation = particulator.dynamics["Condensation"]  # (the Builder registers a copy)
    out = {"init/multiplicity": _host(attr["multiplicity"]).astype(np.int64),
           "init/water_mass": _host(attr["signed water mass"]),
           "init/dry_volume": _host(attr["dry volume"]), "init/kappa": _host(attr["kappa"]),
           "init/f_org": _host(attr["dry volume organic fraction"])}
    rows = {name: [] for name in FLOATS + COUNTERS}
    w_mid = []
    for step in range(cfg["n_steps"]):
        w_mid.append(float(environment.w((step + 1 / 2) * cfg["dt"])))
        particulator.run(steps=1)
        for name, var in ENV.items():
            rows[name].append(float(_first(environment[var])))
        rows["RH_max"].append(float(_first(condensation.rh_max)))
        for name in COUNTERS:
            rows[name].append(int(_first(condensation.counters[name])))
        assert bool(_first(condensation.success))
    for name in FLOATS:
        out[f"profile/{name}"] = np.asarray(rows[name], dtype=float)
    for name in COUNTERS:
        out[f"profile/{name}"] = np.asarray(rows[name], dtype=np.int64)
    out["final/water_mass"] = _host(attr["signed water mass"])
    out["w_mid"] = np.asarray(w_mid, dtype=float)
    for key in ("dt", "p0", "qv0", "mass_of_dry_air", "n_steps"):
        out[f"cfg/{key}"] = np.asarray(cfg[key], dtype=float)
    out["cfg/T0"], out["cfg/z0"] = np.asarray(float(T0)), np.asarray(0.0)
    return out


def main():
    arrays = {}
    for run, cfg in RUNS.items():
        T0 = float(cfg["T0"])
        trio = {"": ascent(cfg, T0), "_up": ascent(cfg, np.nextafter(T0, np.inf)),
                "_down": ascent(cfg, np.nextafter(T0, -np.inf))}
        for suffix, result in trio.items():
            arrays.update({f"{run}{suffix}/{key}": value for key, value in result.items()})
        base = trio[""]
        for name, key in [(q, f"profile/{q}") for q in FLOATS] + [("water_mass",
                                                                   "final/water_mass")]:
            worst = 0.0
            for x in trio.values():
                for y in trio.values():
                    worst = max(worst, float(np.max(np.abs(x[key] - y[key])
                                                    / np.abs(base[key]))))
            arrays[f"spread/{run}/{name}"] = np.asarray(worst)
        print(run, "n_substeps", base["profile/n_substeps"].tolist(), "activating max",
              base["profile/n_activating"].max(), "deactivating max",
              base["profile/n_deactivating"].max(), "spread",
              {q: float(arrays[f"spread/{run}/{q}"]) for q in ("thd", "RH", "water_mass")})
        for suffix in ("_up", "_down"):
            for name in COUNTERS:
                if not np.array_equal(trio[suffix][f"profile/{name}"], base[f"profile/{name}"]):
                    print(f"  note: {run}{suffix} differs from {run} in {name}")
    assert arrays["a/profile/n_activating"].max() > 0, "run a: no activation"
    assert arrays["b/profile/n_deactivating"].max() > 0, "run b: no deactivation"
    assert arrays["b/w_mid"].min() < 0 < arrays["b/w_mid"].max(), "run b: no descent"
    assert arrays["c/init/f_org"].min() > 0, "run c: f_org must be > 0"
    save("parcel_runs", **arrays)


if __name__ == "__main__":
    main()

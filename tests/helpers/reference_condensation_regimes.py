#!/usr/bin/env python3
"""Runs the reference's own code (its CPU backend in its pure-Python mode: `temperature_pressure_rh`,
`critical_volume`, `condensation` with its own TOMS748, and `equilibrate_wet_radii`) on the planted
inputs of tests/golden/condensation_regimes.npz: a guard on how tests/condensation_regime_cases.py
reads the reference, not an accuracy test.

 * pointwise values (T, p, RH, the critical volume) against the float64 run of the restatement
   recorded there, at rtol 1e-12; where CompressedFilmRuehl's isotherm is searched the two sides
   solve it differently (to 1e-6 and to the last bit), so those rows are held to the row's bound;
 * roots (one sub-step of condensation with rtol_x = 1e-14, the wet radii with rtol = 1e-14)
   against the fixture's expected values within the row's bound, the counters exactly: the
   reference's search ends anywhere within its tolerance, which is part of that bound.

Only where the reference tree is present."""
# pylint: disable=wrong-import-position,import-error,too-many-locals,invalid-name
import os
import sys
from types import SimpleNamespace

os.environ.setdefault("CI", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden", "standins"), "/root/reference"]

import numpy as np

from PySDM import Formulae
from PySDM.backends import CPU
from PySDM.initialisation.equilibrate_wet_radii import equilibrate_wet_radii

from tests import condensation_formulae_cases as fc
from tests import condensation_regime_cases as cases

RTOL = 1e-12
_BACKENDS = {}


def backend_of(name):
    if name not in _BACKENDS:
        cfg = cases.SETS[name]
        _BACKENDS[name] = CPU(Formulae(constants={**fc.CONSTANTS, **cfg.get("constants", {})},
                                       **cfg["options"]))
    return _BACKENDS[name]


def tprh(columns):
    out = {key: np.full(len(columns["set"]), np.nan) for key in ("T", "p", "RH")}
    for name in sorted(set(columns["set"].tolist())):
        sel = np.flatnonzero(columns["set"] == name)
        backend = backend_of(name)
        S = backend.Storage.from_ndarray
        res = {key: S(np.zeros(len(sel))) for key in out}
        backend.temperature_pressure_rh(
            rhod=S(np.ascontiguousarray(columns["rhod"][sel])),
            thd=S(np.ascontiguousarray(columns["thd"][sel])),
            water_vapour_mixing_ratio=S(np.ascontiguousarray(columns["qv"][sel])), **res)
        for key, value in res.items():
            out[key][sel] = value.to_ndarray()
    return out


def vcr(columns):
    out = {"v_cr": np.full(len(columns["set"]), np.nan)}
    for name in sorted(set(columns["set"].tolist())):
        sel = np.flatnonzero(columns["set"] == name)
        backend = backend_of(name)
        S = backend.Storage.from_ndarray
        col = {key: S(np.ascontiguousarray(columns[key][sel]))
               for key in ("kappa", "f_org", "v_dry", "v_wet", "T")}
        v_cr = S(np.zeros(len(sel)))
        backend.critical_volume(v_cr=v_cr, cell=S(np.arange(len(sel), dtype=np.int64)), **col)
        out["v_cr"][sel] = v_cr.to_ndarray()
    return out


def wet(columns):
    out = {"r_wet": np.full(len(columns["set"]), np.nan)}
    for name in sorted(set(columns["set"].tolist())):
        sel = np.flatnonzero(columns["set"] == name)
        backend = backend_of(name)
        fields = {key: backend.Storage.from_ndarray(np.ascontiguousarray(columns[key][sel]))
                  for key in ("T", "RH")}
        environment = SimpleNamespace(particulator=SimpleNamespace(formulae=backend.formulae))

        class Environment:  # pylint: disable=too-few-public-methods
            particulator = environment.particulator

            def __getitem__(self, key):
                return fields[key]  # pylint: disable=cell-var-from-loop

        out["r_wet"][sel] = equilibrate_wet_radii(
            r_dry=np.ascontiguousarray(columns["r_dry"][sel]), environment=Environment(),
            kappa_times_dry_volume=np.ascontiguousarray(columns["kappa_times_dry_volume"][sel]),
            f_org=np.ascontiguousarray(columns["f_org"][sel]),
            cell_id=np.arange(len(sel), dtype=np.int64), rtol=cases.RTOL_X,
            max_iters=cases.MAX_ITERS)
    return out


def cond(columns):
    floats, ints = cases.GROUPS["cond"][2], cases.GROUPS["cond"][3]
    n_all = len(columns["set"])
    out = {key: np.full(n_all, np.nan) for key in floats}
    out.update({key: np.full(n_all, -7, dtype=np.int64) for key in ints})
    for name, timestep in sorted(set(zip(columns["set"].tolist(),
                                         columns["timestep"].tolist()))):
        sel = np.flatnonzero((columns["set"] == name) & (columns["timestep"] == timestep))
        backend = backend_of(name)
        S = backend.Storage.from_ndarray
        n_cell = len(sel)
        counts = columns["n_drops"][sel].astype(np.int64)
        cell_start = np.zeros(n_cell + 1, dtype=np.int64)
        cell_start[1:] = np.cumsum(counts)
        where = [(c, i) for c in range(n_cell) for i in range(int(counts[c]))]
        drop = {key: S(np.array([columns[key][sel[c]][i] for c, i in where],
                                dtype=np.int64 if key == "multiplicity" else float))
                for key in cases.DROP_COLUMNS}
        cell = {key: S(np.ascontiguousarray(columns[key][sel], dtype=float))
                for key in cases.CELL_COLUMNS}
        solver = backend.make_condensation_solver(
            timestep, n_cell, dt_range=(1e-4, timestep), adaptive=False, fuse=32, multiplier=2,
            RH_rtol=cases.RH_RTOL, max_iters=cases.MAX_ITERS)
        counters = {key: S(np.full(n_cell, 1 if key == "n_substeps" else -1, dtype=np.int64))
                    for key in cases.COUNTERS}
        RH_max, success = S(np.full(n_cell, np.nan)), S(np.zeros(n_cell, dtype=bool))
        backend.condensation(
            solver=solver, n_cell=n_cell, cell_start_arg=S(cell_start),
            water_mass=drop["water_mass"], multiplicity=drop["multiplicity"], vdry=drop["vdry"],
            idx=S(np.arange(len(where), dtype=np.int64)), rhod=cell["rhod"], thd=cell["thd"],
            water_vapour_mixing_ratio=cell["qv"], dv=float(columns["dv"][sel][0]),
            prhod=cell["prhod"], pthd=cell["pthd"],
            predicted_water_vapour_mixing_ratio=cell["pqv"], kappa=drop["kappa"],
            f_org=drop["f_org"], rtol_x=cases.RTOL_X, rtol_thd=1e-9, v_cr=drop["v_cr"],
            timestep=timestep, counters=counters,
            cell_order=np.arange(n_cell, dtype=np.int64), RH_max=RH_max, success=success,
            cell_id=S(np.array([c for c, _ in where], dtype=np.int64)),
            reynolds_number=drop["reynolds_number"], air_density=cell["air_density"],
            air_dynamic_viscosity=cell["air_dynamic_viscosity"])
        assert success.to_ndarray().all(), name
        mass = drop["water_mass"].to_ndarray()
        for at, (c, i) in enumerate(where):
            out[f"mass{i}"][sel[c]] = mass[at]
        for c in range(n_cell):
            for i in range(int(counts[c]), cases.MAX_DROPS):
                out[f"mass{i}"][sel[c]] = 0.0
        out["pthd"][sel] = cell["pthd"].to_ndarray()
        out["pqv"][sel] = cell["pqv"].to_ndarray()
        out["RH_max"][sel] = RH_max.to_ndarray()
        for key in ints:
            out[key][sel] = counters[key].to_ndarray()
    return out


RUNNERS = {"tprh": tprh, "vcr": vcr, "wet": wet, "cond": cond}


def main():
    fix = cases.Fixture()
    failures = 0
    with np.errstate(all="ignore"):
        for group in fix.groups:
            columns, labels = fix.inputs(group), fix.labels(group)
            got = RUNNERS[group](columns)
            plain, expected = fix.outputs(group, "float64"), fix.outputs(group, "expected")
            ratios = cases.errors_over_bounds(group, got, fix)
            searched = np.array(["ruehl/searched" in str(lab) for lab in labels])
            for key in cases.GROUPS[group][2]:
                if group in ("tprh", "vcr"):
                    good = np.isclose(got[key], plain[key], rtol=RTOL, atol=0)
                    good = np.where(searched, ratios[key] <= 1, good)
                else:
                    good = ratios[key] <= 1
                if not good.all():
                    failures += 1
                    rows = np.flatnonzero(~good)[:5]
                    print(f"{group}/{key}: {int((~good).sum())} rows differ, e.g.",
                          [(int(i), str(labels[i]), float(got[key][i]), float(plain[key][i]),
                            float(ratios[key][i])) for i in rows])
            for key in cases.GROUPS[group][3]:
                if (got[key] != expected[key]).any():
                    failures += 1
                    print(f"{group}/{key}: differs on rows",
                          np.flatnonzero(got[key] != expected[key])[:5].tolist())
            print(f"{group}: compared {len(labels)} rows; worst error over bound "
                  f"{max(float(np.max(r)) for r in ratios.values()):.3g}")
    sys.exit(1 if failures else 0)


if __name__ == "__main__":
    main()

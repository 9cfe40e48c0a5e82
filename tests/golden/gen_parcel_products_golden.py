#!/usr/bin/env python3
"""Generates tests/golden/parcel_products.npz by RUNNING THE REFERENCE (PySDM, at
$PYSDM_REFERENCE) in its pure-Python mode, with the same no-JIT import and stand-ins as
gen_parcel_golden.py.  Run as:

    PYSDM_REFERENCE=<PySDM checkout> PYTHONDONTWRITEBYTECODE=1 CI=1 \
        python3 -B tests/golden/gen_parcel_products_golden.py

The three ascents of gen_parcel_golden.py (`a`, `b`: the one where droplets deactivate, `c`:
Lowe-2019) with the reference's own product objects registered: those of
tests/parcel_products_cases.py `GOLDEN_PRODUCTS`.  For every k-th step (GOLDEN_EVERY) of run <r>
the file holds
  <r>/steps                 the recorded steps (1-based: the state after that many steps)
  <r>/water_mass            the per-droplet water masses, steps x n_sd
  <r>/T, <r>/rhod, <r>/dv   the environment's T and rhod and `mesh.dv` at output time
  <r>/product/<name>        every product's value, steps (x bins)
and <r>/multiplicity, <r>/dry_volume, <r>/kappa, <r>/f_org (constant over the run).

It asserts, on the reference's own attributes, that in the recorded steps no droplet's filter or
bin attribute lies within a relative 1e-9 of a filter bound or bin edge of any product: no
rounding can then move a droplet across one, and counts must agree exactly.
"""
# pylint: disable=wrong-import-position,import-error,too-many-locals,protected-access
import os
import re
import sys

os.environ.setdefault("CI", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.join(HERE, "standins"),
                os.environ["PYSDM_REFERENCE"]]

import numpy as np

import PySDM.products as reference_products
from PySDM import Builder, Formulae
from PySDM.backends import CPU
from PySDM.dynamics import AmbientThermodynamics, Condensation
from PySDM.environments import Parcel
from PySDM.initialisation import spectra
from PySDM.initialisation.sampling.spectral_sampling import ConstantMultiplicity

import pysdm_amd.products as own_products
from tests.condensation_formulae_cases import CONSTANTS
from tests.golden.gen_condensation_golden import _host, save
from tests.golden.gen_parcel_golden import RUNS
from tests.parcel_products_cases import GOLDEN_EVERY, golden_products

# pint reads "kg^-1 m^-1" as a product; the stand-in of tests/golden/standins wants the `*`
import PySDM.products.impl.product as product_module

_parse = product_module._UNIT_REGISTRY.parse_expression
product_module._UNIT_REGISTRY.parse_expression = lambda text, *a, **k: _parse(
    re.sub(r"(?<=[\w)])\s+(?=[A-Za-z(])", " * ", str(text).strip()), *a, **k)

CLEARANCE = 1e-9
# the reference's attribute behind each filter of include/sdm_parcel_diag.h
ATTRIBUTE = {"water mass": "signed water mass", "signed water mass": "signed water mass",
             "volume": "volume", "dry volume": "dry volume",
             "wet to critical volume ratio": "wet to critical volume ratio"}


def bounds_of(formulae):
    """{the reference's attribute name: the finite, non-zero bounds and edges the products
    compare it with}; the products' own statement of their requests, on the reference's
    constants"""
    out = {}
    for product in golden_products(own_products):
        for request in product.requests(formulae):
            out.setdefault(ATTRIBUTE[request.filter_attr], set()).update(
                (request.min_x, request.max_x))
        wanted = product.spectrum(formulae)
        if wanted is not None:
            out.setdefault(ATTRIBUTE[wanted.bin_attr], set()).update(wanted.edges)
    return {name: np.array(sorted(b for b in values if np.isfinite(b) and b != 0))
            for name, values in out.items()}


def ascent(run, cfg):
    formulae = Formulae(constants=dict(CONSTANTS), **cfg["options"]) if cfg["options"] \
        else Formulae()
    backend = CPU(formulae)
    env = Parcel(dt=cfg["dt"], mass_of_dry_air=cfg["mass_of_dry_air"], p0=cfg["p0"],
                 initial_water_vapour_mixing_ratio=cfg["qv0"], T0=float(cfg["T0"]), w=cfg["w"])
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
    for name in set(ATTRIBUTE.values()):
        builder.request_attribute(name)
    particulator = builder.build(attributes=attributes,
                                 products=golden_products(reference_products))
    attr = particulator.attributes
    bounds = bounds_of(formulae)
    out = {"multiplicity": _host(attr["multiplicity"]).astype(np.int64),
           "dry_volume": _host(attr["dry volume"]), "kappa": _host(attr["kappa"]),
           "f_org": _host(attr["dry volume organic fraction"])}
    rows = {key: [] for key in ("steps", "water_mass", "T", "rhod", "dv")}
    values = {name: [] for name in particulator.products}
    closest = np.inf
    for step in range(1, cfg["n_steps"] + 1):
        particulator.run(steps=1)
        if step % GOLDEN_EVERY[run]:
            continue
        rows["steps"].append(step)
        rows["water_mass"].append(_host(attr["signed water mass"]))
        rows["T"].append(float(np.asarray(_host(environment["T"])).reshape(-1)[0]))
        rows["rhod"].append(float(np.asarray(_host(environment["rhod"])).reshape(-1)[0]))
        rows["dv"].append(float(environment.mesh.dv))
        for name, product in particulator.products.items():
            values[name].append(np.array(product.get(), dtype=float, copy=True).reshape(-1))
        for name, edges in bounds.items():
            x = _host(attr[name]).reshape(-1, 1)
            gap = float(np.min(np.abs(x - edges) / edges))
            assert gap > CLEARANCE, (run, step, name, gap)
            closest = min(closest, gap)
    out["steps"] = np.asarray(rows["steps"], dtype=np.int64)
    out["water_mass"] = np.stack(rows["water_mass"])
    for key in ("T", "rhod", "dv"):
        out[key] = np.asarray(rows[key], dtype=float)
    for name, series in values.items():
        out[f"product/{name}"] = np.squeeze(np.stack(series))
    print(run, "recorded steps", rows["steps"], "closest droplet to a bound (relative)", closest,
          "n_act", out["product/n_act"].tolist())
    return out


def main():
    arrays = {}
    for run, cfg in RUNS.items():
        arrays.update({f"{run}/{key}": value for key, value in ascent(run, cfg).items()})
    assert arrays["a/product/n_act"].max() > 0, "run a: nothing activated"
    assert arrays["b/product/n_act"][-1] < arrays["b/product/n_act"].max(), \
        "run b: nothing deactivated"
    save("parcel_products", **arrays)
    limit = os.path.getsize(os.path.join(HERE, "parcel_runs.npz"))
    size = os.path.getsize(os.path.join(HERE, "parcel_products.npz"))
    assert size <= limit, (size, limit)


if __name__ == "__main__":
    main()

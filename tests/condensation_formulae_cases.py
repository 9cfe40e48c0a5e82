"""Shared by the tests of condensation with non-default formulae and by the generator of their
goldens (tests/golden/gen_condensation_formulae_golden.py): the formulae sets, the constants the
organic-film surface tensions need, seeded multi-cell cases for HIP / checker parity and the
tolerances of the replay against the reference's goldens."""
import json
import os

import numpy as np

from pysdm_amd.formulae import Formulae
from pysdm_amd.condensation import descriptor_of
from pysdm_amd.physics.condensation_formulae import CHOICES, HOST_REFUSED
from tests import condensation_cases as cc

# the organic film: Ovadnevaite et al. 2017 (40 mN / m, a 0.1 nm monolayer) and an organic acid
# of Ruehl et al. 2016 (tab. S1: A0, C0, m_sigma; molar volume of 0.2 kg / mol at 1250 kg / m3)
CONSTANTS = {
    "sgm_org": 0.04, "delta_min": 1e-10,
    "RUEHL_nu_org": 1.6e-4, "RUEHL_A0": 115e-20, "RUEHL_C0": 6e-7, "RUEHL_m_sigma": 0.3e17,
    "RUEHL_sgm_min": 0.04,
}

PVS_CHOICES = CHOICES["saturation_vapour_pressure"]
SGM_CHOICES = CHOICES["surface_tension"]
HYGRO_CHOICES = CHOICES["hygroscopicity"]

# one set per non-default choice (the other options at PySDM's defaults) ...
SETS = {}
for _option, _choices in CHOICES.items():
    for _choice in _choices[1:]:
        SETS[_choice if _choice not in SETS else f"{_option}_{_choice}"] = {
            "options": {_option: _choice}, "seed": 20261019 + len(SETS)}
# (kappa < 1 puts a pole of the full kappa-Koehler RH_eq between x_insane and x_old: every failed
# bracket drives the reference's adaptivity to dt_min; the bracket_fail golden pins that case)
SETS["KappaKoehler"].update(kappa_range=(1.0, 1.4), wet_range=(3, 20))
# ... and three combined ones
SETS["lowe2019"] = {"seed": 20261101, "options": {
    "surface_tension": "CompressedFilmOvadnevaite", "diffusion_kinetics": "LoweEtAl2019",
    "diffusion_thermics": "LoweEtAl2019", "latent_heat_vapourisation": "Lowe2019",
    "saturation_vapour_pressure": "AugustRocheMagnus"}}
SETS["ventilated"] = {"seed": 20261102, "options": {
    "ventilation": "PruppacherAndRasmussen1979", "drop_growth": "Fick",
    "diffusion_thermics": "GrabowskiEtAl2011", "saturation_vapour_pressure": "MurphyKoop2005",
    "latent_heat_vapourisation": "Constant"}}
SETS["water_mass"] = {"seed": 20261103, "options": {
    "diffusion_coordinate": "WaterMass", "drop_growth": "Howell1949",
    "saturation_vapour_pressure": "Bolton1980", "ventilation": "Froessling1938",
    "surface_tension": "SzyszkowskiLangmuir"}}
# every golden file condf_<name>.npz of recorded `backend.condensation` calls -> its formulae
GOLDENS = {**{name: cfg["options"] for name, cfg in SETS.items()},
           "bracket_fail": {"hygroscopicity": "KappaKoehler"},
           "parcel_lowe2019": SETS["lowe2019"]["options"]}
SINGLE_SETS = [name for name in SETS if len(SETS[name]["options"]) == 1]
COMBINED_SETS = [name for name in SETS if len(SETS[name]["options"]) > 1]

# Replay of the reference's goldens (condf_<set>.npz): integers exactly; floats within FOUR TIMES
# the worst relative difference checker vs golden measured per set and quantity (DESIGN.md section
# 9 lists the measurements; 0: the checker reproduces the reference bit for bit).  Where a bound
# exceeds the default path's cc.GOLDEN_RTOL the cause is the one named there: the reference ran
# with NumPy's exp / log / power, which are not correctly rounded, and one ulp inside TOMS748
# moves its iterates anywhere within rtol_x.
with open(os.path.join(cc.HERE, "golden", "condf_measured.json"), encoding="utf-8") as _file:
    MEASURED = json.load(_file)  # {golden: {quantity: worst relative difference}}


def golden_rtol(name, key):
    return 4 * MEASURED[name][key]


def _options(name_or_options):
    return GOLDENS[name_or_options] if isinstance(name_or_options, str) else name_or_options


def host_refused(name_or_options):
    """whether `Formulae` refuses one of the choices (HOST_REFUSED): such a set runs through the
    library with an explicit descriptor (`descriptor_for`), not through a backend class"""
    return any(choice in HOST_REFUSED.get(option, ())
               for option, choice in _options(name_or_options).items())


def formulae_for(name_or_options):
    """the Formulae of a set; for a host-refused set the one of its other choices, which carries
    the constants (the choices then travel in `descriptor_for`)"""
    options = {option: choice for option, choice in _options(name_or_options).items()
               if choice not in HOST_REFUSED.get(option, ())}
    return Formulae(constants=dict(CONSTANTS), **options)


def descriptor_for(name_or_options):
    """the explicit descriptor of a host-refused set, None for any other (the formulae's own)"""
    if not host_refused(name_or_options):
        return None
    return descriptor_of(_options(name_or_options), formulae_for(name_or_options).constants)


def seeded_case(seed, counts, options, **kwargs):
    """cc.seeded_case with the formulae of `options`, f_org in {0, 1, between} and Reynolds
    numbers in {0, > 0}"""
    case = cc.seeded_case(seed, counts, **kwargs)
    rng = np.random.default_rng(seed + 1)
    n_sd = case["n_sd"]
    f_org = rng.uniform(0, 1, n_sd)
    f_org[rng.uniform(size=n_sd) < 0.15] = 0.0
    f_org[rng.uniform(size=n_sd) < 0.15] = 1.0
    reynolds = rng.uniform(0, 300, n_sd)
    reynolds[rng.uniform(size=n_sd) < 0.3] = 0.0
    case.update(formulae=formulae_for(options), descriptor=descriptor_for(options), f_org=f_org,
                reynolds_number=reynolds)
    if options.get("hygroscopicity") == "KappaKoehler":
        case["kappa"] = rng.uniform(1.0, 1.4, n_sd)
    return case


def run_case(engine, case, *, adaptive, general=False):
    """cc.run_case, optionally through `sdm_condensation_f` whatever the formulae"""
    from pysdm_amd.condensation import COUNTERS, condensation_call  # pylint: disable=import-outside-toplevel

    up, down = engine.upload, engine.download
    arrays = {k: None if v is None else up(np.asarray(v)) for k, v in case.items()
              if k != "descriptor" and (v is None or isinstance(v, np.ndarray))}
    n_cell = case["n_cell"]
    counters = {k: up(np.full(n_cell, (-1 if adaptive else 3) if k == "n_substeps" else -1,
                              dtype=np.int64)) for k in COUNTERS}
    RH_max, success = up(np.full(n_cell, np.nan)), up(np.zeros(n_cell, dtype=np.uint8))
    scalars = {k: case[k] for k in ("formulae", "n_sd", "n_cell", "dv", "rtol_x", "rtol_thd",
                                    "timestep", "dt_range", "fuse", "multiplier", "RH_rtol",
                                    "max_iters")}
    condensation_call(engine, **scalars, adaptive=adaptive, counters=counters, RH_max=RH_max,
                      success=success, general=general, descriptor=case.get("descriptor"),
                      **arrays)
    out = {k: down(v) for k, v in counters.items()}
    out.update(water_mass=down(arrays["water_mass"]), pthd=down(arrays["pthd"]),
               predicted_water_vapour_mixing_ratio=down(
                   arrays["predicted_water_vapour_mixing_ratio"]),
               RH_max=down(RH_max), success=down(success))
    return out


def replay(backend_class, engine, name, data, call):
    """recorded call `call` of condf_<name>.npz: through the backend class with the set's
    Formulae, or - a host-refused set - through the engine with the set's explicit descriptor"""
    if not host_refused(name):
        return cc.replay(backend_class(formulae_for(name)), data, call)
    solver = cc.solver_of(data)
    case = {key: np.array(data[f"calls/{key}"][call]) for key in (
        "water_mass", "v_cr", "multiplicity", "vdry", "kappa", "f_org", "idx", "reynolds_number",
        "rhod", "thd", "water_vapour_mixing_ratio", "prhod", "pthd",
        "predicted_water_vapour_mixing_ratio", "air_density", "air_dynamic_viscosity",
        "cell_order")}
    case.update(formulae=formulae_for(name), descriptor=descriptor_for(name),
                cell_start=np.array(data["calls/cell_start_arg"][call]),
                n_sd=case["water_mass"].shape[0], n_cell=case["rhod"].shape[0],
                dv=float(data["dv"]), rtol_x=float(data["rtol_x"]),
                rtol_thd=float(data["rtol_thd"]), timestep=solver["timestep"],
                dt_range=solver["dt_range"], fuse=solver["fuse"], multiplier=solver["multiplier"],
                RH_rtol=solver["RH_rtol"], max_iters=solver["max_iters"])
    adaptive = bool(data["calls/adaptive"][call])
    # (run_case starts the counters as the generator's box does: -1, and 3 sub-steps when fixed)
    np.testing.assert_array_equal(data["calls/in_n_substeps"][call], -1 if adaptive else 3)
    out = run_case(engine, case, adaptive=adaptive)
    out["success"] = out["success"].astype(np.int64)
    return out


def assert_matches_golden(out, data, call, name):
    for key in cc.OUT_INTS:
        np.testing.assert_array_equal(out[key], data[f"calls/out_{key}"][call],
                                      err_msg=f"{name} call {call}: {key}")
    for key in cc.OUT_FLOATS:
        np.testing.assert_allclose(out[key], data[f"calls/out_{key}"][call],
                                   rtol=golden_rtol(name, key), atol=0,
                                   err_msg=f"{name} call {call}: {key}")


def worst_relative_difference(out, data, call):
    """{quantity: max |out - golden| / |golden|} of one replayed call (for measuring MEASURED)"""
    worst = {}
    for key in cc.OUT_FLOATS:
        ref = np.asarray(data[f"calls/out_{key}"][call], dtype=float)
        got = np.asarray(out[key], dtype=float)
        both_nan = np.isnan(ref) & np.isnan(got)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(both_nan | (ref == got), 0.0, np.abs(got - ref) / np.abs(ref))
        worst[key] = float(np.max(rel)) if rel.size else 0.0
    return worst

#!/usr/bin/env python3
"""Times the adiabatic parcel on the GPU (pysdm_amd.parcel.ParcelRunner): ensembles of 1, 16, 256
and 1024 parcels of 256 super-droplets, 100 steps of 1 s, updrafts spread over 0.2 .. 5 m/s, with
PySDM's default formulae and with the Lowe-2019 set (tests/condensation_formulae_cases.py).

The fused route (`sdm_parcel_run`: one call, the steps inside the kernel) at every size; the stage
route (the same step written with the symbols of include/sdm_condensation.h, a Python loop over
parcels and steps with its read-backs) at 1 and 16 parcels only - it is a loop over parcels, so
its larger sizes would say nothing new, and nothing here extrapolates it.  The stage route is the
yardstick: it uses only symbols that existed before the fused route.

Timed with HIP events on the stream around `run(steps, profile=False)`, every repetition from the
same restored state, a warm-up call first; the figure is the median of --reps calls.  The longest
single launch is measured separately: the same ascent as calls of `steps_per_launch` steps, each
one launch, the slowest of them reported.  Writes profiles/parcel_timing.json and prints it; a
measurement, not a test: no threshold, no ratio fixed in advance.

`--products` is a measurement of its own (the output above does not change): 1, 16 and 256
parcels, the fused route with `products=()` and with the eleven products of pysdm_amd/products.py
and a 64-bin spectrum (`sdm_parcel_run_diag`: the request table evaluated inside the kernel's step
loop; the rows' download is part of the timed call), and at 1 and 16 parcels the route that
existed before: `run(1)`, `snapshot()` and `diagnostics.moments` / `spectrum_moments` on a
`Population` of the snapshot, per step (it has no activation filter: it computes the moments of
the five unfiltered products and the spectrum only).  `--products-stepwise-only` times just the
latter, which needs nothing of this module's newer interfaces.  Writes
profiles/parcel_products_timing.json.

`--chemistry` is a further measurement of its own: the parcel with aqueous chemistry
(include/sdm_parcel_chem.h), PySDM's default formulae, n_substep = 5, an open and a closed system:
the fused route (`sdm_parcel_run_chem`: per step one launch of the parcel kernel and one of
k_parcel_chem) at 1, 16, 256 and 1024 parcels, the stage route (the stage step, then
`sdm_chemistry_step` on the parcel's slice and the two element-wise updates) at 1 and 16, and the
same ascents without chemistry on the same build.  Writes profiles/parcel_chem_timing.json.

`--ventilation` is a further measurement of its own: the ventilated parcel
(include/sdm_parcel_vent.h; PySDM's default formulae with the ventilation
PruppacherAndRasmussen1979 and the Gunn-Kinzer table): the fused route (`sdm_parcel_run_vent`)
against the fused route with the ventilation Neglect (through k_parcel and through k_parcel_f) at
1, 16, 256 and 1024 parcels, and against the ventilated stage route at 1 and 16.  Writes
profiles/parcel_vent_timing.json with the ratios; no threshold.

`python scripts/bench_parcel.py --coalescence` times the parcel with coalescence
(include/sdm_parcel_coal.h; Coalescence(Geometric()), adaptive): 1024 parcels of 256 rows on the
fused route (`sdm_parcel_run_coal`) against `sdm_parcel_run` with one step per launch at the same
shape (what the collisions add), and against the stage route (the stage step, then
`sdm_collision_step` with n_cell = 1, parcel by parcel) at the same shape; once with the haze of
the other measurements (nothing coalesces) and once with drizzle-sized drops (pairs do).  Writes
profiles/parcel_coal_timing.json with the ratios; no threshold.

`python scripts/bench_parcel.py --breakup` times the parcel with collisional breakup
(include/sdm_parcel_breakup.h; Collision(Geometric(), ConstEc(0.5), ConstEb(1), Straub2010Nf),
adaptive): 1024 parcels of 256 rows of drizzle-sized drops, in which pairs coalesce and break up,
on the fused route (`sdm_parcel_run_collision`) against the stage route (the stage step, then
`sdm_collision_step` with breakup, parcel by parcel) and against the same ascents with
coalescence only.  Writes profiles/parcel_breakup_timing.json with the ratios; the one claim is
that fused is not slower than stages.

`python scripts/bench_parcel.py --ice` times the mixed-phase parcel (include/sdm_parcel_ice.h;
tests/parcel_ice_cases.py's cold ensemble: 1024 parcels of 256 rows, a quarter of them ice, 20
steps of 0.1 s, time-dependent immersion freezing and homogeneous freezing with constant rates,
then deposition, ordered sums): `sdm_parcel_run_ice`, `sdm_parcel_run` alone on the same rows (the
solver leaves the ice alone) and the stage route (parcel by parcel with read-backs; one call).
With `--against DIR` (a checkout of the parent commit with its own library built) it then runs the
default measurement of this script - the four parcel counts, both formulae, fused route - there
and here, alternating, `--rounds` times, each in a process of its own, to show that the existing
kernels did not move.  Writes profiles/parcel_ice_timing.json with the ratios; no threshold.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (1, 16, 256, 1024)
STAGE_SIZES = (1, 16)
N_SD, STEPS, DT = 256, 100, 1.0


CHEM_SUBSTEPS = 5
# ammonium bisulphate and the trace gases of the reference's Kreidenweis et al. 2003 example
CHEM_DRY_RHO, CHEM_DRY_MOLAR_MASS = 1800.0, 0.11511
CHEM_MOLE_FRACTIONS = {"SO2": 0.2e-9, "O3": 50e-9, "H2O2": 0.5e-9, "CO2": 360e-6, "HNO3": 0.1e-9,
                       "NH3": 0.1e-9}


def make_runner(kind, n_parcel, route, steps_per_launch, engine=None, system=None, **more):
    from pysdm_amd import spectra  # pylint: disable=import-outside-toplevel
    from pysdm_amd.condensation import CondensationSetup  # pylint: disable=import-outside-toplevel
    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel
    from pysdm_amd.parcel import ParcelRunner  # pylint: disable=import-outside-toplevel
    from tests.parcel_cases import formulae_of  # pylint: disable=import-outside-toplevel

    updrafts = np.linspace(0.2, 5.0, n_parcel) if n_parcel > 1 else np.array([2.0])
    chemistry = {}
    if system is not None:
        from pysdm_amd.chemistry import ChemistrySetup  # pylint: disable=import-outside-toplevel

        chemistry = dict(chemistry=ChemistrySetup(system, CHEM_SUBSTEPS),
                         mole_fractions=CHEM_MOLE_FRACTIONS, dry_rho=CHEM_DRY_RHO,
                         dry_molar_mass=CHEM_DRY_MOLAR_MASS)
    return ParcelRunner.from_spectrum(
        engine or HipEngine.get(), formulae_of(kind), CondensationSetup(), dt=DT, T0=290.0,
        p0=100000.0, qv0=0.012, w=updrafts, mass_of_dry_air=1.0,
        spectrum=spectra.Lognormal(norm_factor=60e6 / 1.18, m_mode=0.04e-6, s_geom=1.4),
        kappa=1.28, f_org=None if kind == "default" else 0.3, n_sd=N_SD, n_parcel=n_parcel,
        route=route, steps_per_launch=steps_per_launch, **chemistry, **more)


def timed(runner, start, steps, reps, warmup, call=None):
    import torch  # pylint: disable=import-outside-toplevel

    samples = []
    for rep in range(warmup + reps):
        runner.restore(start)
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        if call is None:
            runner.run(steps, profile=False)
        else:
            call(runner, steps)
        end.record()
        end.synchronize()
        if rep >= warmup:
            samples.append(begin.elapsed_time(end))
    return samples


def measure(kind, n_parcel, route, reps, warmup, steps_per_launch):
    runner = make_runner(kind, n_parcel, route, steps_per_launch)
    start = runner.snapshot()
    samples = timed(runner, start, STEPS, reps, warmup)
    final = runner.snapshot()
    assert (final["failed_step"] == -1).all() and (final["steps_done"] == STEPS).all()
    ms = float(np.median(samples))
    out = {"formulae": kind, "route": route, "n_parcel": n_parcel, "n_sd_per_parcel": N_SD,
           "steps": STEPS, "reps": reps, "ms_median": round(ms, 3),
           "ms_min": round(float(np.min(samples)), 3), "ms_max": round(float(np.max(samples)), 3),
           "ms_per_parcel_step": round(ms / (n_parcel * STEPS), 5),
           "n_substeps_last": [int(final["n_substeps"].min()), int(final["n_substeps"].max())],
           "RH_max_last": round(float(final["RH_max"].max()), 5)}
    if route == "fused":
        per_launch = steps_per_launch or SPL_DEFAULT
        out["steps_per_launch"] = per_launch
        runner.restore(start)
        launches = []
        for _ in range(0, STEPS, per_launch):  # one launch per call
            state = runner.snapshot()
            launches.append(float(np.median(timed(runner, state, per_launch, 1, 0))))
        out["longest_launch_ms"] = round(max(launches), 3)
        out["launches"] = len(launches)
    return out


SPL_DEFAULT = 16  # SDM_PARCEL_STEPS_PER_LAUNCH of include/sdm_parcel.h
PRODUCT_SIZES = (1, 16, 256)
SPECTRUM_EDGES = np.geomspace(2e-8, 2e-5, 65)


def eleven_products():
    from pysdm_amd import products as pr  # pylint: disable=import-outside-toplevel

    act = dict(count_unactivated=False, count_activated=True)
    return (pr.ParticleConcentration(), pr.ParticleSpecificConcentration(),
            pr.WaterMixingRatio(), pr.MeanRadius(), pr.EffectiveRadius(),
            pr.ActivatedParticleConcentration(**act),
            pr.ActivatedParticleSpecificConcentration(**act), pr.ActivatedMeanRadius(**act),
            pr.ActivatedEffectiveRadius(**act),
            pr.ParticleSizeSpectrumPerMassOfDryAir(radius_bins_edges=SPECTRUM_EDGES),
            pr.ParticleSizeSpectrumPerVolume(radius_bins_edges=SPECTRUM_EDGES))


def stepwise(runner, steps):
    """the products' moments the way they could be had before: per step one `run(1)`, a
    `snapshot()` and `diagnostics.moments` / `spectrum_moments` on a Population of it"""
    from pysdm_amd import diagnostics  # pylint: disable=import-outside-toplevel
    from pysdm_amd.population import Population  # pylint: disable=import-outside-toplevel

    eng = runner.engine
    multiplicity = eng.download(runner.multiplicity)
    cell_id = np.repeat(np.arange(runner.n_parcel), np.diff(runner.parcel_start_host))
    volume_edges = 4 / 3 * np.pi * SPECTRUM_EDGES ** 3
    out = []
    for _ in range(steps):
        profile = runner.run(1)
        state = runner.snapshot()
        population = Population(eng, multiplicity=multiplicity, mass=state["water_mass"],
                                cell_id=cell_id, n_cell=runner.n_parcel)
        out.append((
            profile["rhod"],
            diagnostics.moments(population, [0, 1], attr="water mass"),  # (host arrays)
            diagnostics.moments(population, [1 / 3, 2 / 3, 1]),
            diagnostics.spectrum_moments(population, volume_edges, bin_attr="volume")))
    return out


def measure_products(kind, n_parcel, mode, reps, warmup):
    runner = make_runner(kind, n_parcel, "fused", 0)
    start = runner.snapshot()
    if mode == "stepwise":
        call = stepwise
    elif mode == "fused":
        call = None
    else:
        products = eleven_products()
        call = lambda r, steps: r.run(steps, profile=False, products=products)  # noqa: E731
    samples = timed(runner, start, STEPS, reps, warmup, call)
    final = runner.snapshot()
    assert (final["failed_step"] == -1).all() and (final["steps_done"] == STEPS).all()
    ms = float(np.median(samples))
    return {"formulae": kind, "mode": mode, "n_parcel": n_parcel, "n_sd_per_parcel": N_SD,
            "steps": STEPS, "reps": reps, "ms_median": round(ms, 3),
            "ms_min": round(float(np.min(samples)), 3),
            "ms_max": round(float(np.max(samples)), 3),
            "ms_per_parcel_step": round(ms / (n_parcel * STEPS), 5)}


def main_products(args):
    results = []
    for kind in ("default", "lowe2019"):
        modes = [] if args.products_stepwise_only else [
            (mode, n) for n in PRODUCT_SIZES for mode in ("fused", "fused+products")]
        modes += [("stepwise", n) for n in STAGE_SIZES]
        for mode, n_parcel in modes:
            results.append(measure_products(kind, n_parcel, mode, args.reps, args.warmup))
            print(json.dumps(results[-1]), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "parcel_products_timing.json")
    with open(out, "w", encoding="utf-8") as handle:
        handle.write(json.dumps({
            "workload": f"{N_SD} super-droplets per parcel, {STEPS} steps of {DT} s, updrafts "
                        "0.2 .. 5 m/s (2 m/s for one parcel); eleven products, 64 bins",
            "results": results}, indent=1) + "\n")
    print("wrote", out)


def measure_chemistry(system, n_parcel, route, reps, warmup):
    """`system`: "open", "closed", or None for the same ascent without chemistry"""
    runner = make_runner("default", n_parcel, route, 0, system=system)
    start = runner.snapshot()
    samples = timed(runner, start, STEPS, reps, warmup)
    final = runner.snapshot()
    assert (final["failed_step"] == -1).all() and (final["steps_done"] == STEPS).all()
    ms = float(np.median(samples))
    out = {"chemistry": system or "none", "route": route, "n_parcel": n_parcel,
           "n_sd_per_parcel": N_SD, "steps": STEPS, "reps": reps, "ms_median": round(ms, 3),
           "ms_min": round(float(np.min(samples)), 3), "ms_max": round(float(np.max(samples)), 3),
           "ms_per_parcel_step": round(ms / (n_parcel * STEPS), 5)}
    if system is not None:
        out["n_substep"] = CHEM_SUBSTEPS
        out["n_flagged_last"] = [int(v) for v in runner.last_chem_profile["n_flagged"][-1][
            [0, -1]]] if runner.last_chem_profile is not None else None
        out["counts"] = [int(final[name].sum()) for name in
                         ("n_failed", "n_negative", "n_exceeded")]
    return out


def main_chemistry(args):
    results = []
    for system in (None, "open", "closed"):
        for n_parcel in SIZES:
            results.append(measure_chemistry(system, n_parcel, "fused", args.reps, args.warmup))
            print(json.dumps(results[-1]), flush=True)
        if system is not None:
            for n_parcel in STAGE_SIZES:
                results.append(measure_chemistry(system, n_parcel, "stages", args.reps,
                                                 args.warmup))
                print(json.dumps(results[-1]), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "parcel_chem_timing.json")
    with open(out, "w", encoding="utf-8") as handle:
        handle.write(json.dumps({
            "workload": f"{N_SD} super-droplets per parcel, {STEPS} steps of {DT} s, updrafts "
                        f"0.2 .. 5 m/s (2 m/s for one parcel); PySDM's default formulae; "
                        f"AqueousChemistry with n_substep = {CHEM_SUBSTEPS}; HIP events, median of "
                        f"{args.reps} after {args.warmup} warm-up call(s)",
            "results": results}, indent=1) + "\n")
    print("wrote", out)


VENTILATION, VENTILATION_LAW = "PruppacherAndRasmussen1979", "GunnKinzer1949"


def measure_ventilation(mode, n_parcel, route, reps, warmup):
    """`mode`: "ventilated" (k_parcel_v), "neglect" (PySDM's defaults: k_parcel) or
    "neglect-general" (the same through the general kernel k_parcel_f, which k_parcel_v extends)"""
    from pysdm_amd import spectra  # pylint: disable=import-outside-toplevel
    from pysdm_amd.condensation import CondensationSetup  # pylint: disable=import-outside-toplevel
    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel
    from pysdm_amd.formulae import Formulae  # pylint: disable=import-outside-toplevel
    from pysdm_amd.parcel import ParcelRunner  # pylint: disable=import-outside-toplevel

    ventilated = mode == "ventilated"
    formulae = Formulae(ventilation=VENTILATION) if ventilated else Formulae()
    updrafts = np.linspace(0.2, 5.0, n_parcel) if n_parcel > 1 else np.array([2.0])
    runner = ParcelRunner.from_spectrum(
        HipEngine.get(), formulae, CondensationSetup(), dt=DT, T0=290.0, p0=100000.0, qv0=0.012,
        w=updrafts, mass_of_dry_air=1.0,
        spectrum=spectra.Lognormal(norm_factor=60e6 / 1.18, m_mode=0.04e-6, s_geom=1.4),
        kappa=1.28, n_sd=N_SD, n_parcel=n_parcel, route=route, general=mode == "neglect-general",
        terminal_velocity=VENTILATION_LAW if ventilated else None)
    start = runner.snapshot()
    samples = timed(runner, start, STEPS, reps, warmup)
    final = runner.snapshot()
    assert (final["failed_step"] == -1).all() and (final["steps_done"] == STEPS).all()
    ms = float(np.median(samples))
    out = {"mode": mode, "route": route, "n_parcel": n_parcel, "n_sd_per_parcel": N_SD,
           "steps": STEPS, "reps": reps, "ms_median": round(ms, 3),
           "ms_min": round(float(np.min(samples)), 3), "ms_max": round(float(np.max(samples)), 3),
           "ms_per_parcel_step": round(ms / (n_parcel * STEPS), 5)}
    if ventilated:
        out["reynolds_number_max_last"] = float(final["reynolds_number"].max())
    return out


def main_ventilation(args):
    results = []
    for mode in ("neglect", "neglect-general", "ventilated"):
        for n_parcel in SIZES:
            results.append(measure_ventilation(mode, n_parcel, "fused", args.reps, args.warmup))
            print(json.dumps(results[-1]), flush=True)
    for n_parcel in STAGE_SIZES:
        results.append(measure_ventilation("ventilated", n_parcel, "stages", args.reps,
                                           args.warmup))
        print(json.dumps(results[-1]), flush=True)
    by = {(r["mode"], r["route"], r["n_parcel"]): r["ms_median"] for r in results}
    ratios = {
        "fused ventilated / fused neglect": {
            str(n): round(by["ventilated", "fused", n] / by["neglect", "fused", n], 3)
            for n in SIZES},
        "fused ventilated / fused neglect-general": {
            str(n): round(by["ventilated", "fused", n] / by["neglect-general", "fused", n], 3)
            for n in SIZES},
        "stages ventilated / fused ventilated": {
            str(n): round(by["ventilated", "stages", n] / by["ventilated", "fused", n], 3)
            for n in STAGE_SIZES}}
    out = args.out or os.path.join(ROOT, "profiles", "parcel_vent_timing.json")
    with open(out, "w", encoding="utf-8") as handle:
        handle.write(json.dumps({
            "workload": f"{N_SD} super-droplets per parcel, {STEPS} steps of {DT} s, updrafts "
                        f"0.2 .. 5 m/s (2 m/s for one parcel); PySDM's default formulae, with "
                        f"ventilation {VENTILATION} and the law {VENTILATION_LAW} or without; HIP "
                        f"events, median of {args.reps} after {args.warmup} warm-up call(s)",
            "results": results, "ratios": ratios}, indent=1) + "\n")
    print(json.dumps(ratios))
    print("wrote", out)


COAL_PARCELS, COAL_STEPS = 1024, 20
COAL_DRIZZLE_RADII = (10e-6, 50e-6)


def measure_coalescence(mode, n_parcel, reps, warmup, spectrum="haze", engine=None):
    """`mode`: "fused" (sdm_parcel_run_coal), "stages" (the stage step, then sdm_collision_step with
    n_cell = 1, parcel by parcel) or "condensation only" (sdm_parcel_run, one step per launch).
    `spectrum`: "haze" (the aerosol of the other measurements at equilibrium: the Geometric kernel
    finds next to nothing to collect in 20 s, so a step is one sub-step of shuffle, pairing and
    probabilities) or "drizzle" (the same rows with seeded radii of 10 - 50 micrometres: pairs
    coalesce)"""
    from pysdm_amd import recipe  # pylint: disable=import-outside-toplevel

    more = {}
    if mode != "condensation only":
        more["collisions"] = recipe.CollisionSetup.coalescence(recipe.Geometric(), adaptive=True)
    runner = make_runner("default", n_parcel, "stages" if mode == "stages" else "fused",
                         1 if mode == "condensation only" else 0, engine=engine, **more)
    if spectrum == "drizzle":
        rng = np.random.default_rng(11)
        radii = np.exp(rng.uniform(*np.log(COAL_DRIZZLE_RADII), runner.n_sd))
        runner.restore({"water_mass": 1000.0 * 4 / 3 * np.pi * radii ** 3})
    start = runner.snapshot()
    samples = timed(runner, start, COAL_STEPS, reps, warmup)
    final = runner.snapshot()
    assert (final["failed_step"] == -1).all() and (final["steps_done"] == COAL_STEPS).all()
    ms = float(np.median(samples))
    out = {"mode": mode, "spectrum": spectrum, "n_parcel": n_parcel, "n_sd_per_parcel": N_SD,
           "steps": COAL_STEPS,
           "reps": reps, "ms_median": round(ms, 3), "ms_min": round(float(np.min(samples)), 3),
           "ms_max": round(float(np.max(samples)), 3),
           "ms_per_parcel_step": round(ms / (n_parcel * COAL_STEPS), 5)}
    if mode != "condensation only":
        out["collision_substeps_per_step"] = round(
            float(runner.last_coal_profile["n_substeps"].mean()), 2)
        out["coalescence_rate_total"] = int(final["coalescence_rate"].sum())
        out["n_live_min"] = int(final["n_live"].min())
    return out


def main_coalescence(args):
    results = []
    for spectrum in ("haze", "drizzle"):
        for mode in ("condensation only", "fused", "stages"):
            # (the stage route: some 20 s per call at this shape; one call, no warm-up)
            reps, warmup = (1, 0) if mode == "stages" else (args.reps, args.warmup)
            results.append(measure_coalescence(mode, COAL_PARCELS, reps, warmup, spectrum))
            print(json.dumps(results[-1]), flush=True)
    by = {(r["mode"], r["spectrum"]): r["ms_median"] for r in results}
    ratios = {
        f"{spectrum}: {name}": round(by[top, spectrum] / by[bottom, spectrum], 3)
        for spectrum in ("haze", "drizzle")
        for name, top, bottom in (
            ("fused with coalescence / condensation only", "fused", "condensation only"),
            ("stages / fused", "stages", "fused"))}
    out = args.out or os.path.join(ROOT, "profiles", "parcel_coal_timing.json")
    with open(out, "w", encoding="utf-8") as handle:
        handle.write(json.dumps({
            "workload": f"{N_SD} super-droplets per parcel, {COAL_STEPS} steps of {DT} s, updrafts "
                        "0.2 .. 5 m/s; PySDM's default formulae; Coalescence(Geometric()), "
                        f"adaptive, Gunn-Kinzer table; {COAL_PARCELS} parcels on every route; "
                        "spectrum haze: the aerosol at equilibrium (next to no coalescence: one "
                        "sub-step of shuffle and probabilities per step), drizzle: seeded radii of "
                        f"10 - 50 micrometres (pairs coalesce); HIP events, median of {args.reps} "
                        f"after {args.warmup} warm-up call(s) (the stage route: one call)",
            "results": results, "ratios": ratios}, indent=1) + "\n")
    print(json.dumps(ratios))
    print("wrote", out)


BREAKUP_STEPS = 10


def breakup_collisions():
    """the set-up of --breakup: half of the colliding pairs coalesce, the others break up into
    Straub's fragments (at most 10 of them, none below a radius of 5 micrometres)"""
    from pysdm_amd import recipe  # pylint: disable=import-outside-toplevel

    return recipe.CollisionSetup.collision(
        recipe.Geometric(), recipe.ConstEc(0.5), recipe.ConstEb(1.0),
        recipe.Straub2010Nf(vmin=4 / 3 * np.pi * 5e-6 ** 3, nfmax=10), adaptive=True)


def measure_breakup(mode, n_parcel, reps, warmup, engine=None, time_it=timed):
    """`mode`: "fused" (sdm_parcel_run_collision), "stages" (the stage step, then
    sdm_collision_step with n_cell = 1 and breakup, parcel by parcel) or "coalescence only"
    (sdm_parcel_run_coal on the same drops)"""
    from pysdm_amd import recipe  # pylint: disable=import-outside-toplevel

    breakup = mode != "coalescence only"
    collisions = breakup_collisions() if breakup else recipe.CollisionSetup.coalescence(
        recipe.Geometric(), adaptive=True)
    runner = make_runner("default", n_parcel, "stages" if mode == "stages" else "fused", 0,
                         engine=engine, collisions=collisions, breakup=breakup)
    rng = np.random.default_rng(11)
    radii = np.exp(rng.uniform(*np.log(COAL_DRIZZLE_RADII), runner.n_sd))
    runner.restore({"water_mass": 1000.0 * 4 / 3 * np.pi * radii ** 3})
    start = runner.snapshot()
    samples = time_it(runner, start, BREAKUP_STEPS, reps, warmup)
    final = runner.snapshot()
    assert (final["failed_step"] == -1).all() and (final["steps_done"] == BREAKUP_STEPS).all()
    ms = float(np.median(samples))
    out = {"mode": mode, "n_parcel": n_parcel, "n_sd_per_parcel": N_SD, "steps": BREAKUP_STEPS,
           "reps": reps, "ms_median": round(ms, 3), "ms_min": round(float(np.min(samples)), 3),
           "ms_max": round(float(np.max(samples)), 3),
           "ms_per_parcel_step": round(ms / (n_parcel * BREAKUP_STEPS), 5),
           "collision_substeps_per_step": round(
               float(runner.last_coal_profile["n_substeps"].mean()), 2),
           "coalescence_rate_total": int(final["coalescence_rate"].sum()),
           "n_live_min": int(final["n_live"].min())}
    if breakup:
        assert final["breakup_rate"].sum() > 0  # a set-up in which breakups happen
        out["breakup_rate_total"] = int(final["breakup_rate"].sum())
        out["breakup_rate_deficit_total"] = int(final["breakup_rate_deficit"].sum())
        out["n_overflow_total"] = int(runner.last_coal_profile["n_overflow"].sum())
    return out


def main_breakup(args):
    results = []
    for mode in ("coalescence only", "fused", "stages"):
        # (the stage route: seconds per call at this shape; one call, no warm-up)
        reps, warmup = (1, 0) if mode == "stages" else (args.reps, args.warmup)
        results.append(measure_breakup(mode, COAL_PARCELS, reps, warmup))
        print(json.dumps(results[-1]), flush=True)
    by = {r["mode"]: r["ms_median"] for r in results}
    ratios = {"stages / fused": round(by["stages"] / by["fused"], 3),
              "fused with breakup / fused with coalescence only":
                  round(by["fused"] / by["coalescence only"], 3)}
    assert by["fused"] <= by["stages"], "the fused route is slower than the stage route"
    out = args.out or os.path.join(ROOT, "profiles", "parcel_breakup_timing.json")
    with open(out, "w", encoding="utf-8") as handle:
        handle.write(json.dumps({
            "workload": f"{N_SD} super-droplets per parcel, {BREAKUP_STEPS} steps of {DT} s, "
                        "updrafts 0.2 .. 5 m/s; PySDM's default formulae; seeded radii of 10 - 50 "
                        "micrometres; Collision(Geometric(), ConstEc(0.5), ConstEb(1), "
                        "Straub2010Nf(vmin: r = 5 um, nfmax = 10)), adaptive, Gunn-Kinzer table; "
                        f"{COAL_PARCELS} parcels on every route; HIP events, median of {args.reps} "
                        f"after {args.warmup} warm-up call(s) (the stage route: one call)",
            "results": results, "ratios": ratios}, indent=1) + "\n")
    print(json.dumps(ratios))
    print("wrote", out)


ICE_PARCELS, ICE_STEPS = 1024, 20


def measure_ice(mode, n_parcel, reps, warmup, engine=None, time_it=timed):
    """`mode`: "fused" (sdm_parcel_run_ice), "stages" (the chain of stage symbols) or
    "condensation only" (sdm_parcel_run on the same rows)"""
    from pysdm_amd.condensation import CondensationSetup  # pylint: disable=import-outside-toplevel
    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel
    from pysdm_amd.formulae import Formulae  # pylint: disable=import-outside-toplevel
    from pysdm_amd.parcel import ParcelRunner  # pylint: disable=import-outside-toplevel
    from tests import parcel_cases as pc  # pylint: disable=import-outside-toplevel
    from tests import parcel_ice_cases as ic  # pylint: disable=import-outside-toplevel

    engine = engine or HipEngine.get()
    kwargs = ic.ensemble((N_SD,) * n_parcel, seed=3, mode="both")
    if mode == "condensation only":
        formulae = Formulae()
        plain = {key: value for key, value in kwargs.items() if key not in (
            "freezing_temperature", "immersed_surface_area", "ice_seed")}
        runner = ParcelRunner(engine, formulae, CondensationSetup(), route="fused",
                              **pc.saturated(plain, formulae))
        call = None
    else:
        runner = ic.runner(engine, kwargs, mode, mode="both")
        call = lambda r, steps: r.run(steps, profile=False)  # noqa: E731
    start = runner.snapshot()
    samples = time_it(runner, start, ICE_STEPS, reps, warmup, call)
    final = runner.snapshot()
    assert (final["failed_step"] == -1).all() and (final["steps_done"] == ICE_STEPS).all()
    ms = float(np.median(samples))
    out = {"mode": mode, "n_parcel": n_parcel, "n_sd_per_parcel": N_SD, "steps": ICE_STEPS,
           "reps": reps, "ms_median": round(ms, 3), "ms_min": round(float(np.min(samples)), 3),
           "ms_max": round(float(np.max(samples)), 3),
           "ms_per_parcel_step": round(ms / (n_parcel * ICE_STEPS), 5)}
    if mode != "condensation only":
        out["frozen_fraction"] = round(ic.frozen_fraction(kwargs, final), 3)
        out["n_exceeded"] = int(final["n_exceeded"].sum())
    return out


def default_line_against(parent_root, rounds):
    """the default measurement (fused route, the four parcel counts, both formulae) in the parent's
    tree and in this one, alternating, each run a process of its own; ms_median per run"""
    import subprocess  # pylint: disable=import-outside-toplevel
    import tempfile  # pylint: disable=import-outside-toplevel

    runs = []
    for round_ in range(rounds):
        for which, root in (("parent", os.path.abspath(parent_root)), ("this commit", ROOT)):
            with tempfile.NamedTemporaryFile(suffix=".json") as handle:
                subprocess.run([sys.executable, os.path.join(root, "scripts", "bench_parcel.py"),
                                "--out", handle.name], cwd=root, check=True,
                               stdout=subprocess.DEVNULL, timeout=300)
                with open(handle.name, encoding="utf-8") as result:
                    rows = json.load(result)["results"]
            runs.append({"round": round_, "tree": which, "ms_median": {
                f"{r['formulae']}, {r['n_parcel']} parcels": r["ms_median"]
                for r in rows if r["route"] == "fused"}})
            print(json.dumps(runs[-1]), flush=True)
    return runs


def main_ice(args):
    results = []
    for mode in ("condensation only", "fused", "stages"):
        # (the stage route: tens of seconds per call at this shape; one call, no warm-up)
        reps, warmup = (1, 0) if mode == "stages" else (args.reps, args.warmup)
        results.append(measure_ice(mode, ICE_PARCELS, reps, warmup))
        print(json.dumps(results[-1]), flush=True)
    by = {r["mode"]: r for r in results}
    ratios = {"stages / fused": round(by["stages"]["ms_median"] / by["fused"]["ms_median"], 1),
              "fused / condensation only":
                  round(by["fused"]["ms_median"] / by["condensation only"]["ms_median"], 3)}
    against = "not measured"
    if args.against:
        against = default_line_against(args.against, args.rounds)
    out = args.out or os.path.join(ROOT, "profiles", "parcel_ice_timing.json")
    with open(out, "w", encoding="utf-8") as handle:
        handle.write(json.dumps({
            "workload": f"{N_SD} rows per parcel, a quarter ice, {ICE_STEPS} steps of 0.1 s at 255 "
                        "- 262 K, water-saturated ascents; Freezing(singular=False, "
                        "homogeneous_freezing=True) with constant rates, then "
                        "VapourDepositionOnIce, ordered sums; HIP events, median of "
                        f"{args.reps} after {args.warmup} warm-up call(s); the stage route: one "
                        "call",
            "results": results, "ratios": ratios,
            "default measurement, this commit against the parent, alternating": against},
            indent=1) + "\n")
    print(json.dumps(ratios))
    print("wrote", out)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=1)
    parser.add_argument("--steps-per-launch", type=int, default=0, help="0: the library's default")
    parser.add_argument("--out", default=None,
                        help="default: profiles/parcel_timing.json (parcel_products_timing.json "
                             "with --products)")
    parser.add_argument("--products", action="store_true",
                        help="time the products instead (see the module's docstring)")
    parser.add_argument("--products-stepwise-only", action="store_true")
    parser.add_argument("--chemistry", action="store_true",
                        help="time the parcel with aqueous chemistry instead (see the docstring)")
    parser.add_argument("--ventilation", action="store_true",
                        help="time the ventilated parcel instead (see the docstring)")
    parser.add_argument("--coalescence", action="store_true",
                        help="time the parcel with coalescence instead (see the docstring)")
    parser.add_argument("--breakup", action="store_true",
                        help="time the parcel with collisional breakup instead (see the docstring)")
    parser.add_argument("--ice", action="store_true",
                        help="time the mixed-phase parcel instead (see the docstring)")
    parser.add_argument("--against", default=None,
                        help="with --ice: a checkout of the parent commit (library built) to run "
                             "the default measurement against, alternating")
    parser.add_argument("--rounds", type=int, default=2)
    args = parser.parse_args()
    if args.ice:
        main_ice(args)
        return
    if args.breakup:
        main_breakup(args)
        return
    if args.coalescence:
        main_coalescence(args)
        return
    if args.ventilation:
        main_ventilation(args)
        return
    if args.chemistry:
        main_chemistry(args)
        return
    if args.products or args.products_stepwise_only:
        main_products(args)
        return
    args.out = args.out or os.path.join(ROOT, "profiles", "parcel_timing.json")
    results = []
    for kind in ("default", "lowe2019"):
        for n_parcel in SIZES:
            results.append(measure(kind, n_parcel, "fused", args.reps, args.warmup,
                                   args.steps_per_launch))
            print(json.dumps(results[-1]), flush=True)
        for n_parcel in STAGE_SIZES:
            results.append(measure(kind, n_parcel, "stages", args.reps, args.warmup, 0))
            print(json.dumps(results[-1]), flush=True)
    text = json.dumps({"workload": f"{N_SD} super-droplets per parcel, {STEPS} steps of {DT} s, "
                                   "updrafts 0.2 .. 5 m/s (2 m/s for one parcel)",
                       "results": results}, indent=1)
    with open(args.out, "w", encoding="utf-8") as out:
        out.write(text + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

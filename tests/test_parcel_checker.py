"""The adiabatic parcel (include/sdm_parcel.h) without a GPU: the binding, the CPU checker
(tests/parcel_checker/) against the reference's recorded calls and free runs, the fused route
against the stage route bit for bit, resumption, failing parcels, refusals and the PySDM hook."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from pysdm_amd import abi
from pysdm_amd.condensation import CondensationSetup
from pysdm_amd.formulae import Formulae
from pysdm_amd.parcel import ParcelRunner
from tests import condensation_cases as cc
from tests import condensation_formulae_cases as fc
from tests import parcel_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = os.environ.get("PYSDM_REFERENCE", "/root/reference")
FLOATS = ("z", "rhod", "thd", "qv", "T", "p", "RH", "RH_max")
COUNTERS = ("n_substeps", "n_activating", "n_deactivating", "n_ripening")
# the bound the ambient tests use against the reference (plain double arithmetic on both sides)
INPUT_RTOL = 1e-12


@pytest.fixture(scope="module")
def engine():
    from tests.parcel_checker import ParcelCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelCheckerEngine.get()


@pytest.fixture(scope="module")
def runs():
    return np.load(os.path.join(HERE, "golden", "parcel_runs.npz"))


# ---- 1. binding ------------------------------------------------------------------------------------
def test_header_parses_and_the_symbol_binds(engine):
    table = abi.parse_header(abi.PARCEL_HEADER_PATH)
    assert list(table) == ["sdm_parcel_run"]
    params = {p.name: p for p in table["sdm_parcel_run"][1]}
    assert params["ctx"].kind == "ctx" and params["cfg"].base == "sdm_parcel_cfg"
    assert params["consts"].kind == "host_array" and params["consts"].array_len == 34
    assert params["state"].kind == params["profile"].kind == params["formulae"].kind == "pointer"
    assert hasattr(engine.parcel_library.cdll, "sdm_parcel_run")
    assert hasattr(abi.parcel_library().cdll, "sdm_parcel_run")  # the product library


def test_struct_layouts_match_the_header():
    structs = (("sdm_parcel_cfg", abi.ParcelCfg), ("sdm_parcel_state", abi.ParcelState),
               ("sdm_parcel_profile", abi.ParcelProfile))
    prints = []
    for c_name, mirror in structs:
        prints.append(f'printf("%zu\\n", sizeof({c_name}));')
        prints += [f'printf("%zu\\n", offsetof({c_name}, {field}));'
                   for field, _ in mirror._fields_]  # pylint: disable=protected-access
    source = ('#include "include/sdm_parcel.h"\n#include <stddef.h>\n#include <stdio.h>\n'
              "int main(){" + "".join(prints) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w", encoding="utf-8") as handle:
            handle.write(source)
        subprocess.check_call(["gcc", "-I", ROOT, src, "-o", exe], cwd=ROOT)
        numbers = [int(x) for x in subprocess.check_output([exe]).split()]
    expected = []
    for _, mirror in structs:
        expected.append(ctypes.sizeof(mirror))
        expected += [getattr(mirror, field).offset for field, _ in mirror._fields_]  # pylint: disable=protected-access
    assert numbers == expected


def test_an_engine_without_a_parcel_library_says_so(oracle_engine):
    with pytest.raises(NotImplementedError, match="no parcel library"):
        oracle_engine.call_parcel("sdm_parcel_run")
    from tests.checker import CheckerEngine  # pylint: disable=import-outside-toplevel

    kwargs = pc.ensemble((5, 9), seed=3)
    with pytest.raises(NotImplementedError, match="no parcel library.*route='fused'"):
        pc.runner(CheckerEngine.get(), "default", kwargs, "fused")
    # ... and gets the stage route
    stages = pc.runner(CheckerEngine.get(), "default", kwargs, "stages")
    stages.run(2)
    assert stages.snapshot()["steps_done"].tolist() == [2, 2]


# ---- 2. lockstep against the reference's recorded calls ---------------------------------------------
LOCKSTEP = {"cond_parcel_a1": ("default", True), "cond_parcel_a0": ("default", False),
            "condf_parcel_lowe2019": ("lowe2019", True)}
# recorded calls whose adaptive error estimate sits within 1e-10 (relative) of its threshold and
# whose counters may therefore differ: {golden: {call: (recorded, computed)}}; at most 2 of the 89
COUNTER_EXCEPTIONS = {}


def _replay_bound(name, key):
    if name == "condf_parcel_lowe2019":
        return fc.golden_rtol("parcel_lowe2019", key) + INPUT_RTOL
    return cc.GOLDEN_RTOL[key] + INPUT_RTOL


@pytest.mark.parametrize("route", ("fused", "stages"))
@pytest.mark.parametrize("name", sorted(LOCKSTEP))
def test_one_step_from_every_recorded_state(engine, name, route):
    """for every recorded call k >= 1: the state the golden holds before call k restored, ONE
    step, and what the reference computed: prhod, dv and v_cr (plain double arithmetic from the
    recorded inputs) at 1e-12; water mass, pthd, pqv and RH_max at the replay bounds of the
    condensation tests plus 1e-12 (the inputs' own tolerance; the outputs' relative sensitivity to
    the inputs is below one); counters exactly; success"""
    data = cc.gold(name)
    kind, adaptive = LOCKSTEP[name]
    assert bool(data["solver/adaptive"]) == adaptive
    n_sd, n_calls = int(data["parcel/n_sd"]), int(data["n_calls"])
    assert np.array_equal(data["idx"], np.arange(n_sd))  # the sum order is row order
    dt, mass_of_dry_air = float(data["parcel/dt"]), float(data["parcel/mass_of_dry_air"])
    setup = CondensationSetup(adaptive=adaptive, dt_cond_range=tuple(data["solver/dt_range"]),
                              max_iters=int(data["solver/max_iters"]),
                              rtol_x=float(data["calls/rtol_x"][0]),
                              rtol_thd=float(data["calls/rtol_thd"][0]))
    runner = ParcelRunner(
        engine, pc.formulae_of(kind), setup, dt=dt, T0=float(data["parcel/T0"]),
        p0=float(data["parcel/p0"]), qv0=float(data["parcel/qv0"]), w=float(data["parcel/w"]),
        mass_of_dry_air=mass_of_dry_air, counts=[n_sd], multiplicity=data["multiplicity"],
        water_mass=data["calls/water_mass"][0], dry_volume=data["vdry"], kappa=data["kappa"],
        f_org=data["f_org"], route=route)
    qv_key = "water_vapour_mixing_ratio"
    listed = COUNTER_EXCEPTIONS.get(name, {})
    for k in range(1, n_calls):
        for key in ("rhod", "thd", qv_key):  # the recorded inputs chain
            previous = "prhod" if key == "rhod" else f"out_p{key}" if key == "thd" \
                else "out_predicted_" + qv_key
            assert np.array_equal(data[f"calls/{key}"][k], data[f"calls/{previous}"][k - 1])
        assert np.array_equal(data["calls/water_mass"][k], data["calls/out_water_mass"][k - 1])
        runner.restore({
            "rhod": data["calls/rhod"][k], "thd": data["calls/thd"][k],
            "qv": data[f"calls/{qv_key}"][k], "qv_prev": data[f"calls/{qv_key}"][k - 1],
            "water_mass": data["calls/water_mass"][k], "steps_done": k, "failed_step": -1,
            "n_steps": k,
            **{c: data[f"calls/in_{c}"][k] for c in cc.COUNTERS}})
        profile = runner.run(1)
        after = runner.snapshot()
        assert after["failed_step"].tolist() == [-1] and after["steps_done"].tolist() == [k + 1]
        prhod = profile["rhod"][0]
        np.testing.assert_allclose(prhod, data["calls/prhod"][k], rtol=INPUT_RTOL, atol=0)
        dv = mass_of_dry_air / ((prhod + data["calls/rhod"][k]) / 2)
        np.testing.assert_allclose(dv, data["calls/dv"][k], rtol=INPUT_RTOL, atol=0)
        np.testing.assert_allclose(after["critical_volume"], data["calls/v_cr"][k],
                                   rtol=INPUT_RTOL, atol=0)
        for key, got in (("water_mass", after["water_mass"]), ("pthd", profile["thd"][0]),
                         ("predicted_" + qv_key, profile["qv"][0]),
                         ("RH_max", profile["RH_max"][0])):
            np.testing.assert_allclose(got, data[f"calls/out_{key}"][k], atol=0,
                                       rtol=_replay_bound(name, key), err_msg=f"{key}, call {k}")
        assert int(data["calls/out_success"][k][0]) == 1
        counters = {c: int(data[f"calls/out_{c}"][k][0]) for c in cc.COUNTERS}
        if adaptive:  # the state holds the count after the clamp of dynamics/condensation.py
            counters["n_substeps"] = min(max(counters["n_substeps"], int(runner.cfg.n_clamp_lo)),
                                         int(runner.cfg.n_clamp_hi))
        computed = {c: int(profile[c][0, 0]) for c in cc.COUNTERS}
        if k in listed:
            assert listed[k] == (counters, computed)
        else:
            assert computed == counters, f"call {k}"
    assert len(listed) <= 2


# ---- 3. free runs against the reference ---------------------------------------------------------------
def _free_bound(runs, run, quantity):
    """max(4 x the reference's own spread, the per-call bound of the lockstep test); the factor 4
    is the project's margin over a measured worst case (condensation_formulae_cases.golden_rtol).
    T and p follow thd (they are smooth functions of rhod and thd), RH follows RH_max"""
    name = "condf_parcel_lowe2019" if run == "c" else "cond_parcel_a1"
    per_call = {"rhod": INPUT_RTOL, "thd": _replay_bound(name, "pthd"),
                "qv": _replay_bound(name, "predicted_water_vapour_mixing_ratio"),
                "T": _replay_bound(name, "pthd"), "p": _replay_bound(name, "pthd"),
                "RH": _replay_bound(name, "RH_max"), "RH_max": _replay_bound(name, "RH_max"),
                "water_mass": _replay_bound(name, "water_mass")}[quantity]
    return max(4 * float(runs[f"spread/{run}/{quantity}"]), per_call)


def assert_matches_the_reference(runs, run, profile, final_mass):
    np.testing.assert_array_equal(profile["z"][:, 0].view(np.uint8),
                                  np.array(runs[f"{run}/profile/z"]).view(np.uint8))
    for quantity in FLOATS[1:]:
        np.testing.assert_allclose(profile[quantity][:, 0], runs[f"{run}/profile/{quantity}"],
                                   rtol=_free_bound(runs, run, quantity), atol=0,
                                   err_msg=f"run {run}: {quantity}")
    for counter in COUNTERS:
        np.testing.assert_array_equal(profile[counter][:, 0], runs[f"{run}/profile/{counter}"],
                                      err_msg=f"run {run}: {counter}")
    np.testing.assert_allclose(final_mass, runs[f"{run}/final/water_mass"], atol=0,
                               rtol=_free_bound(runs, run, "water_mass"))


@pytest.fixture(scope="module")
def free_runs(engine, runs):
    """the three recorded ascents on both routes of the checker: computed once"""
    out = {}
    for run in "abc":
        for route in ("fused", "stages"):
            runner = pc.golden_runner(engine, runs, run, route)
            profile = runner.run(int(runs[f"{run}/cfg/n_steps"]))
            out[run, route] = (runner.snapshot(), profile)
    return out


@pytest.mark.parametrize("route", ("fused", "stages"))
@pytest.mark.parametrize("run", "abc")
def test_free_run_against_the_reference(runs, free_runs, run, route):
    snapshot, profile = free_runs[run, route]
    assert snapshot["failed_step"].tolist() == [-1]  # success throughout
    assert_matches_the_reference(runs, run, profile, snapshot["water_mass"])
    if run == "b":
        assert profile["n_deactivating"].max() > 0 and runs["b/w_mid"].min() < 0


# ---- 4. fused == stage route, bit for bit --------------------------------------------------------------
@pytest.mark.parametrize("run", "abc")
def test_fused_equals_stages_on_the_recorded_runs(free_runs, run):
    pc.assert_same_bits(free_runs[run, "fused"][0], free_runs[run, "stages"][0], "state")
    pc.assert_same_bits(free_runs[run, "fused"][1], free_runs[run, "stages"][1], "profile")


@pytest.mark.parametrize("adaptive", (True, False), ids=("adaptive", "fixed"))
@pytest.mark.parametrize("kind", ("default", "lowe2019"))
def test_fused_equals_stages_on_the_edge_ensemble(engine, kind, adaptive):
    """parcels of 1, 63, 64, 65, 256, 257, 1024, 1025 and 2100 rows (COND_CB = 256, COND_CH =
    1024), differing in T0, p0, qv0 and mass_of_dry_air, w of both signs, 6 steps"""
    kwargs = pc.ensemble(f_org=kind != "default")
    assert (np.asarray(kwargs["w"]) > 0).any() and (np.asarray(kwargs["w"]) < 0).any()
    results = []
    for route in ("fused", "stages"):
        runner = pc.runner(engine, kind, kwargs, route, adaptive=adaptive)
        profile = runner.run(6)
        results.append((runner.snapshot(), profile))
    assert (results[0][0]["steps_done"] == 6).all()
    pc.assert_same_bits(results[0][0], results[1][0], "state")
    pc.assert_same_bits(results[0][1], results[1][1], "profile")


def test_from_spectrum_builds_parcels_in_equilibrium(engine):
    """`from_spectrum`: the same bins of the dry spectrum in every parcel, wet radii in Koehler
    equilibrium with each parcel's own air (so the first step changes the masses little), and the
    two routes agree on an ascent that activates"""
    from pysdm_amd import spectra  # pylint: disable=import-outside-toplevel

    results = []
    for route in ("fused", "stages"):
        runner = ParcelRunner.from_spectrum(
            engine, Formulae(), CondensationSetup(), dt=1.0, T0=[290.0, 288.0], p0=100000.0,
            qv0=[0.012, 0.0105], w=[4.0, 0.5], mass_of_dry_air=1.0, n_sd=40, n_parcel=2,
            spectrum=spectra.Lognormal(norm_factor=60e6 / 1.18, m_mode=0.04e-6, s_geom=1.4),
            kappa=1.28, route=route)
        start = runner.snapshot()
        assert runner.n_sd == 80 and runner.parcel_start_host.tolist() == [0, 40, 80]
        dry = engine.download(runner.dry_volume)
        assert np.array_equal(dry[:40], dry[40:])
        assert (start["water_mass"] > 1000.0 * dry).all()
        first = runner.run(1)
        np.testing.assert_allclose(runner.snapshot()["water_mass"], start["water_mass"],
                                   rtol=0.2)
        rest = runner.run(39)
        assert rest["n_activating"][:, 0].max() > 0
        results.append((runner.snapshot(), first, rest))
    for a, b in zip(*results):
        pc.assert_same_bits(a, b, "fused vs stages")


# ---- 5. chunking and resumption ------------------------------------------------------------------------
@pytest.mark.parametrize("route", ("fused", "stages"))
def test_chunking_and_resumption(engine, route):
    kwargs = pc.ensemble((3, 65, 300, 1100), seed=13)

    def rows(parts):
        return {key: np.concatenate([part[key] for part in parts]) for key in parts[0]}

    reference = pc.runner(engine, "default", kwargs, "fused", steps_per_launch=4)
    ref = (reference.run(9), reference.snapshot())
    for split, spl in (((9,), 9), ((9,), 1), ((4, 5), 0), ((1,) * 9, 0)):
        runner = pc.runner(engine, "default", kwargs, route, steps_per_launch=spl)
        parts = [runner.run(n) for n in split]
        pc.assert_same_bits(ref[1], runner.snapshot(), f"state, {split}, {spl}")
        pc.assert_same_bits(ref[0], rows(parts), f"profile, {split}, {spl}")


# ---- 6. failure -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,setup,sizes,seed", pc.FAILURE_CASES, ids=pc.FAILURE_IDS)
def test_failed_parcels_stop_and_the_others_go_on(engine, kind, setup, sizes, seed):  # pylint: disable=too-many-locals
    """`failed_step` is the step at which the stage route fails for that parcel; a failed parcel's
    columns equal its state before that step; the others equal their solo runs; `run` raises
    afterwards, and a further `run` leaves failed parcels untouched"""
    kwargs = pc.ensemble(sizes, seed=seed, f_org=kind != "default")
    n_parcel = len(sizes)
    ensemble = {}
    for route in ("fused", "stages"):
        runner = pc.runner(engine, kind, kwargs, route, setup=setup)
        with pytest.raises(RuntimeError, match="Condensation failed") as raised:
            runner.run(5)
        ensemble[route] = runner
        failed = runner.snapshot()["failed_step"]
        first = int(np.flatnonzero(failed >= 0)[0])
        assert raised.value.args == ("Condensation failed", first, int(failed[first]))
    state = ensemble["fused"].snapshot()
    # failed_step equals the step at which the stage route fails for that parcel
    pc.assert_same_bits(state, ensemble["stages"].snapshot(), "fused vs stages")
    failed = state["failed_step"]
    assert (failed >= 0).any() and (failed == -1).any()
    starts = ensemble["fused"].parcel_start_host
    formulae = pc.formulae_of(kind)
    full = pc.saturated(kwargs, formulae)
    for c in range(n_parcel):  # every parcel against its solo run
        rows = slice(int(starts[c]), int(starts[c + 1]))
        solo_kwargs = {key: (value if key == "dt" else value[rows] if key in (
            "multiplicity", "water_mass", "dry_volume", "kappa", "f_org") and value is not None
                             else None if value is None else np.asarray(value)[c:c + 1])
                       for key, value in full.items()}
        solo = ParcelRunner(engine, formulae, setup, route="fused", **solo_kwargs)
        steps = 5 if failed[c] < 0 else int(failed[c])
        solo.run(steps)  # a failed parcel's columns equal its state before that step
        alone = solo.snapshot()
        for key in pc.STATE_KEYS:
            if key in ("failed_step",) or (key == "critical_volume" and failed[c] >= 0):
                continue  # (v_cr is the failed step's own: an output, not state)
            per_row = key in ("water_mass", "critical_volume")
            got = state[key][rows] if per_row else state[key][c:c + 1]
            assert np.array_equal(pc.bits(got), pc.bits(alone[key])), (c, key)
    # a further run leaves failed parcels untouched and does not raise again for them (it
    # raises for a parcel that fails only now)
    try:
        ensemble["fused"].run(2)
    except RuntimeError as error:
        assert failed[error.args[1]] == -1 and error.args[2] >= 5
    again = ensemble["fused"].snapshot()
    for key in pc.STATE_KEYS:
        per_row = key in ("water_mass", "critical_volume")
        for c in np.flatnonzero(failed >= 0):
            rows = slice(int(starts[c]), int(starts[c + 1])) if per_row else slice(c, c + 1)
            assert np.array_equal(pc.bits(again[key][rows]), pc.bits(state[key][rows])), (c, key)
    going = again["failed_step"] == -1
    assert (again["steps_done"][going] == 7).all() and going.any()


# ---- 7. refusals ------------------------------------------------------------------------------------------
def test_refusals(engine):
    kwargs = pc.saturated(pc.ensemble((5, 9), seed=3), Formulae())
    setup = CondensationSetup()
    with pytest.raises(ValueError, match="at least one super-droplet"):
        ParcelRunner(engine, Formulae(), setup, **{**kwargs, "counts": [14, 0]})
    # the library itself refuses a parcel without rows
    good = ParcelRunner(engine, Formulae(), setup, **kwargs)
    good.parcel_start = engine.upload(np.array([0, 14, 14], dtype=np.int64))
    with pytest.raises(RuntimeError, match="no rows"):
        good.run(1)
    ventilated = Formulae(ventilation="PruppacherAndRasmussen1979")
    with pytest.raises(NotImplementedError, match="ventilation"):
        ParcelRunner(engine, ventilated, setup, **kwargs)
    with pytest.raises(ValueError, match="non-zero"):
        ParcelRunner(engine, Formulae(), setup, **{**kwargs, "w": [1.0, 0.0]}).run(1)
    with pytest.raises(ValueError, match="non-zero"):
        ParcelRunner(engine, Formulae(), setup,
                     **{**kwargs, "w": lambda t: 0.0 if t > 2 else 1.0}).run(4)
    # dt_min == 0: CondensationSetup refuses it, and so does the library
    with pytest.raises(NotImplementedError, match="dt_cond_range"):
        CondensationSetup(dt_cond_range=(0, 1.0))
    runner = ParcelRunner(engine, Formulae(), setup, **kwargs)
    runner.cfg.dt_min = 0.0
    with pytest.raises(RuntimeError, match="dt_min"):
        runner.run(1)
    foreign = Formulae()
    foreign.hydrostatics = "Default"
    with pytest.raises(NotImplementedError, match="hydrostatics"):
        ParcelRunner(engine, foreign, setup, **kwargs)


# ---- 8. the PySDM hook ------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "PySDM")),
                    reason="reference tree not present")
def test_run_parcel_leaves_the_particulator_as_run_would(engine, runs):  # pylint: disable=unused-argument,too-many-locals
    os.environ.setdefault("CI", "1")
    added = [os.path.join(HERE, "golden", "standins"), REFERENCE]
    sys.path[:0] = added
    try:
        from PySDM import Builder  # pylint: disable=import-outside-toplevel,import-error
        from PySDM import Formulae as PySDMFormulae  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.dynamics import AmbientThermodynamics, Condensation  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.environments import Parcel  # pylint: disable=import-outside-toplevel,import-error
    except Exception as error:  # pylint: disable=broad-except
        pytest.skip(f"PySDM not importable here: {error}")
    finally:
        for path in added:
            sys.path.remove(path)
    from pysdm_amd.pysdm_plugin import as_pysdm_backend, run_parcel  # pylint: disable=import-outside-toplevel
    from tests.parcel_checker import ParcelCheckerBackend  # pylint: disable=import-outside-toplevel

    gold = cc.gold("cond_parcel_a1")
    cfg = {k[len("parcel/"):]: gold[k] for k in gold.files if k.startswith("parcel/")}

    def twin():
        backend = as_pysdm_backend(ParcelCheckerBackend)(PySDMFormulae())
        env = Parcel(dt=float(cfg["dt"]), mass_of_dry_air=float(cfg["mass_of_dry_air"]),
                     p0=float(cfg["p0"]), initial_water_vapour_mixing_ratio=float(cfg["qv0"]),
                     T0=float(cfg["T0"]), w=lambda t: 5.0 if t < 6 else 3.0)
        builder = Builder(n_sd=int(cfg["n_sd"]), backend=backend, environment=env)
        builder.add_dynamic(AmbientThermodynamics())
        builder.add_dynamic(Condensation(adaptive=True))
        attributes = {k[len("init/"):]: np.array(gold[k]) for k in gold.files
                      if k.startswith("init/")}
        return builder.build(attributes=attributes, products=())

    def state_of(particulator):
        env, cond = particulator.environment, particulator.dynamics["Condensation"]
        out = {"n_steps": np.asarray(particulator.n_steps), "dv": np.asarray(env.mesh.dv),
               "delta": np.asarray(env.delta_liquid_water_mixing_ratio),
               "success": cond.success.to_ndarray(), "rh_max": cond.rh_max.to_ndarray()}
        for name in ("signed water mass", "multiplicity", "dry volume", "kappa",
                     "critical volume"):
            out[name] = particulator.attributes[name].to_ndarray(raw=True)
        for var in env.variables:
            out["current/" + var] = env[var].to_ndarray()
            out["tmp/" + var] = env._tmp[var].to_ndarray()  # pylint: disable=protected-access
        for name, counter in cond.counters.items():
            out[name] = counter.to_ndarray()
        return out

    def same(a, b, what):
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(pc.bits(np.asarray(a[key])), pc.bits(np.asarray(b[key]))), (
                what, key, a[key], b[key])

    stepped, fused = twin(), twin()
    stepped.run(10)
    run_parcel(fused, 10)
    same(state_of(stepped), state_of(fused), "after 10 steps")
    stepped.run(1)
    fused.run(1)
    same(state_of(stepped), state_of(fused), "after one further particulator.run(1)")
    run_parcel(fused, 1)
    stepped.run(1)
    same(state_of(stepped), state_of(fused), "after one further run_parcel(1)")
    fused.dynamics["Extra"] = object()
    with pytest.raises(ValueError, match="exactly the dynamics"):
        run_parcel(fused, 1)

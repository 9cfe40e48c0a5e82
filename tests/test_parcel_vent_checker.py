"""The ventilated parcel (include/sdm_parcel_vent.h) without a GPU: the binding, the CPU checker
(tests/parcel_vent_checker/) on its fused call against the stage route over the existing checkers'
symbols, continuation, the timing of the carried air pair, the qualitative physics, the table's
range, a failing solver, the products and the refusals.  Every comparison of two routes is bit for
bit (floats viewed as integers): both sides run the same functions."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from pysdm_amd import abi
from pysdm_amd import terminal_velocity as tv
from pysdm_amd.condensation import CONSTANT_NAMES, CondensationSetup
from pysdm_amd.formulae import Formulae
from pysdm_amd.parcel import ParcelRunner, _vent_struct, parcel_call, parcel_cfg, vent_law
from tests import parcel_cases as pc
from tests import parcel_products_cases as ppc
from tests import parcel_vent_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
from tests.test_parcel_checker import REFERENCE  # noqa: E402  (where the reference tree lies)
PR79 = "PruppacherAndRasmussen1979"


@pytest.fixture(scope="module")
def engine():
    from tests.parcel_vent_checker import ParcelVentCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelVentCheckerEngine.get()


# ---- 0. binding ------------------------------------------------------------------------------------
def test_header_parses_and_the_symbol_binds(engine):
    table = abi.parse_header(abi.PARCEL_VENT_HEADER_PATH)
    assert list(table) == ["sdm_parcel_run_vent"]
    params = [p.name for p in table["sdm_parcel_run_vent"][1]]
    diag = [p.name for p in abi.parse_header(abi.PARCEL_DIAG_HEADER_PATH)["sdm_parcel_run_diag"][1]]
    assert params == diag + ["vent"]
    assert hasattr(engine.parcel_vent_library.cdll, "sdm_parcel_run_vent")
    assert hasattr(abi.parcel_vent_library().cdll, "sdm_parcel_run_vent")  # the product library


def test_struct_layout_matches_the_header():
    mirror = abi.ParcelVent
    prints = ['printf("%zu\\n", sizeof(sdm_parcel_vent));']
    prints += [f'printf("%zu\\n", offsetof(sdm_parcel_vent, {field}));'
               for field, _ in mirror._fields_]  # pylint: disable=protected-access
    source = ('#include "include/sdm_parcel_vent.h"\n#include <stddef.h>\n#include <stdio.h>\n'
              "int main(){" + "".join(prints) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w", encoding="utf-8") as handle:
            handle.write(source)
        subprocess.check_call(["gcc", "-I", ROOT, src, "-o", exe], cwd=ROOT)
        numbers = [int(x) for x in subprocess.check_output([exe]).split()]
    assert numbers == [ctypes.sizeof(mirror)] + [
        getattr(mirror, field).offset for field, _ in mirror._fields_]  # pylint: disable=protected-access


# ---- 1. fused == stage route -----------------------------------------------------------------------
@pytest.mark.parametrize("direction", ("up", "down"))
@pytest.mark.parametrize("law", vc.LAWS)
@pytest.mark.parametrize("ventilation", vc.VENTILATIONS)
def test_fused_equals_the_stage_route(engine, ventilation, law, direction):
    """parcels of 1, 255, 256, 257 and 1025 rows, 3 steps: the state (the air pair, the Reynolds
    column included) and the profile"""
    kwargs = vc.ascending() if direction == "up" else vc.descending()
    fused = vc.run(engine, ventilation, law, kwargs, "fused", 3)
    stages = vc.run(engine, ventilation, law, kwargs, "stages", 3)
    assert (fused[0]["steps_done"] == 3).all() and (fused[0]["failed_step"] == -1).all()
    assert set(vc.VENT_KEYS) <= set(fused[0])
    assert np.isfinite(fused[0]["reynolds_number"]).all()
    if direction == "down":  # Re of 1 .. 1000: the factor differs from 1
        assert fused[0]["reynolds_number"].min() > 0.5 and fused[0]["reynolds_number"].max() > 100
    pc.assert_same_bits(fused[0], stages[0], "state, fused vs stages")
    pc.assert_same_bits(fused[1], stages[1], "profile, fused vs stages")


# ---- 2. continuation -------------------------------------------------------------------------------
@pytest.mark.parametrize("law", ("GunnKinzer1949", "PowerSeries"))
def test_continuation(engine, law):
    """run(5) in launches of 2 steps == five run(1) == run(2); run(3): a wrongly carried air pair
    (from launch to launch, from call to call) shows here"""
    kwargs = vc.descending((3, 257, 40), seed=21)
    rows = lambda parts: {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}  # noqa: E731
    ref = vc.run(engine, PR79, law, kwargs, "fused", 5, steps_per_launch=2)
    assert (ref[0]["steps_done"] == 5).all()
    for split in ((1,) * 5, (2, 3)):
        runner = vc.runner(engine, PR79, law, kwargs, "fused")
        parts = [runner.run(n) for n in split]
        pc.assert_same_bits(ref[0], runner.snapshot(), f"state, runs of {split}")
        pc.assert_same_bits(ref[1], rows(parts), f"profile, runs of {split}")


def test_snapshot_and_restore_carry_the_air_pair(engine):
    kwargs = vc.descending((5, 300), seed=22)
    ref = vc.run(engine, PR79, "RogersYau", kwargs, "fused", 4)
    runner = vc.runner(engine, PR79, "RogersYau", kwargs, "fused")
    runner.run(2)
    saved = runner.snapshot()
    runner.run(1)
    runner.restore(saved)
    pc.assert_same_bits(saved, runner.snapshot(), "restored")
    runner.run(2)
    pc.assert_same_bits(ref[0], runner.snapshot(), "state after restore")


# ---- 3. the timing of the air pair ------------------------------------------------------------------
@pytest.mark.parametrize("route", ("fused", "stages"))
def test_the_air_pair_is_the_one_of_moist_sync(engine, route):
    """after a step from a state with qv_prev != qv the carried density is that of Moist.sync -
    the advanced rhod with the qv of BEFORE the step's condensation - and not that of the state
    after the step"""
    kwargs = vc.descending((40, 7), seed=23)
    runner = vc.runner(engine, PR79, "GunnKinzer1949", kwargs, route)
    runner.run(1)
    before = runner.snapshot()
    assert (before["qv_prev"] != before["qv"]).all()
    runner.run(1)
    after = runner.snapshot()
    prhod = after["rhod"]  # (condensation leaves the advanced rhod as it is)
    of_sync = prhod * (1 + before["qv"])
    of_the_new_state = prhod * (1 + after["qv"])
    assert np.array_equal(pc.bits(after["air_density"]), pc.bits(of_sync))
    assert (after["air_density"] != of_the_new_state).all()
    # and the viscosity is that of T(prhod, thd before), which update_TpRH does not refresh
    assert (after["air_dynamic_viscosity"] != before["air_dynamic_viscosity"]).all()


def test_the_initial_air_pair_is_that_of_register(engine):
    kwargs = vc.descending((4, 9), seed=24)
    runner = vc.runner(engine, PR79, "GunnKinzer1949", kwargs, "fused")
    state = runner.snapshot()
    assert np.array_equal(pc.bits(state["air_density"]),
                          pc.bits(state["rhod"] * (1 + state["qv"])))
    k = runner.formulae.constants
    T = state["T"]
    eta = (k.ZOGRAFOS_1987_COEFF_T3 * T ** 3 + k.ZOGRAFOS_1987_COEFF_T2 * T ** 2
           + k.ZOGRAFOS_1987_COEFF_T1 * T + k.ZOGRAFOS_1987_COEFF_T0)
    np.testing.assert_allclose(state["air_dynamic_viscosity"], eta, rtol=1e-14)


# ---- 4. physics, qualitative ------------------------------------------------------------------------
def test_ventilation_speeds_up_the_evaporation_of_drizzle(engine):
    kwargs = vc.descending((60, 300), seed=25)
    start = vc.liquid_water({"water_mass": np.asarray(kwargs["water_mass"])}, kwargs)
    ventilated = vc.run(engine, PR79, "GunnKinzer1949", kwargs, "fused", 10)[0]
    neglect = vc.run(engine, "Neglect", None, kwargs, "fused", 10)[0]
    assert (ventilated["steps_done"] == 10).all() and (neglect["steps_done"] == 10).all()
    lost_ventilated = start - vc.liquid_water(ventilated, kwargs)
    lost_neglect = start - vc.liquid_water(neglect, kwargs)
    assert (lost_neglect > 0).all()
    assert (lost_ventilated > lost_neglect).all()


def test_ventilation_does_nothing_to_haze(engine):
    """all radii below 1 um: Re is about 0, the factor about 1 - the two runs agree to 1e-9
    relative in qv (a sanity condition on these inputs, not a parity claim)"""
    kwargs = vc.ascending((50, 257), seed=26)
    kwargs["water_mass"] = kwargs["water_mass"] * 0.6 ** 3  # (the ensemble's radii reach 1.6 um)
    radius =(np.asarray(kwargs["water_mass"]) / vc.RHO_W / (4 / 3 * np.pi)) ** (1 / 3)
    assert radius.max() < 1e-6
    ventilated = vc.run(engine, PR79, "GunnKinzer1949", kwargs, "fused", 3)
    neglect = vc.run(engine, "Neglect", None, kwargs, "fused", 3)
    assert ventilated[0]["reynolds_number"].max() < 1e-3
    np.testing.assert_allclose(ventilated[1]["qv"], neglect[1]["qv"], rtol=1e-9, atol=0)


# ---- 5. failure cases ---------------------------------------------------------------------------------
def test_a_radius_above_the_table_stops_its_parcel_only(engine):
    """a 7 mm row in the second of three parcels, at the second step (the first step's run leaves
    the row in place: it is set between the calls)"""
    kwargs = vc.descending((20, 300, 9), seed=27)
    states = []
    for route in ("fused", "stages"):
        runner = vc.runner(engine, PR79, "GunnKinzer1949", kwargs, route)
        runner.run(1)
        mass = runner.snapshot()["water_mass"]
        mass[20 + 260] = vc.RHO_W * 4 / 3 * np.pi * 7e-3 ** 3
        runner.restore({"water_mass": mass})
        before = runner.snapshot()
        with pytest.raises(ValueError, match=r"Radii can be interpolated up to 0\.006"):
            runner.run(2)
        after = runner.snapshot()
        states.append((after, runner.last_profile))
        assert after["out_of_table"].tolist() == [0, 1, 0]
        assert after["failed_step"].tolist() == [-1, 1, -1]
        assert after["steps_done"].tolist() == [3, 1, 3]
        rows = slice(20, 320)
        for key, value in after.items():  # every key of the stopped parcel as before the step
            if key == "n_steps":
                continue
            part = rows if value.size == 329 else slice(1, 2)
            if key not in ("failed_step", "out_of_table"):
                assert np.array_equal(pc.bits(value[part]), pc.bits(before[key][part])), key
        runner.run(1)  # the neighbours go on, the stopped parcel is skipped, nothing raises again
        assert runner.snapshot()["steps_done"].tolist() == [4, 1, 4]
    pc.assert_same_bits(states[0][0], states[1][0], "state, fused vs stages")
    pc.assert_same_bits(states[0][1], states[1][1], "profile, fused vs stages")


@pytest.mark.parametrize("kind,setup,sizes,seed", pc.FAILURE_CASES, ids=pc.FAILURE_IDS)
def test_a_failing_solver_leaves_the_air_pair_untouched(engine, kind, setup, sizes, seed):
    """the solvers of tests/parcel_cases.py that give up in some parcels (their formulae with the
    ventilation added): these stop with their state, the air pair included, as before the step;
    fused == stages"""
    kwargs = pc.ensemble(sizes, seed=seed, f_org=kind != "default")
    results = []
    for route in ("fused", "stages"):
        runner = vc.runner(engine, PR79, "RogersYau", kwargs, route, setup=setup, kind=kind)
        start = runner.snapshot()
        with pytest.raises(RuntimeError, match="Condensation failed"):
            runner.run(5)
        results.append((runner.snapshot(), runner.last_profile))
    pc.assert_same_bits(results[0][0], results[1][0], "state, fused vs stages")
    pc.assert_same_bits(results[0][1], results[1][1], "profile, fused vs stages")
    state = results[0][0]
    failed = state["failed_step"]
    assert (failed >= 0).any() and (failed == -1).any()
    at_once = failed == 0  # stopped in their first step: the pair of the initial state
    for key in ("air_density", "air_dynamic_viscosity"):
        assert np.array_equal(pc.bits(state[key][at_once]), pc.bits(start[key][at_once])), key
        assert (state[key][failed == -1] != start[key][failed == -1]).all(), key
    # a parcel stopped later carries the pair formed in its last good step: rhod is that step's
    # advanced rhod and qv_prev the qv of before its condensation
    later = failed > 0
    assert np.array_equal(pc.bits(state["air_density"][later]),
                          pc.bits((state["rhod"] * (1 + state["qv_prev"]))[later]))


# ---- 6. products ----------------------------------------------------------------------------------------
def test_products_equal_the_stage_routes_diagnose_after_each_step(engine):
    kwargs = vc.descending((1, 257, 1025), seed=28)
    formulae, _ = vc.formulae_of(PR79)
    table = ppc.full_table(formulae)
    fused = vc.runner(engine, PR79, "GunnKinzer1949", kwargs, "fused", steps_per_launch=2)
    profile, rows = ppc.run_with_table(fused, table, (3,))
    stages = vc.runner(engine, PR79, "GunnKinzer1949", kwargs, "stages")
    expected = ppc.diagnose_after_each_step(stages, table, 3)
    for key, value in expected.items():
        assert np.array_equal(pc.bits(rows[key]), pc.bits(value)), key
    assert np.isfinite(rows["dv"]).all() and profile["qv"].shape == (3, 3)
    pc.assert_same_bits(fused.snapshot(), stages.snapshot(), "state")
    # and the stage route with products= is the same again
    again = vc.runner(engine, PR79, "GunnKinzer1949", kwargs, "stages")
    _, rows_stages = ppc.run_with_table(again, table, (3,))
    pc.assert_same_bits(rows, rows_stages, "rows, fused vs stages")


# ---- 7. refusals ------------------------------------------------------------------------------------------
def _raw_call(engine, symbol_call, formulae, descriptor, vent_changes=None, n_sd=6):
    """one raw call on a tiny parcel; `symbol_call(args dict)` makes it"""
    setup = CondensationSetup()
    up = engine.upload
    state = {name: up(np.full(1, 1.0)) for name in abi.PARCEL_STATE_FLOATS}
    state.update({name: up(np.full(1, -1, dtype=np.int64)) for name in
                  ("n_substeps", "n_activating", "n_deactivating", "n_ripening", "failed_step")})
    state["RH_max"], state["steps_done"] = up(np.zeros(1)), up(np.zeros(1, dtype=np.int64))
    law = tv.make_law("GunnKinzer1949", engine)
    vent = {**vent_law(engine, law), "air_density": up(np.ones(1)),
            "air_dynamic_viscosity": up(np.ones(1)), "reynolds_number": up(np.zeros(n_sd)),
            "out_of_table": up(np.zeros(1, dtype=np.int64))}
    vent.update(vent_changes or {})
    return symbol_call(dict(
        engine=engine, formulae=formulae, cfg=parcel_cfg(formulae, setup, 1.0), n_steps=1,
        parcel_start=up(np.array([0, n_sd], dtype=np.int64)), water_mass=up(np.full(n_sd, 1e-12)),
        multiplicity=up(np.ones(n_sd, dtype=np.int64)), dry_volume=up(np.full(n_sd, 1e-21)),
        kappa=up(np.ones(n_sd)), f_org=up(np.zeros(n_sd)), critical_volume=up(np.zeros(n_sd)),
        state=state, w_mid=up(np.ones(1)), descriptor=descriptor), vent)


def test_the_library_refuses(engine):
    ventilated, _ = vc.formulae_of(PR79)
    froessling, froessling_descriptor = vc.formulae_of("Froessling1938")
    plain = Formulae()

    def old(args, _vent):
        parcel_call(args.pop("engine"), args.pop("formulae"), args.pop("cfg"), **args)

    def new(args, vent):
        parcel_call(args.pop("engine"), args.pop("formulae"), args.pop("cfg"), **args, vent=vent)

    # the old symbols go on refusing a ventilated descriptor (SDM_E_ARG = -1)
    for formulae, descriptor in ((ventilated, None), (froessling, froessling_descriptor)):
        with pytest.raises(RuntimeError, match="error -1"):
            _raw_call(engine, old, formulae, descriptor)
    # the new one refuses Neglect, a NULL air pair, the table law without its table
    with pytest.raises(RuntimeError, match="error -1"):
        _raw_call(engine, new, plain, None)
    for changes in ({"air_density": None}, {"air_dynamic_viscosity": None},
                    {"reynolds_number": None}, {"gk_a": None}, {"gk_b": None},
                    {"gk_table_len": 0}, {"velocity_law": 1}, {"velocity_law": 7},
                    {"velocity_law": 2, "velocity_terms": 3}):
        with pytest.raises(RuntimeError, match="error -1"):
            _raw_call(engine, new, ventilated, None, changes)
    # ... and a NULL `formulae` (the raw symbol: parcel_call always passes a descriptor)
    def without_formulae(args, vent):
        eng = args["engine"]
        c_state = abi.ParcelState()
        for name in abi.PARCEL_STATE_FIELDS:
            setattr(c_state, name, args["state"][name].ctypes.data)
        eng.call_parcel_vent(
            "sdm_parcel_run_vent", args["cfg"], 1, 1, 6, args["parcel_start"], args["water_mass"],
            args["multiplicity"], args["dry_volume"], args["kappa"], args["f_org"],
            args["critical_volume"], c_state, args["w_mid"], None,
            [float(getattr(plain.constants, name)) for name in CONSTANT_NAMES],
            None, None, None, _vent_struct(eng, vent, 1, 6))

    with pytest.raises(RuntimeError, match="error -1"):
        _raw_call(engine, without_formulae, ventilated, None)
    # a good call goes through (the arguments above are otherwise valid)
    too_short = {"gk_a": engine.upload(np.zeros(5))}
    with pytest.raises(ValueError, match="gk_a"):
        _raw_call(engine, new, ventilated, None, too_short)


def test_the_runner_refuses(engine):
    kwargs = pc.saturated(pc.ensemble((5, 9), seed=3), Formulae())
    setup = CondensationSetup()
    ventilated, _ = vc.formulae_of(PR79)
    for route in ("fused", "stages"):
        with pytest.raises(NotImplementedError, match="ventilation"):
            ParcelRunner(engine, ventilated, setup, route=route, **kwargs)
        with pytest.raises(NotImplementedError, match="ventilation"):
            ParcelRunner(engine, ventilated, setup, route=route, terminal_velocity="RogersYau",
                         chemistry=object(), **kwargs)
    with pytest.raises(ValueError, match="terminal_velocity"):
        ParcelRunner(engine, ventilated, setup, terminal_velocity="Stokes", **kwargs)
    # without a ventilation the argument is accepted and not read
    plain = ParcelRunner(engine, Formulae(), setup, terminal_velocity="RogersYau", **kwargs)
    assert not plain.ventilated and "air_density" not in plain.snapshot()


def test_the_recorded_resource_table_shows_the_old_kernels_unchanged():
    """profiles/parcel_vent_kernel_resources.tsv (the compiler's remarks, recorded): the six
    kernels that existed have the parent's VGPRs, AGPRs, LDS and scratch; the new ones are there"""
    rows = {}
    with open(os.path.join(ROOT, "profiles", "parcel_vent_kernel_resources.tsv"),
              encoding="utf-8") as handle:
        lines = [line.rstrip("\n").split("\t") for line in handle if not line.startswith("#")]
    header = lines[0]
    for line in lines[1:]:
        rows[line[0], line[1]] = dict(zip(header[2:], line[2:]))
    for kernel in ("k_condensation", "k_condensation_f", "k_parcel", "k_parcel_f", "k_parcel_d",
                   "k_parcel_f_d"):
        for column in ("vgprs", "agprs", "lds_bytes", "scratch_bytes_per_lane", "vgpr_spill"):
            assert rows["parent", kernel][column] == rows["change", kernel][column], (kernel,
                                                                                     column)
    assert ("change", "k_parcel_v") in rows and ("change", "k_parcel_v_d") in rows
    assert ("parent", "k_parcel_v") not in rows


# ---- 8. the PySDM hook ------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "PySDM")),
                    reason="reference tree not present")
def test_run_parcel_leaves_a_ventilated_particulator_as_run_would(engine):  # pylint: disable=unused-argument,too-many-locals
    """twins with PruppacherAndRasmussen1979: `particulator.run` against `run_parcel`, to the bit,
    then one further step of either kind on both (a wrongly left air pair shows there)"""
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
    from tests.parcel_vent_checker import ParcelVentCheckerBackend  # pylint: disable=import-outside-toplevel

    n_sd = 40
    rng = np.random.default_rng(5)
    r_wet = np.exp(rng.uniform(np.log(50e-6), np.log(400e-6), n_sd))
    dry_volume = np.full(n_sd, 4 / 3 * np.pi * 1e-7 ** 3)

    def twin():
        backend = as_pysdm_backend(ParcelVentCheckerBackend)(PySDMFormulae(ventilation=PR79))
        env = Parcel(dt=1.0, mass_of_dry_air=1.0, p0=90000.0,
                     initial_water_vapour_mixing_ratio=5e-3, T0=285.0, w=-1.0)
        builder = Builder(n_sd=n_sd, backend=backend, environment=env)
        builder.add_dynamic(AmbientThermodynamics())
        builder.add_dynamic(Condensation(adaptive=True))
        attributes = {"multiplicity": np.full(n_sd, 50, dtype=np.int64),
                      "dry volume": dry_volume, "kappa times dry volume": 0.5 * dry_volume,
                      "volume": 4 / 3 * np.pi * r_wet ** 3}
        return builder.build(attributes=attributes, products=())

    def state_of(particulator):
        env, cond = particulator.environment, particulator.dynamics["Condensation"]
        out = {"n_steps": np.asarray(particulator.n_steps), "dv": np.asarray(env.mesh.dv),
               "success": cond.success.to_ndarray(), "rh_max": cond.rh_max.to_ndarray(),
               "signed water mass": particulator.attributes["signed water mass"].to_ndarray(
                   raw=True)}
        for var in env.variables:  # ("air density" and "air dynamic viscosity" among them)
            out["current/" + var] = env[var].to_ndarray()
        for name, counter in cond.counters.items():
            out[name] = counter.to_ndarray()
        return out

    def same(a, b, what):
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(pc.bits(np.asarray(a[key])), pc.bits(np.asarray(b[key]))), (
                what, key, a[key], b[key])

    stepped, fused = twin(), twin()
    assert "air density" in stepped.environment.variables
    stepped.run(4)
    run_parcel(fused, 4)
    same(state_of(stepped), state_of(fused), "after 4 steps")
    stepped.run(1)
    fused.run(1)
    same(state_of(stepped), state_of(fused), "after one further particulator.run(1)")
    run_parcel(fused, 1)
    stepped.run(1)
    same(state_of(stepped), state_of(fused), "after one further run_parcel(1)")

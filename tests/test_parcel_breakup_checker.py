"""The parcel with collisional breakup (include/sdm_parcel_breakup.h) without a GPU: the binding,
the CPU checker (tests/parcel_breakup_checker/) on its fused call against the stage route
(`sdm_collision_step` with breakup, parcel after parcel) bit for bit for every fragmentation
function and coalescence efficiency, continuation, independence, the grid cap, a failed parcel,
overflows, conservation, `enable_breakup = 0` through the new symbol and the refusals.
tests/test_hip_parcel_breakup.py repeats the `check_*` functions on the HIP engine."""
import ctypes
import os
import subprocess
import tempfile
import warnings

import numpy as np
import pytest

from pysdm_amd import abi, recipe
from pysdm_amd.condensation import CondensationSetup
from pysdm_amd.formulae import Formulae
from pysdm_amd.parcel import ParcelRunner
from tests import parcel_breakup_cases as bc
from tests import parcel_cases as pc
from tests import parcel_coal_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def engine():
    from tests.parcel_breakup_checker import ParcelBreakupCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelBreakupCheckerEngine.get()


# ---- 0. binding --------------------------------------------------------------------------------------
def test_header_parses_and_the_symbol_binds(engine):
    table = abi.parse_header(abi.PARCEL_BREAKUP_HEADER_PATH)
    assert list(table) == ["sdm_parcel_run_collision"]
    names = [p.name for p in table["sdm_parcel_run_collision"][1]]
    coal = [p.name for p in abi.parse_header(abi.PARCEL_COAL_HEADER_PATH)["sdm_parcel_run_coal"][1]]
    assert names == coal + ["breakup", "breakup_profile"]  # the arguments of ..._coal plus two
    assert hasattr(engine.parcel_breakup_library.cdll, "sdm_parcel_run_collision")
    assert hasattr(abi.parcel_breakup_library().cdll, "sdm_parcel_run_collision")  # the product


def test_struct_layouts_match_the_header():
    prints = []
    for struct, mirror in (("sdm_parcel_breakup_state", abi.ParcelBreakupState),
                           ("sdm_parcel_breakup_profile", abi.ParcelBreakupProfile)):
        prints.append(f'printf("%zu\\n", sizeof({struct}));')
        prints += [f'printf("%zu\\n", offsetof({struct}, {field}));'
                   for field, _ in mirror._fields_]  # pylint: disable=protected-access
    source = ('#include "include/sdm_parcel_breakup.h"\n#include <stddef.h>\n#include <stdio.h>\n'
              "int main(){" + "".join(prints) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w", encoding="utf-8") as handle:
            handle.write(source)
        subprocess.check_call(["gcc", "-I", ROOT, src, "-o", exe], cwd=ROOT)
        numbers = [int(x) for x in subprocess.check_output([exe]).split()]
    expected = []
    for mirror in (abi.ParcelBreakupState, abi.ParcelBreakupProfile):
        expected += [ctypes.sizeof(mirror)] + [
            getattr(mirror, field).offset for field, _ in mirror._fields_]  # pylint: disable=protected-access
    assert numbers == expected


# ---- 1. fused == stage route -------------------------------------------------------------------------
SEEDS = np.arange(len(bc.SIZES)) + 11


def check_fused_equals_stages(engine, setup, steps=3, sizes=bc.SIZES, seeds=SEEDS):
    """state, every column, idx up to n_live, counters (the breakup pair included), both stream
    positions, the profiles: bit for bit; breakups occurred and the breakup stream moved"""
    kwargs = bc.ensemble(sizes, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # ("overflow", "dt_min": checked where they are the subject)
        fused = bc.run(engine, kwargs, "fused", steps, setup, seed=seeds)
        stages = bc.run(engine, kwargs, "stages", steps, setup, seed=seeds)
    bc.assert_same_run(fused, stages, "fused vs stages")
    state, record = fused[0], fused[2]
    assert (state["steps_done"] == steps).all()
    assert state["breakup_rate"].sum() > 0
    assert np.array_equal(record["breakup_rate"].sum(axis=0), state["breakup_rate"])
    assert np.array_equal(record["breakup_rate_deficit"].sum(axis=0),
                          state["breakup_rate_deficit"])
    # P draws per sub-step from the proc / frag stream, N + P from the collision stream
    counts = np.asarray(sizes)
    sub_steps = record["n_substeps"].sum(axis=0)
    assert np.array_equal(state["rng_offset_breakup"], sub_steps * (counts // 2))
    assert np.array_equal(state["rng_offset"], sub_steps * (counts + counts // 2))
    starts = np.concatenate(([0], np.cumsum(sizes)))
    for c, size in enumerate(sizes):  # a permutation of live rows of the parcel itself
        live = state["idx"][starts[c]:starts[c] + state["n_live"][c]]
        assert len(set(live.tolist())) == live.size
        assert ((live >= starts[c]) & (live < starts[c] + size)).all()
        assert (state["multiplicity"][live] > 0).all()
    return fused


# (Low & List's fragments of cloud droplets leave drops the condensation solver gives up on in
# the third step: two steps)
@pytest.mark.parametrize("frag", list(bc.FRAGMENTATIONS))
def test_fused_equals_the_stage_route_for_every_fragmentation(engine, frag):
    """CollisionSetup.breakup_only; Straub and Low-List with the Geometric kernel (derive_ru), the
    others with ConstantK; adaptive and substeps = 3 alternate"""
    adaptive = list(bc.FRAGMENTATIONS).index(frag) % 2 == 0
    fused = check_fused_equals_stages(
        engine, bc.breakup_setup(frag, adaptive=adaptive, substeps=3),
        steps=2 if frag == "lowlist1982" else 3)
    assert fused[0]["coalescence_rate"].sum() == 0
    if not adaptive:
        assert (fused[2]["n_substeps"][:, 1:] == 3).all()


@pytest.mark.parametrize("ec", list(bc.EFFICIENCIES))
def test_fused_equals_the_stage_route_for_every_efficiency(engine, ec):
    """CollisionSetup.collision with Eb = 0.5: coalescences, breakups and bounces all occur"""
    fused = check_fused_equals_stages(engine, bc.collision_setup(ec=ec))
    state = fused[0]
    assert state["coalescence_rate"].sum() > 0
    assert bc.bounces(state).sum() > 0  # collisions counted in neither rate
    assert (bc.bounces(state) >= 0).all()


@pytest.mark.parametrize("adaptive", (True, False), ids=("adaptive", "substeps3"))
@pytest.mark.parametrize("handle_all", (False, True), ids=("first_breakup", "all_breakups"))
def test_fused_equals_the_stage_route_with_and_without_handle_all_breakups(engine, handle_all,
                                                                          adaptive):
    fused = check_fused_equals_stages(
        engine, bc.collision_setup(adaptive=adaptive, substeps=3, handle_all_breakups=handle_all))
    assert fused[0]["coalescence_rate"].sum() > 0
    if not handle_all:  # breakups that the donor's multiplicity refused
        assert fused[0]["breakup_rate_deficit"].sum() > 0


def check_the_largest_parcel(engine):
    """SDM_PARCEL_COAL_MAX_ROWS rows: four pairs per lane, a list that can hold every pair"""
    fused = check_fused_equals_stages(engine, bc.collision_setup(), steps=2, sizes=bc.CAP_SIZES,
                                      seeds=(5, 6))
    assert fused[0]["breakup_rate"][0] > 0 and fused[0]["coalescence_rate"][0] > 0
    for route in ("fused", "stages"):
        with pytest.raises(ValueError, match="SDM_PARCEL_COAL_MAX_ROWS"):
            bc.runner(engine, bc.ensemble((cc.MAX_ROWS + 1,)), route, bc.collision_setup())


def test_the_largest_parcel_and_one_row_more(engine):
    check_the_largest_parcel(engine)


# ---- 3. shared edge cases ----------------------------------------------------------------------------
def check_continuation(engine):
    kwargs = bc.ensemble((3, 65, 300), seed=13)
    more = dict(seed=(5, 6, 7))
    setup = bc.collision_setup
    whole = bc.run(engine, kwargs, "fused", 9, setup(), **more)
    assert whole[0]["breakup_rate"].sum() > 0 and (whole[0]["rng_offset_breakup"] > 0).all()
    runner = bc.runner(engine, kwargs, "fused", setup(), **more)
    parts = [runner.run(n) for n in (4, 5)]
    pc.assert_same_bits(whole[0], runner.snapshot(), "state")  # (stream positions included)
    pc.assert_same_bits(whole[1], cc.concatenated([p[0] for p in parts]), "profile")
    pc.assert_same_bits(whole[2], cc.concatenated([p[1] for p in parts]), "collision profile")


def test_continuation(engine):
    """run(9) == run(4); run(5)"""
    check_continuation(engine)


def test_snapshot_and_restore_carry_the_breakup_arrays(engine):
    kwargs = bc.ensemble((3, 65, 300), seed=13)
    runner = bc.runner(engine, kwargs, "fused", bc.collision_setup(), seed=(5, 6, 7))
    runner.run(2)
    kept = runner.snapshot()
    assert {"breakup_rate", "breakup_rate_deficit", "rng_offset_breakup"} <= set(kept)
    runner.run(2)
    after = runner.snapshot()
    assert not np.array_equal(after["rng_offset_breakup"], kept["rng_offset_breakup"])
    assert not np.array_equal(after["breakup_rate"], kept["breakup_rate"])
    runner.restore(kept)
    pc.assert_same_bits(runner.snapshot(), kept, "restored")
    runner.run(2)
    pc.assert_same_bits(runner.snapshot(), after, "run again from the snapshot")


PER_PARCEL = cc.COUNTERS + ("breakup_rate", "breakup_rate_deficit", "n_live", "stats_n_substep",
                            "stats_dt_min", "events", "rng_offset", "rng_offset_breakup")


def check_independence(engine):
    sizes = (3, 64, 257)
    kwargs = bc.ensemble(sizes, seed=21)
    seeds = np.array([3, 4, 5])
    whole = bc.runner(engine, kwargs, "fused", bc.collision_setup(), seed=seeds)
    whole.run(3)
    state = whole.snapshot()
    assert state["breakup_rate"].sum() > 0
    starts = whole.parcel_start_host
    formulae = cc.formulae_of("default")
    for c, size in enumerate(sizes):
        alone = bc.runner(engine, cc.solo(kwargs, formulae, starts, c), "fused",
                          bc.collision_setup(), seed=int(seeds[c]))
        alone.run(3)
        rows = slice(int(starts[c]), int(starts[c + 1]))
        for key, value in alone.snapshot().items():
            if key == "n_steps":
                continue
            where = rows if value.size == size and key not in pc.STATE_KEYS[:15] and (
                key not in PER_PARCEL) else slice(c, c + 1)
            mine = state[key][where]
            if key == "idx":
                mine = np.where(mine >= 0, mine - starts[c], -1)
            assert np.array_equal(pc.bits(mine), pc.bits(value)), (c, key)


def test_a_parcel_of_an_ensemble_equals_its_solo_run(engine):
    check_independence(engine)


def check_more_parcels_than_the_grid_cap(engine):
    """cap + 1 parcels of 3 rows: the workgroups stride; the last parcel equals its solo run"""
    n_parcel = cc.GRID_CAP + 1
    kwargs = bc.ensemble((3,) * n_parcel, seed=6)
    seeds = np.arange(n_parcel) + 100
    # (one pair per parcel: a kernel under which most of them collide within two steps)
    setup = lambda: bc.collision_setup(kernel=recipe.ConstantK(a=4e-3))  # noqa: E731
    runner = bc.runner(engine, kwargs, "fused", setup(), seed=seeds)
    runner.run(2)
    state = runner.snapshot()
    assert (state["steps_done"] == 2).all() and (state["rng_offset_breakup"] > 0).all()
    assert state["breakup_rate"].sum() > 0 and state["coalescence_rate"].sum() > 0
    assert state["breakup_rate"][cc.GRID_CAP - 1:].sum() + state["collision_rate"][
        cc.GRID_CAP - 1:].sum() > 0
    formulae = cc.formulae_of("default")
    for c in (0, cc.GRID_CAP - 1, cc.GRID_CAP):
        alone = bc.runner(engine, cc.solo(kwargs, formulae, runner.parcel_start_host, c), "fused",
                          setup(), seed=int(seeds[c]))
        alone.run(2)
        solo = alone.snapshot()
        rows = slice(3 * c, 3 * c + 3)
        for key in ("water_mass", "multiplicity", "dry_volume", "kappa"):
            assert np.array_equal(pc.bits(state[key][rows]), pc.bits(solo[key])), (c, key)
        for key in ("thd", "qv", "n_live", "rng_offset", "rng_offset_breakup", "breakup_rate",
                    "collision_rate"):
            assert np.array_equal(pc.bits(state[key][c:c + 1]), pc.bits(solo[key])), (c, key)


def test_more_parcels_than_the_grid_cap(engine):
    check_more_parcels_than_the_grid_cap(engine)


def check_a_failed_parcel(engine, case=0):
    """a failure case of tests/test_parcel_checker.py (a solver that gives up): the failed parcel
    keeps its rows, permutation, counters - the breakup arrays included - and stream positions,
    the others go on; both routes agree"""
    kind, setup, sizes, seed = pc.FAILURE_CASES[case]
    kwargs = pc.ensemble(sizes, seed=seed)
    kwargs["multiplicity"] = np.where(np.arange(kwargs["multiplicity"].size) % 4 == 0, 1,
                                      kwargs["multiplicity"])
    collisions = lambda: recipe.CollisionSetup.breakup_only(  # noqa: E731
        recipe.ConstantK(a=1e-9), recipe.AlwaysN(2), dt_range=bc.DT_RANGE)
    runners = {}
    for route in ("fused", "stages"):
        runners[route] = bc.runner(engine, kwargs, route, collisions(), kind=kind, setup=setup)
        with pytest.raises(RuntimeError, match="Condensation failed"):
            runners[route].run(5)
    state = runners["fused"].snapshot()
    pc.assert_same_bits(state, runners["stages"].snapshot(), "fused vs stages")
    pc.assert_same_bits(runners["fused"].last_coal_profile, runners["stages"].last_coal_profile,
                        "collision profile, fused vs stages")
    failed = state["failed_step"]
    assert (failed >= 0).any() and (failed == -1).any()
    went_on = failed == -1
    assert (state["rng_offset_breakup"][went_on] > 0).all()
    try:
        runners["fused"].run(2)
    except RuntimeError as error:
        assert failed[error.args[1]] == -1
    again = runners["fused"].snapshot()
    starts = runners["fused"].parcel_start_host
    for c in np.flatnonzero(failed >= 0):
        rows = slice(int(starts[c]), int(starts[c + 1]))
        for key in ("water_mass", "multiplicity", "dry_volume", "kappa", "idx",
                    "kappa_times_dry_volume"):
            assert np.array_equal(pc.bits(again[key][rows]), pc.bits(state[key][rows])), (c, key)
        for key in PER_PARCEL + ("thd", "qv"):
            assert np.array_equal(pc.bits(again[key][c:c + 1]), pc.bits(state[key][c:c + 1])), key
    still = again["failed_step"] == -1
    assert still.any()
    assert (again["rng_offset_breakup"][still] > state["rng_offset_breakup"][still]).all()


def test_a_failed_parcel_keeps_everything_the_breakup_arrays_included(engine):
    check_a_failed_parcel(engine)


# ---- 4. overflow -------------------------------------------------------------------------------------
def check_overflow(engine):
    """a small max_multiplicity: breakups are refused, counted in the step's n_overflow and in
    events, and warned about after the call; fused equals stages"""
    kwargs = bc.ensemble((3, 65, 256), seed=3)
    setup = lambda **more: bc.breakup_setup("always_n", max_multiplicity=1500, **more)  # noqa: E731
    results = {}
    for route in ("fused", "stages"):
        runner = bc.runner(engine, kwargs, route, setup(), seed=(5, 6, 7))
        with pytest.warns(UserWarning, match="overflow"):
            out = runner.run(2)
        results[route] = (runner.snapshot(), *out)
    bc.assert_same_run(results["fused"], results["stages"], "overflow: fused vs stages")
    record = results["fused"][2]
    assert record["n_overflow"].sum() > 0 and (record["n_overflow"] >= 0).all()
    assert (results["fused"][0]["events"] == 0).all()  # (cleared with the warning)
    # events carries the count: the same call without the clearing warning's owner
    quiet = bc.runner(engine, kwargs, "fused", setup(warn_overflows=False), seed=(5, 6, 7))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _, quiet_record = quiet.run(2)
    pc.assert_same_bits(quiet_record, record, "the record does not depend on warn_overflows")


def check_events_carry_the_overflow_count(engine):
    """the raw call (parcel_call keeps events as the library leaves them)"""
    kwargs = bc.ensemble((3, 65, 256), seed=3)
    runner = bc.runner(engine, kwargs, "fused",
                       bc.breakup_setup("always_n", max_multiplicity=1500), seed=(5, 6, 7))
    runner._coal_warnings = lambda: None  # pylint: disable=protected-access
    _, record = runner.run(2)
    events = runner.snapshot()["events"]
    assert np.array_equal(events >> abi.PARCEL_COAL_OVERFLOW_SHIFT, record["n_overflow"].sum(axis=0))
    assert (events >> abi.PARCEL_COAL_OVERFLOW_SHIFT).sum() > 0


def test_overflows_are_counted_recorded_and_warned_about(engine):
    check_overflow(engine)
    check_events_carry_the_overflow_count(engine)


# ---- 5. conservation -------------------------------------------------------------------------------
def check_conservation(engine):
    """the sums of multiplicity x {water mass, dry volume, kappa times dry volume} over the live
    rows across every COLLISION step.  Its input is what a twin with a kernel of zero holds after
    the same step from the same state: the same condensation over the same rows in the same order,
    and no collision.  The tolerance is the deviation the stage route itself shows on the same
    input; the number of live rows never grows"""
    kwargs = bc.ensemble((3, 65, 257), seed=3)
    seeds = (5, 6, 7)
    runners = {route: bc.runner(engine, kwargs, route, bc.collision_setup(), seed=seeds)
               for route in ("fused", "stages")}
    calm = bc.runner(engine, kwargs, "fused",
                     bc.collision_setup(kernel=recipe.ConstantK(a=0.0)), seed=seeds)
    for step in range(3):
        start = runners["fused"].snapshot()
        calm.restore(start)
        calm.run(1)
        assert calm.snapshot()["collision_rate"].sum() == start["collision_rate"].sum()
        entering = bc.extensive_sums(calm)
        leaving = {}
        for route, runner in runners.items():
            runner.run(1)
            leaving[route] = bc.extensive_sums(runner)
        for c in range(3):
            assert leaving["fused"][c][3] <= entering[c][3], (step, c)  # live rows
            for a in range(3):
                tolerance = abs(leaving["stages"][c][a] - entering[c][a])
                assert abs(leaving["fused"][c][a] - entering[c][a]) <= tolerance, (step, c, a)
                # (and the stage route's own deviation is rounding, not a leak)
                assert tolerance <= 1e-9 * abs(entering[c][a]), (step, c, a, tolerance)
    state = runners["fused"].snapshot()
    assert state["breakup_rate"].sum() > 0 and state["coalescence_rate"].sum() > 0


def test_the_extensive_sums_are_conserved_by_every_collision_step(engine):
    check_conservation(engine)


# ---- 6. enable_breakup = 0 through the new symbol ------------------------------------------------------
def check_coalescence_through_the_new_symbol(engine):
    """breakup=True with a set-up of coalescence: sdm_parcel_run_collision with enable_breakup = 0
    gives sdm_parcel_run_coal's results to the bit and leaves the (poisoned) breakup arrays alone"""
    kwargs = cc.ensemble(seed=3)
    more = dict(collisions=cc.setup_of("geometric"), seed=np.arange(len(cc.SIZES)) + 11)
    old = cc.run(engine, "default", kwargs, "fused", 4, **more)
    runner = cc.runner(engine, "default", kwargs, "fused", breakup=True, **more)
    assert runner.coal_cfg.enable_breakup == 0
    poison = {"breakup_rate": np.full(len(cc.SIZES), -77), "rng_offset_breakup":
              np.full(len(cc.SIZES), 123456789), "breakup_rate_deficit": np.full(len(cc.SIZES), -5)}
    runner.restore(poison)
    new = (*runner.run(4),)
    state = runner.snapshot()
    for key, value in poison.items():
        assert np.array_equal(state.pop(key), value), key
    cc.assert_same_run((state, *new), old, "the new symbol without breakup vs sdm_parcel_run_coal")
    assert old[0]["coalescence_rate"].sum() > 0
    stages = cc.runner(engine, "default", kwargs, "stages", breakup=True, **more)
    out = stages.run(4)
    state = stages.snapshot()
    for key in poison:
        state.pop(key)
    cc.assert_same_run((state, *out), old, "the stage route with the keyword")


def test_coalescence_through_the_new_symbol_equals_the_old_one(engine):
    check_coalescence_through_the_new_symbol(engine)


# ---- 7. refusals -------------------------------------------------------------------------------------
def check_refusals(engine):
    kwargs = pc.saturated(bc.ensemble((5, 9), seed=3), Formulae())

    def fresh(setup=None, **more):
        return ParcelRunner(engine, Formulae(), CondensationSetup(), breakup=True,
                            collisions=setup or bc.collision_setup(), **more, **kwargs)

    # without the keyword a breakup set-up is refused as it always was, on either route
    for route in ("fused", "stages"):
        for setup in (bc.collision_setup(), bc.breakup_setup()):
            with pytest.raises(NotImplementedError, match="breakup"):
                ParcelRunner(engine, Formulae(), CondensationSetup(), route=route,
                             collisions=setup, **kwargs)
        # ... and with it what stays out of scope still is
        for name, options in (("optimized_random", dict(optimized_random=True)),
                              ("global croupier", dict(croupier="global"))):
            with pytest.raises(NotImplementedError, match=name):
                fresh(bc.collision_setup(**options), route=route)
    with pytest.raises(ValueError, match="max_multiplicity"):
        fresh(bc.collision_setup(max_multiplicity=0))
    with pytest.raises(ValueError, match="collisions"):
        ParcelRunner(engine, Formulae(), CondensationSetup(), breakup=True, **kwargs)
    # the library, by name, with nothing launched: the state is what it was
    library = {"ec": ("ec", 9), "frag": ("frag", 99), "max_multiplicity": ("max_multiplicity", 0),
               "optimized_random": ("optimized_random", 1), "croupier": ("croupier_local", 0),
               "velocity_source": ("velocity_source", 1), "kernel": ("kernel", 77)}
    for name, (field, value) in library.items():
        runner = fresh()
        before = runner.snapshot()
        setattr(runner.coal_cfg, field, value)
        with pytest.raises(RuntimeError, match=name):
            runner.run(1)
        pc.assert_same_bits(runner.snapshot(), before, f"refused: {name}")
    # a breakup set-up that needs a fall velocity without its table
    runner = fresh(bc.breakup_setup("straub2010", kernel=recipe.ConstantK(a=1e-3)))
    runner._coal_law = None  # pylint: disable=protected-access
    with pytest.raises(RuntimeError, match="gk_a"):
        runner.run(1)
    # a missing breakup column
    for name in ("breakup_rate", "breakup_rate_deficit"):
        runner = fresh()
        runner.breakup_counters[name] = None
        with pytest.raises(RuntimeError, match="breakup"):
            runner.run(1)
    runner = fresh()
    runner.restore({"n_live": np.array([6, 9])})
    with pytest.raises(RuntimeError, match="n_live"):
        runner.run(1)
    # sdm_parcel_run_coal goes on refusing enable_breakup
    runner = ParcelRunner(engine, Formulae(), CondensationSetup(), collisions=cc.setup_of(),
                          **kwargs)
    runner.coal_cfg.enable_breakup = 1
    with pytest.raises(RuntimeError, match="enable_breakup"):
        runner.run(1)
    # an engine without the library says so, and has the stage route
    from tests.parcel_coal_checker import ParcelCoalCheckerEngine  # pylint: disable=import-outside-toplevel

    if engine.name == "parcel_breakup_checker":
        with pytest.raises(NotImplementedError, match="parcel with breakup.*route='fused'"):
            ParcelRunner(ParcelCoalCheckerEngine.get(), Formulae(), CondensationSetup(),
                         breakup=True, collisions=bc.collision_setup(), **kwargs)
        ParcelRunner(ParcelCoalCheckerEngine.get(), Formulae(), CondensationSetup(),
                     route="stages", breakup=True, collisions=bc.collision_setup(),
                     **kwargs).run(1)


def test_refusals_by_name(engine):
    check_refusals(engine)

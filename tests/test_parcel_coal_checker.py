"""The parcel with coalescence (include/sdm_parcel_coal.h) without a GPU: the binding, the CPU
checker (tests/parcel_coal_checker/) on its fused call against the stage route over the existing
checkers' symbols bit for bit, the order the sums follow, continuation, independence and seeds,
the edges, conservation and the refusals."""
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
from tests import parcel_cases as pc
from tests import parcel_coal_cases as cc
from tests import parcel_vent_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def engine():
    from tests.parcel_coal_checker import ParcelCoalCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelCoalCheckerEngine.get()


# ---- 0. binding --------------------------------------------------------------------------------------
def test_header_parses_and_the_symbol_binds(engine):
    table = abi.parse_header(abi.PARCEL_COAL_HEADER_PATH)
    assert list(table) == ["sdm_parcel_run_coal"]
    params = {p.name: p for p in table["sdm_parcel_run_coal"][1]}
    assert params["coal_cfg"].kind == "pointer" and params["coal"].kind == "pointer"
    assert params["consts"].kind == "host_array" and params["consts"].array_len == 34
    assert params["fresh_idx"].kind == "scalar"
    assert hasattr(engine.parcel_coal_library.cdll, "sdm_parcel_run_coal")
    assert hasattr(abi.parcel_coal_library().cdll, "sdm_parcel_run_coal")  # the product library


def test_struct_layouts_and_constants_match_the_header():
    prints = []
    for struct, mirror in (("sdm_parcel_coal_state", abi.ParcelCoalState),
                           ("sdm_parcel_coal_profile", abi.ParcelCoalProfile)):
        prints.append(f'printf("%zu\\n", sizeof({struct}));')
        prints += [f'printf("%zu\\n", offsetof({struct}, {field}));'
                   for field, _ in mirror._fields_]  # pylint: disable=protected-access
    prints += [f'printf("%lld\\n", (long long){name});' for name in (
        "SDM_PARCEL_COAL_MAX_ROWS", "SDM_PARCEL_COAL_MAX_GRID", "SDM_PARCEL_COAL_EVENT_BOUND",
        "SDM_PARCEL_COAL_EVENT_DT_MIN", "SDM_PARCEL_COAL_OVERFLOW_SHIFT")]
    source = ('#include "include/sdm_parcel_coal.h"\n#include <stddef.h>\n#include <stdio.h>\n'
              "int main(){" + "".join(prints) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w", encoding="utf-8") as handle:
            handle.write(source)
        subprocess.check_call(["gcc", "-I", ROOT, src, "-o", exe], cwd=ROOT)
        numbers = [int(x) for x in subprocess.check_output([exe]).split()]
    expected = []
    for mirror in (abi.ParcelCoalState, abi.ParcelCoalProfile):
        expected += [ctypes.sizeof(mirror)] + [
            getattr(mirror, field).offset for field, _ in mirror._fields_]  # pylint: disable=protected-access
    expected += [abi.PARCEL_COAL_MAX_ROWS, abi.PARCEL_COAL_MAX_GRID, abi.PARCEL_COAL_EVENT_BOUND,
                 abi.PARCEL_COAL_EVENT_DT_MIN, abi.PARCEL_COAL_OVERFLOW_SHIFT]
    assert numbers == expected
    assert abi.PARCEL_COAL_MAX_ROWS >= 2048 and cc.MAX_ROWS == abi.PARCEL_COAL_MAX_ROWS
    assert cc.GRID_CAP == abi.PARCEL_COAL_MAX_GRID


# ---- 1. fused == stage route -------------------------------------------------------------------------
def check_fused_equals_stages(engine, kernel, adaptive, kind="default", law=None, steps=5):
    """the check of section 1 on any engine (tests/test_hip_parcel_coal.py repeats it)"""
    kwargs = cc.ensemble(seed=3, multiplicity=int(1e9) if kernel == "electric" else 1000)
    more = dict(collisions=cc.setup_of(kernel, adaptive=adaptive, substeps=3),
                seed=np.arange(len(cc.SIZES)) + 11)
    if law is not None:
        more["terminal_velocity"] = law
    fused = cc.run(engine, kind, kwargs, "fused", steps, **more)
    stages = cc.run(engine, kind, kwargs, "stages", steps, **more)
    cc.assert_same_run(fused, stages, f"{kernel}: fused vs stages")
    state = fused[0]
    assert (state["steps_done"] == steps).all()
    assert state["coalescence_rate"].sum() > 0
    if kernel != "electric":  # (whose constants are the reference's: nobody has to die)
        assert (state["n_live"] < np.asarray(cc.SIZES)).sum() >= 2
    starts = np.concatenate(([0], np.cumsum(cc.SIZES)))
    identity = np.where(state["idx"] >= 0, np.arange(state["idx"].size), -1)
    assert not np.array_equal(state["idx"], identity)  # the order was shuffled, and is followed
    for c, size in enumerate(cc.SIZES):  # a permutation of live rows of the parcel itself
        live = state["idx"][starts[c]:starts[c] + state["n_live"][c]]
        assert len(set(live.tolist())) == live.size
        assert ((live >= starts[c]) & (live < starts[c] + size)).all()
        assert (state["multiplicity"][live] > 0).all()
    assert state["rng_offset"][0] == 0 and (state["rng_offset"][1:] > 0).all()
    assert (fused[2]["n_live"][-1] == state["n_live"]).all()
    return fused


@pytest.mark.parametrize("adaptive", (True, False), ids=("adaptive", "substeps3"))
@pytest.mark.parametrize("kernel", ("constant", "golovin", "geometric"))
def test_fused_equals_the_stage_route(engine, kernel, adaptive):
    """parcels of (1, 2, 3, 63, 64, 65, 257, 600) rows with planted multiplicities of 1 and 2, 5
    steps: state, every column, idx up to n_live, n_live, counters, stream positions, both
    profiles; collisions and deaths occur and the order changes"""
    fused = check_fused_equals_stages(engine, kernel, adaptive)
    if adaptive:
        assert fused[2]["n_substeps"].max() > 1  # an adaptive case of more than one sub-step
    else:
        assert (fused[2]["n_substeps"][:, 1:] == 3).all()


def test_fused_equals_the_stage_route_with_the_electric_kernel(engine):
    check_fused_equals_stages(engine, "electric", True, steps=2)


def test_fused_equals_the_stage_route_with_other_formulae(engine):
    """the general condensation kernel's formulae (cc.GENERAL_OPTIONS)"""
    check_fused_equals_stages(engine, "constant", True, kind="general", steps=4)


def test_the_closed_form_velocity_laws_are_refused_where_the_engine_lacks_them(engine):
    """the CPU oracle's collision step evaluates the Gunn-Kinzer table only: on it the other two
    laws are refused by name (the GPU tests run them)"""
    assert engine.fused_velocity_laws == ("GunnKinzer1949",)
    for law in ("RogersYau", "PowerSeries"):
        with pytest.raises(NotImplementedError, match=law):
            cc.runner(engine, "default", cc.ensemble((5, 9)), "stages",
                      collisions=cc.setup_of("geometric"), terminal_velocity=law)


# ---- 2. order matters and is followed --------------------------------------------------------------
def order_case():
    """cloud water of the order of 1 g/kg, so that the order of the sums over the droplets reaches
    the last bits of thd and qv"""
    return cc.ensemble((257, 600), seed=5, multiplicity=3_000_000)


def run_in_row_order(engine, kwargs, steps, **more):
    """the stage route with the parcel step forced to row order: before every step `idx` is
    replaced by its sorted self (the live rows, ascending)"""
    runner = cc.runner(engine, "default", kwargs, "stages", **more)
    for _ in range(steps):
        state = runner.snapshot()
        starts = runner.parcel_start_host
        idx = state["idx"].copy()
        for c in range(runner.n_parcel):
            live = slice(starts[c], starts[c] + state["n_live"][c])
            idx[live] = np.sort(idx[live])
        runner.restore({"idx": idx})
        runner.run(1)
    return runner.snapshot()


def check_order_is_followed(engine, reference_engine):
    kwargs = order_case()
    more = dict(collisions=cc.setup_of("constant"))
    sorted_state = run_in_row_order(reference_engine, kwargs, 3, **more)
    followed = cc.run(reference_engine, "default", kwargs, "stages", 3, **more)[0]
    differs = [not np.array_equal(pc.bits(followed[key]), pc.bits(sorted_state[key]))
               for key in ("thd", "qv")]
    assert any(differs)  # the checker shows the difference on this case ...
    fused = cc.run(engine, "default", kwargs, "fused", 3, **more)[0]
    assert followed["coalescence_rate"].sum() > 0
    pc.assert_same_bits(fused, followed, "fused vs the permutation's order")  # ... and it is followed
    assert any(not np.array_equal(pc.bits(fused[key]), pc.bits(sorted_state[key]))
               for key in ("thd", "qv"))


def test_the_sums_follow_the_permutation(engine):
    check_order_is_followed(engine, engine)


# ---- 3. continuation -------------------------------------------------------------------------------
def check_continuation(engine):
    kwargs = cc.ensemble((3, 65, 300), seed=13)
    more = dict(collisions=cc.setup_of("constant"), seed=(5, 6, 7))
    whole = cc.run(engine, "default", kwargs, "fused", 9, **more)
    assert (whole[0]["n_live"][1:] < (65, 300)).all()
    for split in ((4, 5), (1,) * 9):
        runner = cc.runner(engine, "default", kwargs, "fused", **more)
        parts = [runner.run(n) for n in split]
        pc.assert_same_bits(whole[0], runner.snapshot(), f"state, {split}")
        pc.assert_same_bits(whole[1], cc.concatenated([p[0] for p in parts]), f"profile, {split}")
        pc.assert_same_bits(whole[2], cc.concatenated([p[1] for p in parts]),
                            f"coalescence profile, {split}")


def test_continuation(engine):
    """run(9) == run(4); run(5) == nine run(1): all state, stream positions included, is in the
    arrays"""
    check_continuation(engine)


def test_snapshot_and_restore_carry_the_new_arrays(engine):
    kwargs = cc.ensemble((3, 65, 300), seed=13)
    more = dict(collisions=cc.setup_of("constant"), seed=(5, 6, 7))
    runner = cc.runner(engine, "default", kwargs, "fused", **more)
    runner.run(3)
    kept = runner.snapshot()
    runner.run(4)
    after = runner.snapshot()
    assert not np.array_equal(after["rng_offset"], kept["rng_offset"])
    runner.restore(kept)
    pc.assert_same_bits(runner.snapshot(), kept, "restored")
    runner.run(4)
    pc.assert_same_bits(runner.snapshot(), after, "run again from the snapshot")


# ---- 4. independence and seeds ---------------------------------------------------------------------
def check_independence(engine):
    sizes = (3, 64, 65, 300)
    kwargs = cc.ensemble(sizes, seed=21)
    seeds = np.array([3, 4, 5, 6])
    more = dict(collisions=cc.setup_of("golovin"))
    whole = cc.runner(engine, "default", kwargs, "fused", seed=seeds, **more)
    whole.run(4)
    state = whole.snapshot()
    starts = whole.parcel_start_host
    formulae = cc.formulae_of("default")
    for c, size in enumerate(sizes):
        alone = cc.runner(engine, "default", cc.solo(kwargs, formulae, starts, c), "fused",
                          seed=int(seeds[c]), **{**more, "collisions": cc.setup_of("golovin")})
        alone.run(4)
        solo = alone.snapshot()
        rows = slice(int(starts[c]), int(starts[c + 1]))
        for key, value in solo.items():
            if key == "n_steps":
                continue
            where = rows if value.size == size and key not in pc.STATE_KEYS[:15] and (
                key not in cc.COUNTERS + ("n_live", "stats_n_substep", "stats_dt_min", "events",
                                          "rng_offset")) else slice(c, c + 1)
            mine = state[key][where]
            if key == "idx":
                mine = np.where(mine >= 0, mine - starts[c], -1)
            assert np.array_equal(pc.bits(mine), pc.bits(value)), (c, key)


def test_a_parcel_of_an_ensemble_equals_its_solo_run(engine):
    check_independence(engine)


def check_seeds(engine):
    one = cc.ensemble((200,), seed=8)
    twice = {key: (value if key == "dt" or value is None else np.concatenate([value] * 3))
             for key, value in one.items()}
    runner = cc.runner(engine, "default", twice, "fused", collisions=cc.setup_of("constant"),
                       seed=(9, 9, 10))
    runner.run(4)
    state = runner.snapshot()
    rows = [slice(200 * c, 200 * (c + 1)) for c in range(3)]
    for key in ("water_mass", "multiplicity", "dry_volume", "kappa"):
        assert np.array_equal(pc.bits(state[key][rows[0]]), pc.bits(state[key][rows[1]])), key
    assert np.array_equal(state["idx"][rows[0]] >= 0, state["idx"][rows[1]] >= 0)
    live = state["idx"][rows[0]] >= 0
    assert np.array_equal(state["idx"][rows[0]][live] + 200, state["idx"][rows[1]][live])
    for key in ("thd", "qv", "n_live", "rng_offset", "coalescence_rate"):
        assert np.array_equal(pc.bits(state[key][0:1]), pc.bits(state[key][1:2])), key
    assert state["coalescence_rate"][0] > 0
    assert not np.array_equal(state["multiplicity"][rows[0]], state["multiplicity"][rows[2]])


def test_equal_seeds_stay_equal_and_different_seeds_differ(engine):
    check_seeds(engine)


# ---- 5. edges ----------------------------------------------------------------------------------------
def check_the_largest_parcel(engine):
    """SDM_PARCEL_COAL_MAX_ROWS rows on both routes; one more is refused by name"""
    kwargs = cc.ensemble((cc.MAX_ROWS, 5), seed=4)
    more = dict(collisions=cc.setup_of("constant"))
    fused = cc.run(engine, "default", kwargs, "fused", 2, **more)
    stages = cc.run(engine, "default", kwargs, "stages", 2, **more)
    cc.assert_same_run(fused, stages, "the largest parcel")
    assert fused[0]["n_live"][0] < cc.MAX_ROWS and fused[0]["coalescence_rate"][0] > 0
    for route in ("fused", "stages"):
        with pytest.raises(ValueError, match="SDM_PARCEL_COAL_MAX_ROWS"):
            cc.runner(engine, "default", cc.ensemble((cc.MAX_ROWS + 1,)), route)


def test_the_largest_parcel_and_one_row_more(engine):
    check_the_largest_parcel(engine)


def check_more_parcels_than_the_grid_cap(engine):
    """cap + 1 parcels of 3 rows: the workgroups stride; the last parcel equals its solo run"""
    n_parcel = cc.GRID_CAP + 1
    kwargs = cc.ensemble((3,) * n_parcel, seed=6)
    more = dict(collisions=cc.setup_of("golovin", dt_range=(0.5, 100.0)))
    seeds = np.arange(n_parcel) + 100
    runner = cc.runner(engine, "default", kwargs, "fused", seed=seeds, **more)
    runner.run(2)
    state = runner.snapshot()
    assert (state["steps_done"] == 2).all() and (state["rng_offset"] > 0).all()
    assert state["coalescence_rate"].sum() > 0
    formulae = cc.formulae_of("default")
    for c in (0, cc.GRID_CAP - 1, cc.GRID_CAP):
        alone = cc.runner(engine, "default",
                          cc.solo(kwargs, formulae, runner.parcel_start_host, c), "fused",
                          seed=int(seeds[c]),
                          collisions=cc.setup_of("golovin", dt_range=(0.5, 100.0)))
        alone.run(2)
        solo = alone.snapshot()
        rows = slice(3 * c, 3 * c + 3)
        for key in ("water_mass", "multiplicity", "dry_volume", "kappa"):
            assert np.array_equal(pc.bits(state[key][rows]), pc.bits(solo[key])), (c, key)
        for key in ("thd", "qv", "n_live", "rng_offset", "coalescence_rate"):
            assert np.array_equal(pc.bits(state[key][c:c + 1]), pc.bits(solo[key])), (c, key)


def test_more_parcels_than_the_grid_cap(engine):
    check_more_parcels_than_the_grid_cap(engine)


def check_all_rows_but_one_die(engine):
    """every multiplicity is 1 and the constant kernel is strong: the parcels end with one row
    (and go on: further steps with one live row), 64 is crossed downward on the way"""
    kwargs = cc.ensemble((2, 65, 130), seed=9)
    kwargs["multiplicity"] = np.ones_like(kwargs["multiplicity"])
    more = dict(collisions=recipe.CollisionSetup.coalescence(recipe.ConstantK(a=1.0),
                                                             dt_range=(0.05, 100.0)))
    fused = cc.run(engine, "default", kwargs, "fused", 8, **more)
    stages = cc.run(engine, "default", kwargs, "stages", 8, **more)
    cc.assert_same_run(fused, stages, "all but one die")
    assert fused[0]["n_live"].tolist() == [1, 1, 1]
    history = fused[2]["n_live"][:, 1]
    assert history[0] < 64 or (history > 64).any()  # 65 rows: 64 is crossed within the run
    assert (fused[2]["n_live"][-2:] == 1).all()     # steps with a single live row
    state = fused[0]
    for c, (start, size) in enumerate(((0, 2), (2, 65), (67, 130))):
        assert state["multiplicity"][start:start + size].sum() == 1, c


def test_all_rows_but_one_die(engine):
    check_all_rows_but_one_die(engine)


@pytest.mark.parametrize("case", range(len(pc.FAILURE_CASES)), ids=pc.FAILURE_IDS)
def test_a_failed_parcel_keeps_everything_and_the_others_go_on(engine, case):
    check_a_failed_parcel(engine, case)


def check_a_failed_parcel(engine, case):
    """the failure cases of tests/test_parcel_checker.py (a solver that gives up): a failed parcel
    keeps its rows, permutation, counters and stream position from the failed step on, the others
    go on; both routes agree"""
    kind, setup, sizes, seed = pc.FAILURE_CASES[case]
    kwargs = pc.ensemble(sizes, seed=seed)
    kwargs["multiplicity"] = np.where(np.arange(kwargs["multiplicity"].size) % 4 == 0, 1,
                                      kwargs["multiplicity"])
    more = dict(collisions=recipe.CollisionSetup.coalescence(recipe.ConstantK(a=1e-9),
                                                             dt_range=(0.05, 100.0)),
                setup=setup)
    runners = {}
    for route in ("fused", "stages"):
        runners[route] = cc.runner(engine, kind, kwargs, route, **more)
        with pytest.raises(RuntimeError, match="Condensation failed"):
            runners[route].run(5)
    state = runners["fused"].snapshot()
    pc.assert_same_bits(state, runners["stages"].snapshot(), "fused vs stages")
    pc.assert_same_bits(runners["fused"].last_coal_profile, runners["stages"].last_coal_profile,
                        "coalescence profile, fused vs stages")
    failed = state["failed_step"]
    assert (failed >= 0).any() and (failed == -1).any()
    went_on = failed == -1
    assert (state["rng_offset"][went_on] > 0).all()
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
        for key in cc.COUNTERS + ("n_live", "rng_offset", "stats_n_substep", "thd", "qv"):
            assert np.array_equal(pc.bits(again[key][c:c + 1]), pc.bits(state[key][c:c + 1])), key
        # its collisions stopped with its condensation: what it drew, it drew in `failed` steps
        per_step = (rows.stop - rows.start) + (rows.stop - rows.start) // 2
        assert state["rng_offset"][c] % per_step == 0
        assert state["rng_offset"][c] >= failed[c] * per_step
    still = again["failed_step"] == -1  # (in the later-step case others fail in the further run)
    assert still.any() and (again["rng_offset"][still] > state["rng_offset"][still]).all()


def check_dt_min_is_reached(engine):
    """a kernel so strong that the optimal sub-step falls below dt_min: the flag is set and the
    warning of the collision runner is raised (once stats_dt_min holds numbers: its initial NaN
    silences the reference's condition)"""
    kwargs = cc.ensemble((65, 130), seed=9)
    collisions = recipe.CollisionSetup.coalescence(recipe.ConstantK(a=1.0), dt_range=(0.25, 1.0))
    runner = cc.runner(engine, "default", kwargs, "fused", collisions=collisions)
    runner.restore({"stats_dt_min": np.full(2, np.inf)})
    with pytest.warns(UserWarning, match="adaptive time-step reached dt_min"):
        _, record = runner.run(1)
    assert (record["n_substeps"] == 4).all()  # dt / dt_min sub-steps
    state = runner.snapshot()
    assert (state["stats_dt_min"] == 0.25).all()
    assert (state["events"] == 0).all()  # (cleared with the warning)
    again = cc.runner(engine, "default", kwargs, "stages", collisions=collisions)
    again.restore({"stats_dt_min": np.full(2, np.inf)})
    with pytest.warns(UserWarning, match="adaptive time-step reached dt_min"):
        again.run(1)
    pc.assert_same_bits(state, again.snapshot(), "fused vs stages")
    quiet = cc.runner(engine, "default", kwargs, "fused", collisions=collisions)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        quiet.run(1)  # the initial NaN: the flag is set, the condition is false
    assert np.isnan(quiet.snapshot()["stats_dt_min"]).all()


def test_dt_min_is_reached_flagged_and_warned_about(engine):
    check_dt_min_is_reached(engine)


# ---- 6. conservation -------------------------------------------------------------------------------
def check_conservation(engine, route="fused"):
    """over the live rows the sums of n vdry and n ktdv keep their initial values within
    (coalescences + rows) x 2^-52 (every coalescence rounds one product and one sum per attribute,
    every row one product of the final sum); the sum of n never grows"""
    kwargs = cc.ensemble(seed=3)
    runner = cc.runner(engine, "default", kwargs, route, collisions=cc.setup_of("golovin"))
    before = cc.conserved(runner)
    total = [b[2] for b in before]
    for _ in range(5):
        runner.run(1)
        now = cc.conserved(runner)
        assert all(n[2] <= t for n, t in zip(now, total))
        total = [n[2] for n in now]
    state = runner.snapshot()
    assert state["coalescence_rate"].sum() > 0 and (state["n_live"] < cc.SIZES).any()
    for c, size in enumerate(cc.SIZES):
        # (coalescence_rate counts droplets; the pairs that coalesced are at most as many)
        bound = (state["coalescence_rate"][c] + size) * 2.0 ** -52
        for was, is_now in zip(before[c][:2], now[c][:2]):
            assert abs(is_now - was) <= bound * was, (c, was, is_now)


@pytest.mark.parametrize("route", ("fused", "stages"))
def test_dry_volume_and_hygroscopicity_are_conserved(engine, route):
    check_conservation(engine, route)


def test_kappa_follows_the_collisions(engine):
    kwargs = cc.ensemble((5, 70), seed=4)
    runner = cc.runner(engine, "default", kwargs, "fused", collisions=cc.setup_of("golovin"))
    before = runner.snapshot()
    runner.run(2)
    after = runner.snapshot()
    live = after["idx"][after["idx"] >= 0]
    assert np.array_equal(pc.bits(after["kappa"][live]),
                          pc.bits((after["kappa_times_dry_volume"] / after["dry_volume"])[live]))
    assert not np.array_equal(pc.bits(after["kappa"]), pc.bits(before["kappa"]))


def test_diagnose_sees_the_live_rows_in_position_order(engine):
    """`run(k); diagnose(products)`: the table on the gathered live rows; the dead are not counted"""
    from pysdm_amd import products as prod  # pylint: disable=import-outside-toplevel
    from tests import parcel_products_cases as ppc  # pylint: disable=import-outside-toplevel

    kwargs = cc.ensemble((65, 130), seed=9)
    runner = cc.runner(engine, "default", kwargs, "fused", collisions=cc.setup_of("golovin"))
    runner.run(3)
    state = runner.snapshot()
    assert (state["n_live"] < (65, 130)).all()
    table = ppc.full_table(Formulae())
    runner.diagnose(table)
    rows = ppc.raw(runner.last_rows)
    # the same table on a runner WITHOUT collisions that holds exactly the live rows, in order
    live = state["idx"][state["idx"] >= 0]
    formulae = Formulae()
    plain = ParcelRunner(engine, formulae, CondensationSetup(), dt=1.0, T0=290.0, p0=90000.0,
                         qv0=0.01, w=1.0, mass_of_dry_air=1.0, counts=state["n_live"],
                         multiplicity=state["multiplicity"][live],
                         water_mass=state["water_mass"][live],
                         dry_volume=state["dry_volume"][live], kappa=state["kappa"][live])
    plain.restore({key: state[key] for key in ("T", "rhod", "mass_of_dry_air")})
    plain.diagnose(table)
    for key, value in ppc.raw(plain.last_rows).items():
        assert np.array_equal(pc.bits(rows[key]), pc.bits(value)), key
    with pytest.raises(NotImplementedError, match="diagnose"):
        runner.run(1, products=[prod.ParticleConcentration()] if hasattr(
            prod, "ParticleConcentration") else table)


# ---- 7. refusals -------------------------------------------------------------------------------------
def test_refusals_by_name(engine):
    kwargs = pc.saturated(cc.ensemble((5, 9), seed=3), Formulae())
    kernel = recipe.ConstantK(a=1e-3)
    refused = {
        "breakup": recipe.CollisionSetup.breakup_only(kernel, recipe.AlwaysN(2)),
        "optimized_random": recipe.CollisionSetup.coalescence(kernel, optimized_random=True),
        "global croupier": recipe.CollisionSetup.coalescence(kernel, croupier="global"),
    }
    for route in ("fused", "stages"):
        for name, setup in refused.items():
            with pytest.raises(NotImplementedError, match=name):
                ParcelRunner(engine, Formulae(), CondensationSetup(), route=route,
                             collisions=setup, **kwargs)
        with pytest.raises(NotImplementedError, match="(?i)coalescence: a ventilation"):
            ventilated, descriptor = vc.formulae_of("Froessling1938")
            ParcelRunner(engine, ventilated, CondensationSetup(), route=route,
                         collisions=cc.setup_of(), terminal_velocity="GunnKinzer1949",
                         descriptor=descriptor, **kwargs)
        with pytest.raises(NotImplementedError, match="chemistry"):
            from tests import parcel_chem_cases as chem  # pylint: disable=import-outside-toplevel

            ParcelRunner(engine, Formulae(), CondensationSetup(), route=route,
                         collisions=cc.setup_of(), chemistry=chem.setup_of(),
                         mole_fractions=chem.MOLE_FRACTIONS, dry_rho=chem.DRY_RHO,
                         dry_molar_mass=chem.DRY_MOLAR_MASS, **kwargs)
    # ... and so does the library, by name
    library = {"enable_breakup": ("enable_breakup", 1), "optimized_random": ("optimized_random", 1),
               "croupier": ("croupier_local", 0), "velocity_source": ("velocity_source", 1)}
    for name, (field, value) in library.items():
        runner = ParcelRunner(engine, Formulae(), CondensationSetup(), collisions=cc.setup_of(),
                              **kwargs)
        setattr(runner.coal_cfg, field, value)
        with pytest.raises(RuntimeError, match=name):
            runner.run(1)
    runner = ParcelRunner(engine, Formulae(), CondensationSetup(), collisions=cc.setup_of(),
                          **kwargs)
    runner.restore({"idx": np.arange(14)[::-1].copy()})  # rows of the other parcel
    with pytest.raises(RuntimeError, match="idx"):
        runner.run(1)
    runner = ParcelRunner(engine, Formulae(), CondensationSetup(), collisions=cc.setup_of(),
                          **kwargs)
    runner.restore({"n_live": np.array([6, 9])})
    with pytest.raises(RuntimeError, match="n_live"):
        runner.run(1)
    # an engine without the library says so, and has the stage route
    from tests.parcel_diag_checker import ParcelDiagCheckerEngine  # pylint: disable=import-outside-toplevel

    with pytest.raises(NotImplementedError, match="parcel with coalescence.*route='fused'"):
        ParcelRunner(ParcelDiagCheckerEngine.get(), Formulae(), CondensationSetup(),
                     collisions=cc.setup_of(), **kwargs)
    ParcelRunner(ParcelDiagCheckerEngine.get(), Formulae(), CondensationSetup(), route="stages",
                 collisions=cc.setup_of(), **kwargs).run(1)

"""The fused collision step with the closed-form fall-velocity laws (Rogers-Yau, power series) on
the GPU: on every route of fused.hip the fused step, the stage route on the GPU and the stage route
of the CPU checker leave the same state - integers equal, floats bit for bit, breakup included
(every side evaluates pow with csrc/sdm_math.h, and the laws are one function in physics.h).
Shapes are the smallest that reach each route; the input plants radii on, and within eight ulps of,
both limits of Rogers-Yau (tests/velocity_law_cases.py)."""
import copy
import warnings

import numpy as np
import pytest

from pysdm_amd import recipe as R
from pysdm_amd.cases import make_box

from . import velocity_law_cases as vc
from .trajectory import compare

pytestmark = pytest.mark.gpu

LAWS = ("rogers_yau", "power_series", "two_terms")
_EXPECTED = {}


def assert_same(a, b):
    """as test_hip_parity.assert_same: everything, `idx` up to the live length"""
    length = int(a["length"])
    assert length == int(b["length"])
    for key, value in a.items():
        ref = b[key]
        if key == "idx":  # beyond `length`: dead storage (see trajectory.compare)
            value, ref = value[:length], ref[:length]
        assert value.dtype == ref.dtype, key
        np.testing.assert_array_equal(value, ref, err_msg=key)


def run(runner, chunks, sync=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for steps in chunks:
            runner.run(steps)
        if sync:
            runner.sync()
    return runner.snapshot()


def expected(key, make, steps):
    """the CPU checker's stage route, computed once per case"""
    if key not in _EXPECTED:
        _EXPECTED[key] = run(make("chain"), (steps,))
    return _EXPECTED[key]


def cells_input(n_cell, per_cell):
    """the planted input spread over `n_cell` cells of exactly `per_cell`; dv of one cell such that
    the concentration is the box's"""
    n_sd = n_cell * per_cell
    volume, multiplicity = vc.planted(n_sd)
    cell_id = np.random.default_rng(vc.PLANT_SEED + n_cell).permutation(n_sd) % n_cell
    return {"volume": volume, "multiplicity": multiplicity, "cell_id": cell_id.astype(np.int64),
            "dv": vc.PLANT_DV * per_cell / 1024}


# ---- one cell ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", LAWS)
def test_one_cell_non_adaptive_every_way_of_stepping(law, hip_engine, oracle_engine):
    """four calls of one step (k_pair_all), one call of four (k_pair_all_sort with the build in
    between), and the same without read-back followed by sync()"""
    def make(engine, route, **options):
        return vc.box_runner(engine, vc.law_of(law), route=route, adaptive=False, **options)

    want = expected(("box_na", law), lambda route: make(oracle_engine, route), 4)
    assert want["coalescence_rate"].sum() > 100 and int(want["length"]) < 1024
    assert_same(run(make(hip_engine, "chain"), (4,)), want)
    assert_same(run(make(hip_engine, "fused"), (1, 1, 1, 1)), want)
    assert_same(run(make(hip_engine, "fused"), (4,)), want)
    lazy = make(hip_engine, "fused")
    lazy.read_back = False
    assert_same(run(lazy, (4,), sync=True), want)


@pytest.mark.parametrize("law", LAWS)
def test_one_cell_adaptive(law, hip_engine, oracle_engine):
    """k_pair_prob / k_pair_update"""
    def make(engine, route):
        return vc.box_runner(engine, vc.law_of(law), route=route, adaptive=True)

    want = expected(("box_a", law), lambda route: make(oracle_engine, route), 4)
    assert want["stats_n_substep"].max() > 4
    assert_same(run(make(hip_engine, "chain"), (4,)), want)
    assert_same(run(make(hip_engine, "fused"), (1, 3)), want)


@pytest.mark.parametrize("law", LAWS)
def test_one_cell_breakup_on_a_rain_spectrum(law, hip_engine, oracle_engine):
    """Straub2010Ec + Straub2010Nf (k_resolve_dense), 8 steps.  The closed forms have no table top:
    the fused route neither faults nor refuses whatever size the drops reach (the largest radius is
    printed; the stage routes with the table refuse above 6 mm)"""
    def make(engine, route):
        return make_box(engine, "straub_rain", n_sd=2048, adaptive=True, dt=10.0, route=route,
                        terminal_velocity=vc.law_of(law))

    want = expected(("rain", law), lambda route: make(oracle_engine, route), 8)
    assert want["breakup_rate"].sum() > 0 and want["coalescence_rate"].sum() > 0
    alive = want["multiplicity"] > 0
    print(f"{law}: largest radius {vc.device_radius(want['attributes'][0][alive] / 1000).max()} m")
    assert_same(run(make(hip_engine, "chain"), (8,)), want)
    assert_same(run(make(hip_engine, "fused"), (3, 5)), want)


# ---- cells --------------------------------------------------------------------------------------------
def _cells(law, hip_engine, oracle_engine, key, n_cell, per_cell, grid, chunks, shapes=(0,),
           second_row=False, adaptive=True, **options):
    given = cells_input(n_cell, per_cell)
    more = {"tracer": np.linspace(1.0, 2.0, n_cell * per_cell)} if second_row else None

    def make(engine, route):
        return vc.box_runner(engine, vc.law_of(law), route=route, adaptive=adaptive, grid=grid,
                             more_extensive=copy.deepcopy(more), **given, **options)

    steps = sum(chunks)
    want = expected((key, law), lambda route: make(oracle_engine, route), steps)
    assert want["coalescence_rate"].sum() > 100
    sizes = np.bincount(given["cell_id"], minlength=n_cell)  # (as the first step meets them)
    assert_same(run(make(hip_engine, "chain"), (steps,)), want)
    try:
        for shape in shapes:
            hip_engine.call("sdm_ctx_set_option", 2, shape)
            assert_same(run(make(hip_engine, "fused"), chunks), want)
    finally:
        hip_engine.call("sdm_ctx_set_option", 2, 0)
    return sizes


@pytest.mark.parametrize("law", LAWS)
def test_sixteen_cells_of_64_packed(law, hip_engine, oracle_engine):
    """k_cell_step2, eight cells per workgroup, both variants: cells of 64 take the one for cells of
    at most 384 by themselves (TINY), and SDM_CELL_SHAPE_512 forces the one for cells of at most
    704 on them (sdm_hip.h), which cells of 385 .. 704 take"""
    sizes = _cells(law, hip_engine, oracle_engine, "16x64", 16, 64, (4, 4), (1, 3), shapes=(0, 1))
    assert sizes.max() == 64


@pytest.mark.parametrize("law", LAWS)
def test_four_cells_of_1000_in_every_shape(law, hip_engine, oracle_engine):
    """k_cell_step2 one cell per workgroup: the automatic shape (1024 threads: fewer cells than
    CUs) and the two others forced (SDM_OPT_CELL_SHAPE: 512 and 256 threads)"""
    sizes = _cells(law, hip_engine, oracle_engine, "4x1000", 4, 1000, (2, 2), (1, 3),
                   shapes=(0, 1, 3))
    assert sizes.max() == 1000  # (above the 704 of the packed variant, below every shape's cap)


@pytest.mark.parametrize("law", LAWS)
def test_sixteen_cells_of_64_with_a_second_extensive_row(law, hip_engine, oracle_engine):
    """k_cell_step (the kernel for any number of attributes)"""
    _cells(law, hip_engine, oracle_engine, "16x64+row", 16, 64, (4, 4), (1, 3), second_row=True)


@pytest.mark.parametrize("law", LAWS)
def test_two_cells_of_7000_take_the_generic_kernels(law, hip_engine, oracle_engine):
    """above CELL_CAP = 6144"""
    sizes = _cells(law, hip_engine, oracle_engine, "2x7000", 2, 7000, (2, 1), (1, 2))
    assert sizes.max() > 6144


@pytest.mark.parametrize("law", LAWS)
def test_four_by_four_global_croupier_non_adaptive(law, hip_engine, oracle_engine):
    _cells(law, hip_engine, oracle_engine, "4x4 global", 16, 64, (4, 4), (1, 3), adaptive=False,
           croupier="global")


# ---- the reference's recorded runs ------------------------------------------------------------------
@pytest.mark.parametrize("route", ["chain", "fused"])
@pytest.mark.parametrize("name", sorted(vc.GOLDENS))
def test_goldens_of_the_reference(name, route, hip_engine):
    runner, gold, steps = vc.golden_runner(name, hip_engine, route)
    breakup = vc.GOLDENS[name][1]
    for step in steps:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runner.run(step - runner.steps_done)
        compare(runner.snapshot(), gold, step, float_rtol=1e-12 if breakup else 0.0,
                idx_tail=route != "fused")


# ---- argument checks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["law out of range", "negative law", "17 terms",
                                  "no Rogers-Yau constants", "no series terms", "no table"])
def test_bad_law_descriptions_are_refused_before_anything_is_launched(case, hip_engine):
    law = {"17 terms": "PowerSeries", "no series terms": "PowerSeries",
           "no table": "GunnKinzer1949"}.get(case, "RogersYau")
    runner = vc.box_runner(hip_engine, law, route="fused", adaptive=False)
    before = runner.snapshot()
    cfg, state = runner.step_cfg(), runner._step_state()  # pylint: disable=protected-access
    if case == "law out of range":
        cfg.velocity_law = 3
    elif case == "negative law":
        cfg.velocity_law = -1
    elif case == "17 terms":
        cfg.velocity_terms = 17
    elif case == "no table":
        state.gk_a = None
    else:
        state.velocity_params = None
    with pytest.raises(RuntimeError, match="error -1"):  # SDM_E_ARG
        hip_engine.call("sdm_collision_step", cfg, state, runner._result, 3)  # pylint: disable=protected-access
    assert "bad argument" in hip_engine.library.last_error()
    hip_engine.synchronize()
    after = runner.snapshot()
    for key, value in before.items():
        np.testing.assert_array_equal(after[key], value, err_msg=key)


def test_a_series_of_no_terms_and_an_unused_law_run(hip_engine, oracle_engine):
    """zero terms is the velocity 0 and reads no parameters; a set-up that needs no velocity
    (Golovin) runs under any law code without them"""
    runner = vc.box_runner(hip_engine, "PowerSeries", route="fused", adaptive=False)
    cfg, state = runner.step_cfg(), runner._step_state()  # pylint: disable=protected-access
    cfg.velocity_terms = 0
    state.velocity_params = None
    hip_engine.call("sdm_collision_step", cfg, state, runner._result, 3)  # pylint: disable=protected-access
    hip_engine.synchronize()
    snap = runner.snapshot()
    assert snap["collision_rate"].sum() == 0  # nothing falls: the geometric kernel vanishes

    volume, multiplicity = vc.planted()
    snaps = []
    for engine, code in ((hip_engine, 1), (oracle_engine, 0)):
        golovin = vc.box_runner(engine, "GunnKinzer1949", route="fused", adaptive=False,
                                volume=volume, multiplicity=multiplicity, dv=1e-6,
                                setup=R.CollisionSetup.coalescence(R.Golovin(b=1.5e3), seed=44))
        golovin.step_cfg().velocity_law = code
        snaps.append(run(golovin, (2,)))
    assert snaps[1]["collision_rate"].sum() > 0
    assert_same(snaps[0], snaps[1])

"""The mixed-phase parcel without a GPU (include/sdm_parcel_ice.h): the CPU checker
(tests/parcel_ice_checker/, `route="fused"` on the checker engine) against the stage route of
pysdm_amd/parcel_ice.py on the same engine - two independent restatements of the header's step over
the same stage symbols -, the properties the header promises, and the refusals.  Comparisons are bit
for bit."""
import ctypes
import json
import os

import numpy as np
import pytest

from pysdm_amd import abi
from pysdm_amd.condensation import CondensationSetup
from pysdm_amd.formulae import Formulae
from pysdm_amd.freezing import FreezingSetup
from pysdm_amd.parcel import ParcelRunner
from tests import parcel_cases as pc
from tests import parcel_ice_cases as ic

MODES = ("singular", "abifm", "constant_thaw", "homogeneous", "both")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = (1, 40, 70, 300)
PLAIN_ONLY = ("freezing_temperature", "immersed_surface_area", "ice_seed")


@pytest.fixture(scope="module")
def engine():
    from tests.parcel_ice_checker import ParcelIceCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelIceCheckerEngine.get()


def test_the_structs_are_the_headers(engine):
    assert (ctypes.sizeof(abi.ParcelIceCfg)
            == engine.parcel_ice_library.cdll.parcel_ice_checker_cfg_size())
    assert ctypes.sizeof(abi.ParcelIceState) == 8 * len(abi.PARCEL_ICE_STATE_FIELDS)
    assert "sdm_parcel_run_ice" in abi.parse_header(abi.PARCEL_ICE_HEADER_PATH)


def test_the_product_library_has_the_symbol():
    assert hasattr(abi.parcel_ice_library().cdll, "sdm_parcel_run_ice")


@pytest.mark.parametrize("coordinate", ("WaterMassLogarithm", "WaterMass"))
@pytest.mark.parametrize("sum_mode", ("ordered", "blocked"))
@pytest.mark.parametrize("order", ("freezing_first", "deposition_first"))
@pytest.mark.parametrize("mode", MODES)
def test_the_checker_equals_the_stage_route(engine, mode, order, sum_mode, coordinate):
    kwargs = ic.ensemble(SIZES, seed=7, mode=mode, dry=(1,))
    tiny = None
    if coordinate == "WaterMass":
        kwargs, tiny = ic.with_tiny_crystal(kwargs, 1)
    more = dict(mode=mode, order=order, sum_mode=sum_mode, coordinate=coordinate)
    fused = ic.run(engine, kwargs, "fused", 5, **more)
    state, _, ice_profile = fused
    assert (state["steps_done"] == 5).all()
    assert 0.1 < ic.frozen_fraction(kwargs, state) < 0.9
    assert (ice_profile["RH_ice"][:, 1] < 1).all() and (ice_profile["RH_ice"][:, 2:] > 1).all()
    if tiny is not None:
        assert kwargs["water_mass"][tiny] < 0 < state["water_mass"][tiny]
    ic.assert_same_run(fused, ic.run(engine, kwargs, "stages", 5, **more), "checker vs stages")


@pytest.fixture(scope="module")
def runs():
    return np.load(os.path.join(GOLDEN, "parcel_ice_runs.npz"))


@pytest.mark.parametrize("route", ("fused", "stages"))
@pytest.mark.parametrize("run", ("a", "b", "c"))
def test_the_recorded_runs_of_the_reference(engine, runs, run, route):
    """tests/golden/parcel_ice_runs.npz (gen_parcel_ice_golden.py: PySDM's `Parcel(mixed_phase=
    True)` itself): z, n_ice per step, the sub-step counts, the final sign pattern and the stream
    position exactly, the floats within max(4 x the reference's spread, the per-call bound) - which
    is what tests the timing of Moist.sync, of the stale T / p / RH and of the streams"""
    worst = ic.compare_with_golden(runs, run, ic.golden_runner(engine, runs, run, route))
    print(run, route, worst)
    assert worst.pop("z") == 0
    for quantity, value in worst.items():
        assert value <= ic.golden_bound(runs, run, quantity), (run, quantity, value)


def test_the_measured_differences_are_the_recorded_ones(engine, runs):
    """tests/golden/parcel_ice_measured.json holds what the comparison above measured when the
    golden was made (a document, not a bound): the checker still measures the same"""
    with open(os.path.join(GOLDEN, "parcel_ice_measured.json"), encoding="utf-8") as handle:
        recorded = json.load(handle)
    for run in ("a", "b", "c"):
        worst = ic.compare_with_golden(runs, run, ic.golden_runner(engine, runs, run, "fused"))
        assert worst == pytest.approx(recorded[run]["checker"], rel=1e-6, abs=1e-300)


def test_the_order_of_the_passes_matters(engine):
    """deposition first: a droplet that freezes in a step does not grow by deposition in it"""
    kwargs = ic.ensemble(SIZES, seed=7, mode="singular")
    a = ic.run(engine, kwargs, "fused", 3, mode="singular", order="freezing_first")
    b = ic.run(engine, kwargs, "fused", 3, mode="singular", order="deposition_first")
    assert np.array_equal(a[0]["water_mass"] < 0, b[0]["water_mass"] < 0)
    assert (a[0]["water_mass"] != b[0]["water_mass"]).any()


def test_the_sum_modes_differ_in_the_last_bits_only(engine):
    """one step (later steps pass the difference through a solver with tolerances of 1e-6): two
    orders of adding at most 600 terms, none larger than the sum, to the same start differ by less
    than 600 roundings of the result"""
    kwargs = ic.ensemble((600,), seed=7, mode="singular")
    a = ic.run(engine, kwargs, "fused", 1, mode="singular", sum_mode="ordered")
    b = ic.run(engine, kwargs, "fused", 1, mode="singular", sum_mode="blocked")
    assert np.array_equal(pc.bits(a[0]["water_mass"]), pc.bits(b[0]["water_mass"]))
    np.testing.assert_allclose(a[1]["qv"], b[1]["qv"], rtol=600 * 2.0 ** -52)
    np.testing.assert_allclose(a[1]["thd"], b[1]["thd"], rtol=600 * 2.0 ** -52)


def test_the_ice_profile(engine):
    """n_ice is the exact count, ice_mass the SUM of include/sdm_parcel_diag.h, the pair is the one
    the next step reads"""
    from pysdm_amd.parcel import diag_sum  # pylint: disable=import-outside-toplevel

    kwargs = ic.ensemble(SIZES, seed=7, mode="both", dry=(1,))
    runner = ic.runner(engine, kwargs, "fused", mode="both")
    _, ice_profile = runner.run(3)
    state = runner.snapshot()
    start = np.concatenate(([0], np.cumsum(SIZES)))
    for c in range(len(SIZES)):
        m = state["water_mass"][start[c]:start[c + 1]]
        mult = kwargs["multiplicity"][start[c]:start[c + 1]]
        assert ice_profile["n_ice"][-1, c] == mult[m < 0].sum()
        assert ice_profile["ice_mass"][-1, c] == diag_sum(mult, np.where(m < 0, -m, 0.0))
    assert np.array_equal(ice_profile["a_w_ice"][-1], state["a_w_ice"])
    assert np.array_equal(ice_profile["RH_ice"][-1], state["RH_ice"])
    assert (ice_profile["dv"] > 0).all()


def test_no_ice_equals_the_plain_parcel(engine):
    kwargs = ic.ensemble(SIZES, seed=9, mode="singular", ice_fraction=0.0)
    kwargs["freezing_temperature"] = np.full_like(kwargs["freezing_temperature"], 100.0)
    state, profile, ice_profile = ic.run(engine, kwargs, "fused", 5, mode="singular")
    assert (ice_profile["n_ice"] == 0).all() and (ice_profile["ice_mass"] == 0).all()
    formulae = Formulae()
    plain = ParcelRunner(engine, formulae, CondensationSetup(), route="fused", **pc.saturated(
        {key: value for key, value in kwargs.items() if key not in PLAIN_ONLY}, formulae))
    plain_profile = plain.run(5)
    plain_state = plain.snapshot()
    pc.assert_same_bits(profile, plain_profile, "profile")
    pc.assert_same_bits({key: state[key] for key in plain_state}, plain_state, "state")


def test_continuation_and_restore(engine):
    kwargs = ic.ensemble((3, 65, 300), seed=13, mode="both", dry=(1,))
    whole = ic.run(engine, kwargs, "fused", 9, mode="both")
    runner = ic.runner(engine, kwargs, "fused", mode="both")
    runner.run(4)
    middle = runner.snapshot()
    runner.run(5)
    pc.assert_same_bits(whole[0], runner.snapshot(), "run(4); run(5)")
    assert whole[0]["rng_offset"].tolist() == [2 * 9 * n for n in (3, 65, 300)]
    again = ic.runner(engine, kwargs, "fused", mode="both")
    again.restore(middle)
    again.run(5)
    pc.assert_same_bits(whole[0], again.snapshot(), "restore(snapshot after 4); run(5)")


def test_a_failed_parcel_keeps_its_state(engine):
    kwargs = ic.ensemble((20, 30, 300, 1100, 7, 65), seed=6, mode="both")
    more = dict(mode="both", setup=CondensationSetup(adaptive=False, substeps=2, max_iters=3))
    results = []
    for route in ("fused", "stages"):
        runner = ic.runner(engine, kwargs, route, **more)
        with pytest.raises(RuntimeError, match="Condensation failed"):
            runner.run(5)
        results.append((runner.snapshot(), runner.last_profile, runner.last_ice_profile))
    state = results[0][0]
    failed = state["failed_step"]
    assert (failed == 0).any() and (failed > 0).any() and (failed == -1).any()
    sizes = np.array((20, 30, 300, 1100, 7, 65))
    assert state["rng_offset"].tolist() == (2 * sizes * state["steps_done"]).tolist()
    ic.assert_same_run(results[0], results[1], "checker vs stages")


def test_a_row_that_exceeds_the_vapour_is_counted(engine):
    kwargs, _ = ic.with_exceeding_row(ic.ensemble((65, 257), seed=5, mode="singular"), 1)
    state, profile, ice_profile = ic.run(engine, kwargs, "fused", 1, mode="singular")
    assert state["n_exceeded"].tolist() == [0, 1] and ice_profile["n_exceeded"].tolist() == [[0, 1]]
    assert profile["qv"][0, 1] < 0


def test_the_refusals(engine):
    kwargs = ic.ensemble((5, 9), seed=1, mode="singular")
    with pytest.raises(NotImplementedError, match="ice_order"):
        ic.runner(engine, kwargs, "fused", mode="singular", order="interleaved")
    with pytest.raises(ValueError, match="freezing_temperature"):
        ic.runner(engine, {**kwargs, "freezing_temperature": None}, "fused", mode="singular")
    with pytest.raises(NotImplementedError, match="MixedPhaseSpheres"):
        formulae = Formulae()
        ParcelRunner(engine, formulae, CondensationSetup(), route="fused",
                     freezing=FreezingSetup(), freezing_temperature=kwargs["freezing_temperature"],
                     **pc.saturated({key: value for key, value in kwargs.items()
                                     if key not in PLAIN_ONLY}, formulae))
    runner = ic.runner(engine, kwargs, "fused", mode="singular")
    cfg = runner.ice.cfg
    cfg.freezing = cfg.deposition = 0  # both passes off: that is sdm_parcel_run
    with pytest.raises(RuntimeError, match="both passes off"):
        runner.run(1)
    runner = ic.runner(engine, kwargs, "fused", mode="singular")
    runner.ice.freezing_temperature = None  # a column the configuration reads
    with pytest.raises(RuntimeError, match="freezing_temperature"):
        runner.run(1)


def test_an_engine_without_the_library_says_so(oracle_engine):
    with pytest.raises(NotImplementedError, match="mixed-phase parcel"):
        oracle_engine.call_parcel_ice("sdm_parcel_run_ice")

"""The mixed-phase parcel on the GPU (include/sdm_parcel_ice.h; k_parcel_i / k_parcel_f_i): every
comparison is HIP against the CPU checker (tests/parcel_ice_checker/), HIP against its own stage
route or HIP against HIP, bit for bit, viewed as uint8.  No test provokes a fault: the failure
cases are solvers that report success = 0, which the kernels handle without trapping."""
import numpy as np
import pytest

from pysdm_amd import deposition as dep
from pysdm_amd.condensation import CondensationSetup
from pysdm_amd.formulae import Formulae
from pysdm_amd.parcel import ParcelRunner
from tests import parcel_cases as pc
from tests import parcel_ice_cases as ic

pytestmark = pytest.mark.gpu

MODES = ("singular", "abifm", "constant_thaw", "homogeneous", "both")
# the second parcel (255 rows) is all ice below ice saturation: its crystals sublimate
DRY = (1,)
N_STEPS = 5


def _checker():
    from tests.parcel_ice_checker import ParcelIceCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelIceCheckerEngine.get()


@pytest.mark.parametrize("coordinate", ("WaterMassLogarithm", "WaterMass"))
@pytest.mark.parametrize("sum_mode", ("ordered", "blocked"))
@pytest.mark.parametrize("order", ("freezing_first", "deposition_first"))
@pytest.mark.parametrize("mode", MODES)
def test_hip_fused_equals_the_checker_equals_the_stage_route(hip_engine, mode, order, sum_mode,
                                                             coordinate):
    """five parcels of 1 .. 1025 rows (one row, the lane edge, past the register-cached rows), five
    steps; PySDM's default coordinate on k_parcel_i, WaterMass on k_parcel_f_i - there with a
    crystal that sublimates through zero.  Non-vacuity is asserted on the checker's result"""
    kwargs = ic.ensemble(ic.EDGE_SIZES, seed=7, mode=mode, dry=DRY)
    tiny = None
    if coordinate == "WaterMass":
        kwargs, tiny = ic.with_tiny_crystal(kwargs, DRY[0])
    more = dict(mode=mode, order=order, sum_mode=sum_mode, coordinate=coordinate)
    checker = ic.run(_checker(), kwargs, "fused", N_STEPS, **more)
    state, profile, ice_profile = checker
    assert (state["failed_step"] == -1).all() and (state["steps_done"] == N_STEPS).all()
    if mode in ic.STOCHASTIC:
        assert 0.1 < ic.frozen_fraction(kwargs, state) < 0.9
        passes = 2 if mode == "both" else 1
        assert state["rng_offset"].tolist() == [passes * N_STEPS * n for n in ic.EDGE_SIZES]
    else:
        assert 0.0 < ic.frozen_fraction(kwargs, state) < 1.0
    assert (ice_profile["RH_ice"][:, DRY[0]] < 1).all()  # sublimation ...
    rows = slice(ic.EDGE_SIZES[0] + 1, ic.EDGE_SIZES[0] + ic.EDGE_SIZES[1])
    assert (np.abs(state["water_mass"][rows]) < np.abs(kwargs["water_mass"][rows])).all()
    assert (ice_profile["RH_ice"][:, 2:] > 1).all()  # ... and growth
    grown = (np.asarray(kwargs["water_mass"]) < 0) & (np.arange(state["water_mass"].size)
                                                      >= sum(ic.EDGE_SIZES[:2]))
    assert (state["water_mass"][grown] < kwargs["water_mass"][grown]).all()
    if tiny is not None:
        assert kwargs["water_mass"][tiny] < 0 < state["water_mass"][tiny]
    hip = ic.run(hip_engine, kwargs, "fused", N_STEPS, **more)
    ic.assert_same_run(hip, checker, "fused HIP vs checker")
    ic.assert_same_run(hip, ic.run(hip_engine, kwargs, "stages", N_STEPS, **more),
                       "fused HIP vs stages on HIP")


@pytest.mark.parametrize("run", ("a", "b", "c"))
def test_hip_the_recorded_runs_of_the_reference(hip_engine, run):
    """tests/golden/parcel_ice_runs.npz: the fused route against PySDM's own ascents, with the
    bounds of tests/test_parcel_ice_checker.py, and bit for bit against the checker"""
    import os  # pylint: disable=import-outside-toplevel

    data = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                "parcel_ice_runs.npz"))
    hip = ic.golden_runner(hip_engine, data, run, "fused")
    worst = ic.compare_with_golden(data, run, hip)
    print(run, worst)
    assert worst.pop("z") == 0
    for quantity, value in worst.items():
        assert value <= ic.golden_bound(data, run, quantity), (run, quantity, value)
    checker = ic.golden_runner(_checker(), data, run, "fused")
    checker.run(int(data[f"{run}/cfg/n_steps"]))
    pc.assert_same_bits(hip.snapshot(), checker.snapshot(), "state, fused HIP vs checker")


@pytest.mark.parametrize("capacity,kinetics", (("Columnar", "Standard"), ("Spherical", "Neglect")))
def test_hip_the_other_capacity_and_kinetics(hip_engine, capacity, kinetics):
    kwargs = ic.ensemble((65, 300), seed=3, mode="singular", dry=(0,))
    more = dict(mode="singular", capacity=capacity, kinetics=kinetics)
    hip = ic.run(hip_engine, kwargs, "fused", 3, **more)
    ic.assert_same_run(hip, ic.run(_checker(), kwargs, "fused", 3, **more), "HIP vs checker")


def test_hip_one_pass_only(hip_engine):
    """freezing without deposition and deposition without freezing"""
    kwargs = ic.ensemble((65, 300), seed=3, mode="both", dry=(0,))
    for more in (dict(mode="both", deposition=False), dict(mode="none")):
        hip = ic.run(hip_engine, kwargs, "fused", 3, **more)
        ic.assert_same_run(hip, ic.run(_checker(), kwargs, "fused", 3, **more), "HIP vs checker")


def test_hip_default_formulae_through_the_general_kernel(hip_engine):
    kwargs = ic.ensemble((1, 65, 257), seed=11, mode="both", dry=(1,))
    default = ic.run(hip_engine, kwargs, "fused", 3, mode="both")
    general = ic.run(hip_engine, kwargs, "fused", 3, mode="both", general=True)
    ic.assert_same_run(default, general, "k_parcel_i vs k_parcel_f_i")


def test_hip_more_parcels_than_workgroups_in_flight(hip_engine):
    """3000 parcels of 2 .. 5 rows, 2 steps: far more workgroups than the card holds at once (one
    per CU with this kernel's registers)"""
    sizes = tuple(2 + (c % 4) for c in range(3000))
    kwargs = ic.ensemble(sizes, seed=17, mode="both")
    hip = ic.run(hip_engine, kwargs, "fused", 2, mode="both")
    assert (hip[0]["steps_done"] == 2).all()
    ic.assert_same_run(hip, ic.run(_checker(), kwargs, "fused", 2, mode="both"), "HIP vs checker")


def test_hip_steps_per_launch(hip_engine):
    """1, 5 and 16 steps per launch give the same bits"""
    kwargs = ic.ensemble((3, 65, 300), seed=13, mode="both", dry=(1,))
    runs = [ic.run(hip_engine, kwargs, "fused", 7, mode="both", steps_per_launch=per)
            for per in (1, 5, 16)]
    ic.assert_same_run(runs[0], runs[1], "steps_per_launch 1 vs 5")
    ic.assert_same_run(runs[0], runs[2], "steps_per_launch 1 vs 16")


def test_hip_continuation(hip_engine):
    """run(9) == run(4); run(5), stream positions included"""
    kwargs = ic.ensemble((3, 65, 300), seed=13, mode="both", dry=(1,))
    more = dict(mode="both", sum_mode="blocked")
    whole = ic.run(hip_engine, kwargs, "fused", 9, **more)
    runner = ic.runner(hip_engine, kwargs, "fused", **more)
    parts = [runner.run(n) for n in (4, 5)]
    end = runner.snapshot()
    assert end["rng_offset"].tolist() == [2 * 9 * n for n in (3, 65, 300)]
    pc.assert_same_bits(whole[0], end, "state")
    pc.assert_same_bits(whole[1], ic.concatenated([p[0] for p in parts]), "profile")
    pc.assert_same_bits(whole[2], ic.concatenated([p[1] for p in parts]), "ice profile")


def test_hip_no_ice_equals_the_plain_parcel(hip_engine):
    """nothing is ice and nothing ever freezes (freezing temperatures of 100 K): state, profile
    and masses are those of `sdm_parcel_run`, bit for bit"""
    kwargs = ic.ensemble((1, 65, 257, 1025), seed=9, mode="singular", ice_fraction=0.0)
    kwargs["freezing_temperature"] = np.full_like(kwargs["freezing_temperature"], 100.0)
    state, profile, ice_profile = ic.run(hip_engine, kwargs, "fused", N_STEPS, mode="singular")
    assert (ice_profile["n_ice"] == 0).all() and (ice_profile["ice_mass"] == 0).all()
    plain_kwargs = {key: value for key, value in kwargs.items()
                    if key not in ("freezing_temperature", "immersed_surface_area", "ice_seed")}
    formulae = Formulae()
    plain = ParcelRunner(hip_engine, formulae, CondensationSetup(), route="fused",
                         **pc.saturated(plain_kwargs, formulae))
    plain_profile = plain.run(N_STEPS)
    plain_state = plain.snapshot()
    pc.assert_same_bits(profile, plain_profile, "profile")
    pc.assert_same_bits({key: state[key] for key in plain_state}, plain_state, "state")


def test_hip_all_ice_keeps_the_condensation_s_predictions_plus_the_deposition(hip_engine):
    """a parcel that is all ice: after one step thd and qv are those `sdm_parcel_run` leaves (the
    solver sees no liquid row) with `sdm_deposition`'s ordered additions on top"""
    kwargs = ic.ensemble((300,), seed=21, mode="none", dry=(0,))
    state, profile, _ = ic.run(hip_engine, kwargs, "fused", 1, mode="none")
    assert (state["water_mass"] < 0).all()
    before = ic.runner(hip_engine, kwargs, "fused", mode="none")
    plain_kwargs = {key: value for key, value in kwargs.items()
                    if key not in ("freezing_temperature", "immersed_surface_area", "ice_seed")}
    formulae = Formulae()
    plain = ParcelRunner(hip_engine, formulae, CondensationSetup(), route="fused",
                         **pc.saturated(plain_kwargs, formulae))
    plain_profile = plain.run(1)
    eng, start = hip_engine, before.snapshot()
    ice_formulae = ic.formulae_of("none")
    dv = float(kwargs["mass_of_dry_air"][0]) / ((plain_profile["rhod"][0, 0] + start["rhod"][0]) / 2)
    up = lambda name: eng.upload(np.array(start[name]))  # noqa: E731
    pqv, pthd = eng.upload(plain_profile["qv"][0].copy()), eng.upload(plain_profile["thd"][0].copy())
    eng.call_deposition(
        "sdm_deposition", dep.deposition_cfg(ice_formulae, ic.DT, dv), 300, 1,
        before.multiplicity, before.water_mass, eng.zeros(300, np.int64), up("T"), up("p"),
        up("RH"), up("a_w_ice"), up("qv"), up("rhod"), up("thd"), pqv, pthd, None,
        dep.constants_of(ice_formulae))
    assert np.array_equal(pc.bits(profile["qv"][0]), pc.bits(eng.download(pqv)))
    assert np.array_equal(pc.bits(profile["thd"][0]), pc.bits(eng.download(pthd)))
    assert profile["qv"][0, 0] != plain_profile["qv"][0, 0]
    assert np.array_equal(pc.bits(state["water_mass"]), pc.bits(eng.download(before.water_mass)))


def test_hip_a_failed_parcel_among_good_ones(hip_engine):
    """a solver that gives up (max_iters too small) in some parcels, at the first step and at later
    ones: those parcels stop with masses, stream position and a_w_ice as before the failed step,
    the others go on; HIP == checker == stage route on HIP, also in a second call"""
    kwargs = ic.ensemble((20, 30, 300, 1100, 7, 65), seed=6, mode="both")
    more = dict(mode="both", setup=CondensationSetup(adaptive=False, substeps=2, max_iters=3))
    results = []
    for engine, route in ((hip_engine, "fused"), (_checker(), "fused"), (hip_engine, "stages")):
        runner = ic.runner(engine, kwargs, route, **more)
        with pytest.raises(RuntimeError, match="Condensation failed"):
            runner.run(5)
        first = (runner.snapshot(), runner.last_profile, runner.last_ice_profile)
        try:
            runner.run(2)
        except RuntimeError:  # (a parcel may fail in the second call too)
            pass
        results.append((*first, runner.snapshot(), runner.last_profile, runner.last_ice_profile))
    state = results[0][0]
    failed = state["failed_step"]
    assert (failed == 0).any() and (failed > 0).any() and (failed == -1).any()
    sizes = np.array((20, 30, 300, 1100, 7, 65))
    assert state["rng_offset"].tolist() == (2 * sizes * state["steps_done"]).tolist()
    # a parcel that failed at its first step is where it started
    fresh = ic.runner(hip_engine, kwargs, "fused", **more).snapshot()
    start = np.concatenate(([0], np.cumsum(sizes)))
    for c in np.flatnonzero(failed == 0):
        rows = slice(start[c], start[c + 1])
        assert np.array_equal(pc.bits(state["water_mass"][rows]), pc.bits(fresh["water_mass"][rows]))
        for key in ("a_w_ice", "RH_ice", "thd", "qv", "T"):
            assert state[key][c] == fresh[key][c], key
    for other, what in ((results[1], "checker"), (results[2], "stage route on HIP")):
        for a, b in zip(results[0], other):
            pc.assert_same_bits(a, b, f"fused HIP vs {what}")


def test_hip_thawed_rows_condense_in_the_next_step(hip_engine):
    """a descent through 273.15 K with thaw=True (and a nucleation rate at which nothing freezes
    again): the crystals turn liquid, and the next step's condensation changes their masses; HIP ==
    checker"""
    kwargs = ic.ensemble((65, 257), seed=5, mode="constant_thaw", ice_fraction=0.5)
    kwargs["T0"] = np.array([273.135, 273.14])
    kwargs["w"] = np.array([-3.0, -2.5])
    more = dict(mode="constant_thaw", constants={"J_HET": 1e-300})
    hip = ic.runner(hip_engine, kwargs, "fused", **more)
    masses, n_ice = [hip.snapshot()["water_mass"]], []
    for _ in range(10):
        n_ice.append(int(hip.run(1)[1]["n_ice"].sum()))
        masses.append(hip.snapshot()["water_mass"])
    assert n_ice[0] > 0 and n_ice[-1] == 0
    step = next(k for k, count in enumerate(n_ice) if count == 0)  # the last thaw ran in `step`
    ice = masses[step] < 0
    assert ice.any() and (masses[step + 1][ice] == -masses[step][ice]).all()
    assert (masses[step + 2][ice] != masses[step + 1][ice]).all()
    checker = ic.runner(_checker(), kwargs, "fused", **more)
    checker.run(10)
    pc.assert_same_bits(hip.snapshot(), {**checker.snapshot(), "n_steps": 10}, "state")


def test_hip_a_row_that_exceeds_the_vapour_is_counted_not_trapped(hip_engine):
    kwargs = ic.ensemble((65, 257), seed=5, mode="singular")
    kwargs, _ = ic.with_exceeding_row(kwargs, 1)
    hip = ic.run(hip_engine, kwargs, "fused", 1, mode="singular")
    assert hip[0]["n_exceeded"].tolist() == [0, 1] and hip[2]["n_exceeded"].tolist() == [[0, 1]]
    assert hip[1]["qv"][0, 1] < 0  # (every row was processed as if the assertion were absent)
    ic.assert_same_run(hip, ic.run(_checker(), kwargs, "fused", 1, mode="singular"),
                       "HIP vs checker")


def test_hip_condensation_leaves_ice_rows_alone(hip_engine):
    """stage level: `sdm_condensation` on a cell with ice rows equals the call with those rows
    removed, bit for bit, and leaves the ice rows untouched"""
    from pysdm_amd.condensation import condensation_call  # pylint: disable=import-outside-toplevel

    kwargs = ic.ensemble((1300,), seed=2, mode="singular", ice_fraction=0.3)
    formulae = Formulae()
    sat = pc.saturated({k: v for k, v in kwargs.items() if k not in (
        "freezing_temperature", "immersed_surface_area", "ice_seed")}, formulae)
    probe = ParcelRunner(hip_engine, formulae, CondensationSetup(), route="fused", **sat)
    start = probe.snapshot()
    eng, setup = hip_engine, CondensationSetup()
    results = []
    mass_all = np.array(kwargs["water_mass"])
    for keep in (np.ones(1300, dtype=bool), mass_all > 0):
        n = int(keep.sum())
        column = lambda values: eng.upload(np.ascontiguousarray(np.asarray(values)[keep]))  # noqa: E731
        mass = column(mass_all)
        one = {name: eng.upload(np.array(start[name])) for name in ("rhod", "thd", "qv")}
        pthd, pqv = eng.upload(np.array(start["thd"])), eng.upload(np.array(start["qv"]))
        counters = {name: eng.full(1, np.int64, 4 if name == "n_substeps" else 0) for name in
                    ("n_substeps", "n_activating", "n_deactivating", "n_ripening")}
        success = eng.zeros(1, np.uint8)
        condensation_call(
            eng, formulae=formulae, n_sd=n, n_cell=1,
            cell_start=eng.upload(np.array([0, n], dtype=np.int64)), water_mass=mass,
            v_cr=eng.full(n, np.float64, 1e-15), multiplicity=column(kwargs["multiplicity"]),
            vdry=column(kwargs["dry_volume"]), idx=eng.upload(np.arange(n, dtype=np.int64)),
            rhod=one["rhod"], thd=one["thd"], water_vapour_mixing_ratio=one["qv"], dv=1.0,
            prhod=one["rhod"], pthd=pthd, predicted_water_vapour_mixing_ratio=pqv,
            kappa=column(kwargs["kappa"]), f_org=eng.zeros(n, np.float64), rtol_x=setup.rtol_x,
            rtol_thd=setup.rtol_thd, timestep=ic.DT, counters=counters,
            cell_order=eng.zeros(1, np.int64), RH_max=eng.zeros(1, np.float64), success=success,
            reynolds_number=None, air_density=None, air_dynamic_viscosity=None,
            dt_range=(1e-4, ic.DT), adaptive=False, fuse=setup.fuse, multiplier=setup.multiplier,
            RH_rtol=setup.RH_rtol, max_iters=setup.max_iters)
        assert eng.download(success)[0] == 1
        results.append((eng.download(mass), eng.download(pthd), eng.download(pqv)))
    (with_ice, thd_a, qv_a), (without, thd_b, qv_b) = results
    liquid = mass_all > 0
    assert np.array_equal(pc.bits(with_ice[liquid]), pc.bits(without))
    assert np.array_equal(pc.bits(with_ice[~liquid]), pc.bits(mass_all[~liquid]))
    assert (with_ice[liquid] != mass_all[liquid]).any()
    assert np.array_equal(pc.bits(thd_a), pc.bits(thd_b)) and np.array_equal(pc.bits(qv_a),
                                                                             pc.bits(qv_b))

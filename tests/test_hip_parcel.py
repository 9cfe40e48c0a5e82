"""The adiabatic parcel on the GPU (include/sdm_parcel.h; k_parcel and k_parcel_f): every
comparison is HIP against the CPU checker (tests/parcel_checker/) or HIP against HIP, bit for bit,
viewed as uint8.  No test provokes a fault: the failure case is a solver that reports
success = 0, which the kernel handles without trapping."""
import os

import numpy as np
import pytest

from tests import parcel_cases as pc

pytestmark = pytest.mark.gpu


def _checker():
    from tests.parcel_checker import ParcelCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelCheckerEngine.get()


def _run(engine, kind, kwargs, route, steps, **more):
    runner = pc.runner(engine, kind, kwargs, route, **more)
    profile = runner.run(steps)
    return runner.snapshot(), profile


@pytest.mark.parametrize("adaptive", (True, False), ids=("adaptive", "fixed"))
@pytest.mark.parametrize("kind", ("default", "lowe2019"))
def test_hip_fused_equals_the_checker_and_the_stage_route(hip_engine, kind, adaptive):
    """parcels of 1 .. 2100 rows (lane, wave and register-chunk edges), differing in T0, p0, qv0
    and mass_of_dry_air, updrafts of both signs, 6 steps"""
    kwargs = pc.ensemble(f_org=kind != "default")
    fused = _run(hip_engine, kind, kwargs, "fused", 6, adaptive=adaptive)
    assert (fused[0]["failed_step"] == -1).all() and (fused[0]["steps_done"] == 6).all()
    assert fused[1]["n_activating"].max() > 0 and fused[1]["n_deactivating"].max() > 0
    for what, other in (("checker", _run(_checker(), kind, kwargs, "fused", 6, adaptive=adaptive)),
                        ("stages", _run(hip_engine, kind, kwargs, "stages", 6,
                                        adaptive=adaptive))):
        pc.assert_same_bits(fused[0], other[0], f"state, fused HIP vs {what}")
        pc.assert_same_bits(fused[1], other[1], f"profile, fused HIP vs {what}")


def test_hip_default_descriptor_through_the_general_kernel(hip_engine):
    """both instantiations: PySDM's defaults through k_parcel_f must equal k_parcel"""
    kwargs = pc.ensemble((1, 65, 257, 1100), seed=11)
    default = _run(hip_engine, "default", kwargs, "fused", 4)
    general = _run(hip_engine, "default", kwargs, "fused", 4, general=True)
    pc.assert_same_bits(default[0], general[0], "state")
    pc.assert_same_bits(default[1], general[1], "profile")


def test_hip_chunking_and_resumption(hip_engine):
    """9 steps in launches of 4, 9 and 1 steps, as run(4); run(5), and as nine run(1): identical,
    profile rows included"""
    kwargs = pc.ensemble((3, 65, 300, 1100), seed=13)

    def rows(parts):
        return {key: np.concatenate([part[key] for part in parts]) for key in parts[0]}

    ref = _run(hip_engine, "default", kwargs, "fused", 9, steps_per_launch=4)
    for spl in (9, 1):
        other = _run(hip_engine, "default", kwargs, "fused", 9, steps_per_launch=spl)
        pc.assert_same_bits(ref[0], other[0], f"state, steps_per_launch={spl}")
        pc.assert_same_bits(ref[1], other[1], f"profile, steps_per_launch={spl}")
    for split in ((4, 5), (1,) * 9):
        runner = pc.runner(hip_engine, "default", kwargs, "fused")
        parts = [runner.run(n) for n in split]
        pc.assert_same_bits(ref[0], runner.snapshot(), f"state, runs of {split}")
        pc.assert_same_bits(ref[1], rows(parts), f"profile, runs of {split}")


def test_hip_more_parcels_than_workgroups_in_flight(hip_engine):
    """one parcel per workgroup across more parcels than the card holds at once: 1030 parcels of
    8 rows, 3 steps (indexing by block past the first wave of workgroups)"""
    kwargs = pc.ensemble((8,) * 1030, seed=17)
    hip = _run(hip_engine, "default", kwargs, "fused", 3)
    assert (hip[0]["steps_done"] == 3).all()
    ref = _run(_checker(), "default", kwargs, "fused", 3)
    pc.assert_same_bits(hip[0], ref[0], "state")
    pc.assert_same_bits(hip[1], ref[1], "profile")


@pytest.mark.parametrize("kind,setup,sizes,seed", pc.FAILURE_CASES, ids=pc.FAILURE_IDS)
def test_hip_failed_parcels_stop_and_the_context_stays_usable(hip_engine, kind, setup, sizes,
                                                              seed):
    """a solver that gives up (max_iters too small) in some parcels: they stop with their state as
    before the step, the others go on; HIP == checker; a small good run follows"""
    kwargs = pc.ensemble(sizes, seed=seed, f_org=kind != "default")
    states = []
    for engine, route in ((hip_engine, "fused"), (_checker(), "fused"), (hip_engine, "stages")):
        runner = pc.runner(engine, kind, kwargs, route, setup=setup)
        with pytest.raises(RuntimeError, match="Condensation failed"):
            runner.run(5)
        states.append((runner.snapshot(), runner.last_profile))
    for other, what in ((states[1], "checker"), (states[2], "stage route on HIP")):
        pc.assert_same_bits(states[0][0], other[0], f"state, fused HIP vs {what}")
        pc.assert_same_bits(states[0][1], other[1], f"profile, fused HIP vs {what}")
    failed = states[0][0]["failed_step"]
    assert (failed >= 0).any() and (failed == -1).any()
    assert (states[0][0]["steps_done"][failed == -1] == 5).all()
    # the context is usable afterwards
    good = _run(hip_engine, "default", pc.ensemble((10, 20), seed=6), "fused", 2)
    assert (good[0]["failed_step"] == -1).all() and (good[0]["steps_done"] == 2).all()


@pytest.mark.parametrize("run", "abc")
def test_hip_recorded_ascents_against_the_reference(hip_engine, run):
    """the three runs of tests/golden/parcel_runs.npz on the GPU: within the bounds of the CPU
    suite's free-run test against the reference, and bit for bit what the checker computes"""
    from tests.test_parcel_checker import assert_matches_the_reference  # pylint: disable=import-outside-toplevel

    runs = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                "parcel_runs.npz"))
    n_steps = int(runs[f"{run}/cfg/n_steps"])
    results = []
    for engine in (hip_engine, _checker()):
        runner = pc.golden_runner(engine, runs, run, "fused")
        profile = runner.run(n_steps)
        results.append((runner.snapshot(), profile))
    assert results[0][0]["failed_step"].tolist() == [-1]
    assert_matches_the_reference(runs, run, results[0][1], results[0][0]["water_mass"])
    pc.assert_same_bits(results[0][0], results[1][0], "state")
    pc.assert_same_bits(results[0][1], results[1][1], "profile")

"""The parcel's diagnostics on the GPU (include/sdm_parcel_diag.h; k_parcel_d, k_parcel_f_d,
k_parcel_diagnose, k_parcel_diagnose_f): every comparison is HIP against the CPU checker
(tests/parcel_diag_checker/) or HIP against HIP, bit for bit, viewed as uint8.  No test provokes
a fault: the failure case is a solver that reports success = 0, which the kernels handle without
trapping."""
import os

import numpy as np
import pytest

from tests import parcel_cases as pc
from tests import parcel_products_cases as ppc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _checker():
    from tests.parcel_diag_checker import ParcelDiagCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelDiagCheckerEngine.get()


@pytest.mark.parametrize("kind", ("default", "lowe2019"))
def test_hip_equals_the_checker_every_output(hip_engine, kind):
    """parcels of 1 .. 2049 rows in one call (lane, wave and register-cache edges, rows past the
    cache), 3 steps, 16 moment requests (one selecting nothing) and a 256-bin spectrum: the fused
    rows, dv, the profile and the state, and `diagnose` of the final state; both instantiations"""
    kwargs = pc.ensemble(ppc.EDGE_SIZES, seed=21, f_org=kind != "default")
    results = []
    for engine in (hip_engine, _checker()):
        runner = pc.runner(engine, kind, kwargs, "fused")
        table = ppc.full_table(runner.formulae)
        profile, rows = ppc.run_with_table(runner, table, (3,))
        runner.diagnose(table)
        results.append((runner.snapshot(), profile, rows, ppc.raw(runner.last_rows, dv=False)))
    hip, ref = results
    assert (hip[0]["failed_step"] == -1).all() and (hip[0]["steps_done"] == 3).all()
    for at, what in enumerate(("state", "profile", "fused rows", "diagnose rows")):
        pc.assert_same_bits(hip[at], ref[at], f"{kind}: {what}, HIP vs checker")
    rows = hip[2]
    assert (rows["moment_0"][..., 15] == 0).all() and (rows["moments"][..., 15] == 0).all()
    assert (rows["moment_0"][:, -1, :10] > 0).all() and rows["spectrum"].sum() > 0  # (2049 rows)
    # the fused rows of the last step are the diagnose rows of the final state
    for key in ("moment_0", "moments", "spectrum"):
        assert np.array_equal(pc.bits(rows[key][-1]), pc.bits(hip[3][key])), key


def test_hip_default_descriptor_through_the_general_kernels(hip_engine):
    """PySDM's defaults through k_parcel_f_d / k_parcel_diagnose_f must equal k_parcel_d /
    k_parcel_diagnose"""
    kwargs = pc.ensemble((1, 65, 257, 1100), seed=11)
    results = []
    for general in (False, True):
        runner = pc.runner(hip_engine, "default", kwargs, "fused", general=general)
        table = ppc.full_table(runner.formulae)
        _, rows = ppc.run_with_table(runner, table, (3,))
        runner.diagnose(table)
        results.append((rows, ppc.raw(runner.last_rows, dv=False)))
    pc.assert_same_bits(results[0][0], results[1][0], "fused rows")
    pc.assert_same_bits(results[0][1], results[1][1], "diagnose rows")


def test_hip_more_parcels_than_workgroups_in_flight(hip_engine):
    """1030 parcels of 2 to 5 rows, 2 steps: the fused rows equal `diagnose` of the state after
    each step (one workgroup per parcel past the first wave of workgroups, in both kernels)"""
    sizes = tuple(2 + (c % 4) for c in range(1030))
    kwargs = pc.ensemble(sizes, seed=17)
    fused = pc.runner(hip_engine, "default", kwargs, "fused")
    table = ppc.full_table(fused.formulae)
    _, rows = ppc.run_with_table(fused, table, (2,))
    assert (fused.snapshot()["steps_done"] == 2).all()
    staged = ppc.diagnose_after_each_step(pc.runner(hip_engine, "default", kwargs, "fused"),
                                          table, 2)
    rows.pop("dv")
    pc.assert_same_bits(rows, staged, "fused rows vs diagnose after each step")


def test_hip_launch_edges_and_resumption(hip_engine):
    """9 steps in launches of 4: run(9) == run(4); run(5), rows included, and == the checker"""
    kwargs = pc.ensemble((3, 65, 300, 1100), seed=13)
    results = []
    for engine, splits in ((hip_engine, (9,)), (hip_engine, (4, 5)), (_checker(), (9,))):
        runner = pc.runner(engine, "default", kwargs, "fused", steps_per_launch=4)
        table = ppc.full_table(runner.formulae)
        results.append((*ppc.run_with_table(runner, table, splits), runner.snapshot()))
    for other, what in ((results[1], "run(4); run(5)"), (results[2], "the checker")):
        pc.assert_same_bits(results[0][0], other[0], f"profile, run(9) vs {what}")
        pc.assert_same_bits(results[0][1], other[1], f"rows, run(9) vs {what}")
        pc.assert_same_bits(results[0][2], other[2], f"state, run(9) vs {what}")


def test_hip_a_failing_parcel_leaves_its_rows_untouched(hip_engine):
    """a solver that gives up in some parcels (max_iters too small): the rows of the steps they
    did not carry out keep the sentinel the outputs were prefilled with, the other parcels'
    rows are unaffected; HIP == checker"""
    kind, setup, sizes, seed = pc.FAILURE_CASES[2]
    kwargs = pc.ensemble(sizes, seed=seed)
    sentinel = -7.25
    results = []
    for engine in (hip_engine, _checker()):
        runner = pc.runner(engine, kind, kwargs, "fused", setup=setup)
        runner.diag_fill = sentinel
        table = ppc.full_table(runner.formulae)
        with pytest.raises(RuntimeError, match="Condensation failed"):
            runner.run(5, products=table)
        results.append((runner.snapshot(), ppc.raw(runner.last_rows)))
    pc.assert_same_bits(results[0][0], results[1][0], "state")
    pc.assert_same_bits(results[0][1], results[1][1], "rows")
    state, rows = results[0]
    failed, done = state["failed_step"], state["steps_done"]
    assert (failed >= 0).any() and (failed == -1).any()
    for c in range(len(sizes)):
        for key, value in rows.items():
            assert (value[done[c]:, c] == sentinel).all(), (key, c)
            assert (value[:done[c], c] != sentinel).all(), (key, c)
    # the parcels that went on are what they are without the failing ones beside them
    good = np.flatnonzero(failed == -1)
    alone = pc.runner(hip_engine, kind, {
        **kwargs, "counts": np.asarray(sizes)[good],
        **{k: np.concatenate([np.split(np.asarray(kwargs[k]), np.cumsum(sizes)[:-1])[c]
                              for c in good])
           for k in ("multiplicity", "water_mass", "dry_volume", "kappa")},
        **{k: np.asarray(kwargs[k])[good] for k in ("T0", "p0", "RH0", "w", "mass_of_dry_air",
                                                    "z0")}}, "fused", setup=setup)
    _, rows_alone = ppc.run_with_table(alone, ppc.full_table(alone.formulae), (5,))
    pc.assert_same_bits({k: np.ascontiguousarray(v[:, good]) for k, v in rows.items()},
                        rows_alone, "the parcels that went on")


def test_hip_recorded_steps_of_run_c_through_the_general_kernel(hip_engine):
    """the recorded steps of run `c` (Lowe-2019) of tests/golden/parcel_products.npz: the
    reference's own products from the recorded masses, on the GPU"""
    from tests.test_parcel_products_checker import assert_products_match_the_reference  # pylint: disable=import-outside-toplevel

    data = np.load(os.path.join(HERE, "golden", "parcel_products.npz"))
    assert_products_match_the_reference(hip_engine, data, "c")

"""The parcel with aqueous chemistry on the GPU (include/sdm_parcel_chem.h; k_parcel_chem after
one-step launches of k_parcel / k_parcel_f): every comparison is HIP against the CPU checker
(tests/parcel_chem_checker/) or HIP against HIP, bit for bit, viewed as uint8.  No test provokes a
fault: the failure cases are solvers that report success = 0, which the kernels handle without
trapping."""
import numpy as np
import pytest

from pysdm_amd.formulae import Formulae
from tests import parcel_cases as pc
from tests import parcel_chem_cases as cc
from tests import parcel_products_cases as ppc

pytestmark = pytest.mark.gpu

# rows per parcel: lane, wave, register-resident (256) and COND_CH (1024) edges
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
GRID_CAP = 1024  # SDM_PARCEL_CHEM_MAX_GRID


def _checker():
    from tests.parcel_chem_checker import ParcelChemCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelChemCheckerEngine.get()


def test_the_grid_cap_is_the_headers():
    import os  # pylint: disable=import-outside-toplevel
    import re  # pylint: disable=import-outside-toplevel

    from pysdm_amd import abi  # pylint: disable=import-outside-toplevel

    with open(abi.PARCEL_CHEM_HEADER_PATH, encoding="utf-8") as header:
        found = re.search(r"#define SDM_PARCEL_CHEM_MAX_GRID (\d+)", header.read())
    assert os.path.exists(abi.PARCEL_CHEM_HEADER_PATH) and int(found.group(1)) == GRID_CAP


@pytest.mark.parametrize("kind", ("default", "general"))
@pytest.mark.parametrize("sum_mode", ("ordered", "blocked"))
@pytest.mark.parametrize("system", ("open", "closed"))
def test_hip_equals_the_checker_at_the_edges(hip_engine, system, sum_mode, kind):
    """eight parcels of 1 .. 1025 rows, half of the rows flagged, three sub-steps, three steps;
    both instantiations of the condensation solver"""
    kwargs = cc.ensemble(EDGE_SIZES, seed=7)
    more = dict(system=system, sum_mode=sum_mode, n_substep=3)
    hip = cc.run(hip_engine, kind, kwargs, "fused", 3, **more)
    assert (hip[0]["failed_step"] == -1).all() and (hip[0]["steps_done"] == 3).all()
    assert hip[2]["n_flagged"][-1, 1:].min() > 0
    cc.assert_same_run(hip, cc.run(_checker(), kind, kwargs, "fused", 3, **more),
                       "fused HIP vs checker")


@pytest.mark.parametrize("sizes,system,sum_mode,n_substep", (
    ((257,), "closed", "blocked", 1), ((65, 256, 1025), "closed", "ordered", 3),
    ((64, 255, 600), "open", "ordered", 1)), ids=("one-parcel", "three-parcels", "open"))
def test_hip_equals_its_stage_route(hip_engine, sizes, system, sum_mode, n_substep):
    """1 and 3 parcels, n_substep 1 and 3: `sdm_parcel_run_chem` against the stage step followed
    by `sdm_chemistry_step` on the parcel's slice and the two element-wise updates, on the GPU"""
    kwargs = cc.ensemble(sizes, seed=11)
    more = dict(system=system, sum_mode=sum_mode, n_substep=n_substep)
    fused = cc.run(hip_engine, "default", kwargs, "fused", 3, **more)
    cc.assert_same_run(fused, cc.run(hip_engine, "default", kwargs, "stages", 3, **more),
                       "fused vs stages on HIP")
    cc.assert_same_run(fused, cc.run(_checker(), "default", kwargs, "fused", 3, **more),
                       "fused HIP vs checker")


def test_hip_default_formulae_through_the_general_kernel(hip_engine):
    kwargs = cc.ensemble((1, 65, 257), seed=11)
    default = cc.run(hip_engine, "default", kwargs, "fused", 3, n_substep=2)
    general = cc.run(hip_engine, "default", kwargs, "fused", 3, n_substep=2, general=True)
    cc.assert_same_run(default, general, "k_parcel vs k_parcel_f")


def test_hip_more_parcels_than_the_grid_cap(hip_engine):
    """cap + 6 parcels of 2 .. 5 rows, 2 steps: the workgroups stride over the parcels"""
    sizes = tuple(2 + (c % 4) for c in range(GRID_CAP + 6))
    kwargs = cc.ensemble(sizes, seed=17)
    hip = cc.run(hip_engine, "default", kwargs, "fused", 2, system="closed")
    assert (hip[0]["steps_done"] == 2).all()
    assert hip[2]["n_flagged"][-1, GRID_CAP:].max() > 0  # the chemistry ran past the cap
    cc.assert_same_run(hip, cc.run(_checker(), "default", kwargs, "fused", 2, system="closed"),
                       "fused HIP vs checker")


def test_hip_a_closed_parcel_without_a_flagged_row_keeps_its_mixing_ratios(hip_engine):
    """haze only (tests/parcel_cases.py's ensemble: no row dilute enough) beside a parcel with
    flagged rows"""
    haze, mixed = pc.ensemble((40,), seed=5), cc.ensemble((40,), seed=5)
    kwargs = {key: (value if key == "dt" else None if value is None else
                    np.concatenate([np.atleast_1d(value), np.atleast_1d(mixed[key])]))
              for key, value in haze.items()}
    runner = cc.runner(hip_engine, "default", kwargs, "fused", system="closed", n_substep=3)
    start = runner.snapshot()
    _, record = runner.run(3)
    end = runner.snapshot()
    assert record["n_flagged"][:, 0].tolist() == [0, 0, 0] and record["n_flagged"][-1, 1] > 0
    for gas in cc.GASES:
        key = f"mixing_ratio_{gas}"
        assert np.array_equal(pc.bits(end[key][:1]), pc.bits(start[key][:1])), gas
    assert end["mixing_ratio_SO2"][1] < start["mixing_ratio_SO2"][1]
    checker = cc.runner(_checker(), "default", kwargs, "fused", system="closed", n_substep=3)
    checker.run(3)
    pc.assert_same_bits(end, checker.snapshot(), "state, fused HIP vs checker")


@pytest.mark.parametrize("case,seed", cc.FAILURE_CASES, ids=cc.FAILURE_IDS)
def test_hip_a_failed_parcel_among_good_ones(hip_engine, case, seed):
    """a solver that gives up (max_iters too small) in some parcels, at the first step and at a
    later one: five steps (ten launches) and two more; HIP == checker == stage route on HIP"""
    kind, setup, sizes, _ = pc.FAILURE_CASES[case]
    kwargs = cc.ensemble(sizes, seed=seed)
    more = dict(system="closed", n_substep=2, setup=setup)
    results = []
    for engine, route in ((hip_engine, "fused"), (_checker(), "fused"), (hip_engine, "stages")):
        runner = cc.runner(engine, kind, kwargs, route, **more)
        with pytest.raises(RuntimeError, match="Condensation failed"):
            runner.run(5)
        first = (runner.snapshot(), runner.last_profile, runner.last_chem_profile)
        try:
            runner.run(2)
        except RuntimeError:
            pass
        results.append((*first, runner.snapshot(), runner.last_profile,
                        runner.last_chem_profile))
    failed = results[0][0]["failed_step"]
    assert (failed >= 0).any() and (failed == -1).any()
    for other, what in ((results[1], "checker"), (results[2], "stage route on HIP")):
        for a, b in zip(results[0], other):
            pc.assert_same_bits(a, b, f"fused HIP vs {what}")


def test_hip_continuation(hip_engine):
    """run(9) == run(4); run(5) == nine run(1)"""
    kwargs = cc.ensemble((3, 65, 300), seed=13)
    more = dict(system="closed", sum_mode="blocked", n_substep=2)
    whole = cc.run(hip_engine, "default", kwargs, "fused", 9, **more)
    for split in ((4, 5), (1,) * 9):
        runner = cc.runner(hip_engine, "default", kwargs, "fused", **more)
        parts = [runner.run(n) for n in split]
        pc.assert_same_bits(whole[0], runner.snapshot(), f"state, {split}")
        pc.assert_same_bits(whole[1], cc.concatenated([p[0] for p in parts]), f"profile, {split}")
        pc.assert_same_bits(whole[2], cc.concatenated([p[1] for p in parts]),
                            f"chemistry profile, {split}")


@pytest.mark.parametrize("kind", ("default", "general"))
def test_hip_the_request_table_after_the_chemistry(hip_engine, kind):
    """the sixteen moments and the 256-bin spectrum after every step: HIP == checker, and == the
    stage symbol `sdm_parcel_diagnose` on the state after each step"""
    kwargs = cc.ensemble((5, 257, 1025), seed=4)
    table = ppc.full_table(Formulae())
    more = dict(system="closed", n_substep=2)
    hip = cc.runner(hip_engine, kind, kwargs, "fused", **more)
    _, record, _ = hip.run(3, products=table)
    rows = ppc.raw(hip.last_rows)
    checker = cc.runner(_checker(), kind, kwargs, "fused", **more)
    checker.run(3, products=table)
    pc.assert_same_bits(rows, ppc.raw(checker.last_rows), "rows, fused HIP vs checker")
    pc.assert_same_bits(hip.snapshot(), checker.snapshot(), "state, fused HIP vs checker")
    stepped = cc.runner(hip_engine, kind, kwargs, "fused", **more)
    after = ppc.diagnose_after_each_step(stepped, table, 3)
    for key, value in after.items():
        assert np.array_equal(pc.bits(rows[key]), pc.bits(value)), key
    assert np.array_equal(pc.bits(rows["dv"]), pc.bits(record["dv"]))

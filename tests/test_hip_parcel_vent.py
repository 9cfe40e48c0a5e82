"""The ventilated parcel on the GPU (include/sdm_parcel_vent.h; k_parcel_v and k_parcel_v_d): every
comparison is HIP against the CPU checker (tests/parcel_vent_checker/) or HIP against HIP, bit for
bit.  No test provokes a fault: a radius above the table's top stops its parcel before the table
is read."""
import numpy as np
import pytest

from tests import parcel_cases as pc
from tests import parcel_products_cases as ppc
from tests import parcel_vent_cases as vc

pytestmark = pytest.mark.gpu
PR79 = "PruppacherAndRasmussen1979"


def _checker():
    from tests.parcel_vent_checker import ParcelVentCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelVentCheckerEngine.get()


@pytest.mark.parametrize("direction", ("up", "down"))
@pytest.mark.parametrize("law", vc.LAWS)
@pytest.mark.parametrize("ventilation", vc.VENTILATIONS)
def test_hip_fused_equals_the_checker_and_the_stage_route(hip_engine, ventilation, law, direction):
    """parcels of 1, 255, 256, 257 and 1025 rows, 3 steps, ascending haze and descending drizzle"""
    kwargs = vc.ascending() if direction == "up" else vc.descending()
    fused = vc.run(hip_engine, ventilation, law, kwargs, "fused", 3)
    assert (fused[0]["steps_done"] == 3).all() and (fused[0]["failed_step"] == -1).all()
    for what, other in (("checker", vc.run(_checker(), ventilation, law, kwargs, "fused", 3)),
                        ("stages", vc.run(hip_engine, ventilation, law, kwargs, "stages", 3))):
        pc.assert_same_bits(fused[0], other[0], f"state, fused HIP vs {what}")
        pc.assert_same_bits(fused[1], other[1], f"profile, fused HIP vs {what}")


def test_hip_more_parcels_than_workgroups_in_flight(hip_engine):
    """1030 parcels of 3 rows, 2 steps: more parcels than resident workgroups"""
    kwargs = vc.descending((3,) * 1030, seed=17)
    hip = vc.run(hip_engine, PR79, "GunnKinzer1949", kwargs, "fused", 2)
    assert (hip[0]["steps_done"] == 2).all()
    ref = vc.run(_checker(), PR79, "GunnKinzer1949", kwargs, "fused", 2)
    pc.assert_same_bits(hip[0], ref[0], "state")
    pc.assert_same_bits(hip[1], ref[1], "profile")


def test_hip_continuation(hip_engine):
    """run(5) in launches of 2 steps == five run(1) == run(2); run(3), and == the checker"""
    kwargs = vc.descending((3, 257, 40), seed=21)
    rows = lambda parts: {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}  # noqa: E731
    ref = vc.run(hip_engine, PR79, "PowerSeries", kwargs, "fused", 5, steps_per_launch=2)
    assert (ref[0]["steps_done"] == 5).all()
    for split in ((1,) * 5, (2, 3)):
        runner = vc.runner(hip_engine, PR79, "PowerSeries", kwargs, "fused")
        parts = [runner.run(n) for n in split]
        pc.assert_same_bits(ref[0], runner.snapshot(), f"state, runs of {split}")
        pc.assert_same_bits(ref[1], rows(parts), f"profile, runs of {split}")
    checker = vc.run(_checker(), PR79, "PowerSeries", kwargs, "fused", 5)
    pc.assert_same_bits(ref[0], checker[0], "state, HIP vs checker")


def test_hip_a_radius_above_the_table_stops_its_parcel_only(hip_engine):
    """a 7 mm row in the second of three parcels at the second step: that parcel keeps its state,
    the neighbours go on; HIP == checker"""
    kwargs = vc.descending((20, 300, 9), seed=27)
    states = []
    for engine in (hip_engine, _checker()):
        runner = vc.runner(engine, PR79, "GunnKinzer1949", kwargs, "fused")
        runner.run(1)
        mass = runner.snapshot()["water_mass"]
        mass[20 + 260] = vc.RHO_W * 4 / 3 * np.pi * 7e-3 ** 3
        runner.restore({"water_mass": mass})
        with pytest.raises(ValueError, match=r"Radii can be interpolated up to 0\.006"):
            runner.run(2)
        states.append((runner.snapshot(), runner.last_profile))
    assert states[0][0]["out_of_table"].tolist() == [0, 1, 0]
    assert states[0][0]["steps_done"].tolist() == [3, 1, 3]
    pc.assert_same_bits(states[0][0], states[1][0], "state, HIP vs checker")
    pc.assert_same_bits(states[0][1], states[1][1], "profile, HIP vs checker")


def test_hip_products(hip_engine):
    """the request table inside k_parcel_v_d == the stage route's diagnose after each step"""
    kwargs = vc.descending((1, 257, 1025), seed=28)
    formulae, _ = vc.formulae_of(PR79)
    table = ppc.full_table(formulae)
    fused = vc.runner(hip_engine, PR79, "GunnKinzer1949", kwargs, "fused", steps_per_launch=2)
    _, rows = ppc.run_with_table(fused, table, (3,))
    stages = vc.runner(hip_engine, PR79, "GunnKinzer1949", kwargs, "stages")
    expected = ppc.diagnose_after_each_step(stages, table, 3)
    for key, value in expected.items():
        assert np.array_equal(pc.bits(rows[key]), pc.bits(value)), key
    pc.assert_same_bits(fused.snapshot(), stages.snapshot(), "state")
    checker = vc.runner(_checker(), PR79, "GunnKinzer1949", kwargs, "fused")
    _, rows_checker = ppc.run_with_table(checker, table, (3,))
    pc.assert_same_bits(rows, rows_checker, "rows, HIP vs checker")

"""The parcel with coalescence on the GPU (include/sdm_parcel_coal.h; k_parcel_p / k_parcel_f_p and
k_parcel_coal): the checks of tests/test_parcel_coal_checker.py repeated on the HIP engine - the
fused call against the stage route (the existing stage step, then `sdm_collision_step` with
n_cell = 1), HIP against HIP - and the HIP fused route against the CPU checker's, bit for bit.
No test provokes a fault: every shape is within the kernel's documented limits."""
import numpy as np
import pytest

from tests import parcel_cases as pc
from tests import parcel_coal_cases as cc
from tests import test_parcel_coal_checker as cpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel

    return HipEngine.get()


@pytest.fixture(scope="module")
def checker():
    from tests.parcel_coal_checker import ParcelCoalCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelCoalCheckerEngine.get()


# ---- 1. fused == stage route -------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", (True, False), ids=("adaptive", "substeps3"))
@pytest.mark.parametrize("kernel", ("constant", "golovin", "geometric"))
def test_fused_equals_the_stage_route(engine, kernel, adaptive):
    fused = cpu.check_fused_equals_stages(engine, kernel, adaptive)
    if adaptive:
        assert fused[2]["n_substeps"].max() > 1
    else:
        assert (fused[2]["n_substeps"][:, 1:] == 3).all()


@pytest.mark.parametrize("law", ("RogersYau", "PowerSeries"))
def test_fused_equals_the_stage_route_with_the_closed_form_velocity_laws(engine, law):
    """the Geometric kernel with the two laws the CPU oracle lacks (the table is the default)"""
    cpu.check_fused_equals_stages(engine, "geometric", True, law=law, steps=4)


def test_fused_equals_the_stage_route_with_the_electric_kernel(engine):
    cpu.check_fused_equals_stages(engine, "electric", True, steps=2)


def test_fused_equals_the_stage_route_with_other_formulae(engine):
    cpu.check_fused_equals_stages(engine, "constant", True, kind="general", steps=4)


@pytest.mark.parametrize("kernel,adaptive", (("constant", True), ("golovin", False),
                                             ("geometric", True)))
def test_hip_fused_equals_the_checkers_fused_route(engine, checker, kernel, adaptive):
    """the same call on the two implementations of the header"""
    kwargs = cc.ensemble(seed=3)
    more = dict(collisions=cc.setup_of(kernel, adaptive=adaptive, substeps=3),
                seed=np.arange(len(cc.SIZES)) + 11)
    hip = cc.run(engine, "default", kwargs, "fused", 5, **more)
    ref = cc.run(checker, "default", kwargs, "fused", 5, **more)
    cc.assert_same_run(hip, ref, f"{kernel}: HIP vs checker")
    assert hip[0]["coalescence_rate"].sum() > 0


# ---- 2. order ----------------------------------------------------------------------------------------
def test_the_sums_follow_the_permutation(engine, checker):
    cpu.check_order_is_followed(engine, checker)


# ---- 3. continuation -------------------------------------------------------------------------------
def test_continuation(engine):
    cpu.check_continuation(engine)


# ---- 4. independence and seeds ---------------------------------------------------------------------
def test_a_parcel_of_an_ensemble_equals_its_solo_run(engine):
    cpu.check_independence(engine)


def test_equal_seeds_stay_equal_and_different_seeds_differ(engine):
    cpu.check_seeds(engine)


# ---- 5. edges ----------------------------------------------------------------------------------------
def test_the_largest_parcel_and_one_row_more(engine):
    cpu.check_the_largest_parcel(engine)


def test_more_parcels_than_the_grid_cap(engine):
    cpu.check_more_parcels_than_the_grid_cap(engine)


def test_all_rows_but_one_die(engine):
    cpu.check_all_rows_but_one_die(engine)


@pytest.mark.parametrize("case", range(len(pc.FAILURE_CASES)), ids=pc.FAILURE_IDS)
def test_a_failed_parcel_keeps_everything_and_the_others_go_on(engine, case):
    cpu.check_a_failed_parcel(engine, case)


def test_dt_min_is_reached_flagged_and_warned_about(engine):
    cpu.check_dt_min_is_reached(engine)


# ---- 6. conservation -------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ("fused", "stages"))
def test_dry_volume_and_hygroscopicity_are_conserved(engine, route):
    cpu.check_conservation(engine, route)


# ---- the rest of the CPU checks, on the HIP engine ---------------------------------------------------
def test_snapshot_and_restore_carry_the_new_arrays(engine):
    cpu.test_snapshot_and_restore_carry_the_new_arrays(engine)


def test_kappa_follows_the_collisions(engine):
    cpu.test_kappa_follows_the_collisions(engine)


def test_diagnose_sees_the_live_rows_in_position_order(engine):
    cpu.test_diagnose_sees_the_live_rows_in_position_order(engine)


def test_refusals_by_name(engine):
    """the host layer's refusals and the library's own (its argument checks name the member;
    nothing is launched)"""
    cpu.test_refusals_by_name(engine)

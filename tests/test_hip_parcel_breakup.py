"""The parcel with collisional breakup on the GPU (include/sdm_parcel_breakup.h; the BREAKUP
instantiations of k_parcel_coal): the checks of tests/test_parcel_breakup_checker.py repeated on
the HIP engine - the fused call against the stage route (`sdm_collision_step` with n_cell = 1 and
breakup), HIP against HIP - and the HIP fused route against the CPU checker's, bit for bit.
No test provokes a fault: every shape is within the kernel's documented limits."""
import warnings

import numpy as np
import pytest

from tests import parcel_breakup_cases as bc
from tests import test_parcel_breakup_checker as cpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel

    return HipEngine.get()


@pytest.fixture(scope="module")
def checker():
    from tests.parcel_breakup_checker import ParcelBreakupCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelBreakupCheckerEngine.get()


# ---- 1. fused == stage route -------------------------------------------------------------------------
@pytest.mark.parametrize("frag", list(bc.FRAGMENTATIONS))
def test_fused_equals_the_stage_route_for_every_fragmentation(engine, frag):
    cpu.test_fused_equals_the_stage_route_for_every_fragmentation(engine, frag)


@pytest.mark.parametrize("ec", list(bc.EFFICIENCIES))
def test_fused_equals_the_stage_route_for_every_efficiency(engine, ec):
    cpu.test_fused_equals_the_stage_route_for_every_efficiency(engine, ec)


@pytest.mark.parametrize("adaptive", (True, False), ids=("adaptive", "substeps3"))
@pytest.mark.parametrize("handle_all", (False, True), ids=("first_breakup", "all_breakups"))
def test_fused_equals_the_stage_route_with_and_without_handle_all_breakups(engine, handle_all,
                                                                          adaptive):
    cpu.test_fused_equals_the_stage_route_with_and_without_handle_all_breakups(
        engine, handle_all, adaptive)


@pytest.mark.parametrize("law", ("RogersYau", "PowerSeries"))
def test_fused_equals_the_stage_route_with_the_closed_form_velocity_laws(engine, law):
    """Straub's fragmentation over the Geometric kernel with the two laws the CPU oracle lacks"""
    kwargs = bc.ensemble((3, 65, 257), seed=3)
    more = dict(seed=(5, 6, 7), terminal_velocity=law)
    fused = bc.run(engine, kwargs, "fused", 3, bc.breakup_setup("straub2010"), **more)
    stages = bc.run(engine, kwargs, "stages", 3, bc.breakup_setup("straub2010"), **more)
    bc.assert_same_run(fused, stages, f"{law}: fused vs stages")
    assert fused[0]["breakup_rate"].sum() > 0


def test_the_largest_parcel_and_one_row_more(engine):
    cpu.check_the_largest_parcel(engine)


# ---- 2. HIP fused == the checker's fused ---------------------------------------------------------------
SETUPS = {
    "collision": lambda: bc.collision_setup(),
    "breakup_straub_substeps3": lambda: bc.breakup_setup("straub2010", adaptive=False, substeps=3),
    "collision_lowlist_all_breakups": lambda: bc.collision_setup(
        frag="exponential", ec="lowlist1982", handle_all_breakups=True),
}


@pytest.mark.parametrize("name", list(SETUPS))
def test_hip_fused_equals_the_checkers_fused_route(engine, checker, name):
    """the same call on the two implementations of the header"""
    kwargs = bc.ensemble(seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hip = bc.run(engine, kwargs, "fused", 3, SETUPS[name](), seed=cpu.SEEDS)
        ref = bc.run(checker, kwargs, "fused", 3, SETUPS[name](), seed=cpu.SEEDS)
    bc.assert_same_run(hip, ref, f"{name}: HIP vs checker")
    assert hip[0]["breakup_rate"].sum() > 0


# ---- 3. shared edge cases ----------------------------------------------------------------------------
def test_continuation(engine):
    cpu.check_continuation(engine)


def test_snapshot_and_restore_carry_the_breakup_arrays(engine):
    cpu.test_snapshot_and_restore_carry_the_breakup_arrays(engine)


def test_a_parcel_of_an_ensemble_equals_its_solo_run(engine):
    cpu.check_independence(engine)


def test_more_parcels_than_the_grid_cap(engine):
    cpu.check_more_parcels_than_the_grid_cap(engine)


def test_a_failed_parcel_keeps_everything_the_breakup_arrays_included(engine):
    cpu.check_a_failed_parcel(engine)


# ---- 4. - 7. -------------------------------------------------------------------------------------------
def test_overflows_are_counted_recorded_and_warned_about(engine):
    cpu.check_overflow(engine)
    cpu.check_events_carry_the_overflow_count(engine)


def test_the_extensive_sums_are_conserved_by_every_collision_step(engine):
    cpu.check_conservation(engine)


def test_coalescence_through_the_new_symbol_equals_the_old_one(engine):
    cpu.check_coalescence_through_the_new_symbol(engine)


def test_refusals_by_name(engine):
    """the host layer's refusals and the library's own (its argument checks name the member;
    nothing is launched)"""
    cpu.check_refusals(engine)

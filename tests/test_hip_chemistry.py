"""Aqueous chemistry on the MI355X: include/sdm_chemistry.h through libsdm_hip.so.

Every comparison is HIP against the CPU checker, bit for bit: the five stage symbols on the
recorded inputs of chem_methods.npz, the fused step against the checker's literal stage sequence,
and the three event counts.  The shapes are the smallest at which the kernels can still go wrong:
1 to 3000 rows (one lane, one row short of / one row over a workgroup of 256, several workgroups),
1 / 3 / 7 / 300 cells (more cells than one workgroup of the per-cell kernel has lanes), cells with
0, 1, 255, 256, 257, 513, 1024 and 3000 flagged rows mixed with unflagged ones (the block edges of
the blocked sum, whose compaction then crosses the 256-position chunks of the walk), open and
closed systems, 1 to 3 sub-steps, both sum shapes.  Then the goldens with the CPU bounds, `step()`
against `step_by_stages()` on the device, and run-to-run equality of the blocked sum."""
import numpy as np
import pytest

from pysdm_amd import chemistry as chem
from tests import chemistry_cases as cc
from tests.test_chemistry_checker import CONSTS, LIMITS, METHODS, STEPS

pytestmark = pytest.mark.gpu
SUMS = ("ordered", "blocked")


@pytest.fixture(scope="module", name="checker")
def checker_engine():
    from tests.chemistry_checker import ChemistryCheckerEngine  # pylint: disable=import-outside-toplevel

    return ChemistryCheckerEngine.get()


def same(got, want, what):
    for at, (a, b) in enumerate(zip(got, want)):
        if isinstance(a, np.ndarray):
            cc.assert_same_bits(a, b, f"{what} [{at}]")
        else:
            assert a == b, f"{what} [{at}]"


def test_stage_symbols_equal_the_checker_on_the_recorded_inputs(hip_engine, checker):
    engines = (hip_engine, checker)
    same(*(cc.call_cell_data(e, METHODS["ambient/T"], CONSTS) for e in engines), "cell data")
    for which, start in ((1, (METHODS["eq1/pH_in"], METHODS["eq1/flag_in"])),
                         (2, (METHODS["eq1/pH"], METHODS["eq1/flag"]))):
        same(*(cc.call_equilibrate(e, METHODS["cell_id"], cc.methods_conc(METHODS, which),
                                   METHODS["cell/equilibrium"], *start, LIMITS, CONSTS)
               for e in engines), f"equilibrate_H {which}")
    same(*([cc.call_drop_data(e, METHODS["eq2/pH"], METHODS["cell_id"],
                              METHODS["cell/equilibrium"], CONSTS)] for e in engines), "drop data")
    case = cc.methods_dissolution_case(METHODS)
    for system in ("open", "closed"):
        for sum_mode in SUMS:
            same(*(cc.call_dissolution(e, case, system, sum_mode) for e in engines),
                 f"dissolution {system} {sum_mode}")
    same(*([cc.call_oxidation(e, METHODS["cell_id"], METHODS["eq2/flag"], METHODS["cell/kinetic"],
                              METHODS["cell/equilibrium"], float(METHODS["oxi/dt"]),
                              METHODS["volume"], METHODS["eq2/pH"], METHODS["drop/df"][3],
                              cc.methods_oxidation_in(METHODS), CONSTS)] for e in engines),
         "oxidation")


def test_hip_replays_the_goldens_with_the_cpu_bounds(hip_engine):
    eq, kin, henry = cc.call_cell_data(hip_engine, METHODS["ambient/T"], CONSTS)
    assert max(cc.worst(eq, METHODS["cell/equilibrium"]), cc.worst(kin, METHODS["cell/kinetic"]),
               cc.worst(henry, METHODS["cell/henry"])) <= cc.RTOL_ARITHMETIC
    pH, flag, n_failed = cc.call_equilibrate(
        hip_engine, METHODS["cell_id"], cc.methods_conc(METHODS, 2), METHODS["cell/equilibrium"],
        METHODS["eq1/pH"], METHODS["eq1/flag"], LIMITS, CONSTS)
    assert cc.worst(pH, METHODS["eq2/pH"]) <= cc.RTOL_PH and n_failed == 0
    np.testing.assert_array_equal(flag, METHODS["eq2/flag"])
    case = cc.methods_dissolution_case(METHODS)
    moles, ratios, _, _ = cc.call_dissolution(hip_engine, case, "closed")
    assert cc.worst(moles, METHODS["dis/moles_out"]) <= cc.RTOL_ARITHMETIC
    assert cc.worst(ratios - case["mixing_ratio"], METHODS["dis/mixing_ratio_closed"]
                    - case["mixing_ratio"]) <= cc.RTOL_ARITHMETIC
    runner = cc.steps_runner(hip_engine, STEPS)
    for step in range(int(STEPS["n_steps"])):
        runner.step()
        got = runner.snapshot()
        np.testing.assert_array_equal(got["flag"], STEPS["steps/flag"][step], err_msg=str(step))
        for key in ("moles", "pH", "mixing_ratio"):
            assert cc.worst(got[key], STEPS[f"steps/{key}"][step]) <= cc.RTOL_STEPS, (step, key)


@pytest.mark.parametrize("system", ["open", "closed"])
@pytest.mark.parametrize("n_sd,n_cell", [(1, 1), (255, 1), (256, 1), (257, 3), (1025, 7),
                                         (3000, 300)])
def test_fused_step_equals_the_checkers_stage_sequence(hip_engine, checker, n_sd, n_cell, system):
    state = cc.drawn_state(100 * n_cell + n_sd, n_sd, n_cell)
    for sum_mode in SUMS if system == "closed" else SUMS[:1]:
        for n_substep in (1, 3):
            snapshots = []
            for engine in (hip_engine, checker):
                runner = cc.runner_for(engine, **state, system=system, n_substep=n_substep,
                                       sum_mode=sum_mode, dt=1.0, dv=1e-3)
                runner.run(2)
                snapshots.append(runner.snapshot())
            for key, value in snapshots[0].items():
                cc.assert_same_bits(value, snapshots[1][key],
                                    f"{key} {sum_mode} n_substep={n_substep}")
    assert (snapshots[0]["moles"] != state["moles"]).any()


@pytest.mark.parametrize("system,sum_mode", [("open", "ordered"), ("closed", "ordered"),
                                             ("closed", "blocked")])
def test_step_equals_step_by_stages_on_the_device(hip_engine, system, sum_mode):
    state = cc.drawn_state(21, 1025, 7)
    snapshots = []
    for route in ("step", "step_by_stages"):
        runner = cc.runner_for(hip_engine, **state, system=system, n_substep=2,
                               sum_mode=sum_mode, dt=1.0, dv=1e-3)
        getattr(runner, route)()
        getattr(runner, route)()
        snapshots.append(runner.snapshot())
    for key, value in snapshots[0].items():
        cc.assert_same_bits(value, snapshots[1][key], key)


@pytest.mark.parametrize("system", ["open", "closed"])
@pytest.mark.parametrize("n_sd,n_cell", [(1, 1), (257, 1), (1025, 7), (3000, 256)])
def test_constants_per_cell_in_lds_equal_constants_per_row(hip_engine, n_sd, n_cell, system):
    state = cc.drawn_state(300 * n_cell + n_sd, n_sd, n_cell)
    snapshots = []
    for constants in ("per_row", "per_cell", "auto"):
        runner = cc.runner_for(hip_engine, **state, system=system, n_substep=3,
                               sum_mode="ordered", dt=1.0, dv=1e-3, constants=constants)
        runner.run(2)
        snapshots.append(runner.snapshot())
    for other in snapshots[1:]:
        for key, value in snapshots[0].items():
            cc.assert_same_bits(value, other[key], key)
    assert (snapshots[0]["moles"] != state["moles"]).any()


def test_constants_per_cell_refuses_more_cells_than_its_table(hip_engine):
    state = cc.drawn_state(15, 600, chem.LDS_CELLS + 1)
    runner = cc.runner_for(hip_engine, **state, system="open", n_substep=1, sum_mode="ordered",
                           dt=1.0, dv=1e-3, constants="per_cell")
    with pytest.raises(RuntimeError, match="error -"):
        runner.step()


def test_flagged_rows_per_cell_at_the_block_and_chunk_edges(hip_engine, checker):
    counts = [0, 1, 255, 256, 257, 3000, 513, 1024]
    case = cc.scale_dv(checker, cc.counted_case(5, counts, unflagged=900))
    for sum_mode in SUMS:
        got = cc.call_dissolution(hip_engine, case, "closed", sum_mode)
        same(got, cc.call_dissolution(checker, case, "closed", sum_mode), f"counts {sum_mode}")
        again = cc.call_dissolution(hip_engine, case, "closed", sum_mode)
        same(again, got, f"run to run {sum_mode}")
    empty = np.array(counts) == 0
    cc.assert_same_bits(got[1][:, empty], case["mixing_ratio"][:, empty], "cell without rows")


def test_event_counts_on_hip(hip_engine, checker):
    case = cc.counted_case(4, [40, 50])
    case["moles"][2, np.flatnonzero(case["flag"])[:3]] = -1.0
    for system in ("open", "closed"):
        got = cc.call_dissolution(hip_engine, case, system)
        same(got, cc.call_dissolution(checker, case, system), f"negative {system}")
        assert got[2] == 3
    case = cc.counted_case(5, [60, 70])
    case["moles"][0] *= 1e-12
    case["henry"][0] *= 1e6
    case["dv"] = 1e-12
    got = cc.call_dissolution(hip_engine, case, "closed")
    same(got, cc.call_dissolution(checker, case, "closed"), "exhausted")
    assert got[3] >= 2
    limits = dict(LIMITS, H_min=1.0, H_max=1.0)
    args = (METHODS["cell_id"], cc.methods_conc(METHODS, 1), METHODS["cell/equilibrium"],
            METHODS["eq1/pH_in"], METHODS["eq1/flag_in"], limits, CONSTS)
    got = cc.call_equilibrate(hip_engine, *args)
    want = cc.call_equilibrate(checker, *args)
    assert got[2] == want[2] == (METHODS["eq1/path"] == 2).sum()
    cc.assert_same_bits(got[1], want[1], "flags")
    np.testing.assert_array_equal(np.isnan(got[0]), np.isnan(want[0]))
    # the runner reports what the fused step counted
    state = cc.drawn_state(12, 300, 2)
    state["moles"] = state["moles"].copy()
    state["moles"][chem.AQUEOUS.index("N_V")] *= 1e-12
    runner = cc.runner_for(hip_engine, **state, system="closed", n_substep=1, sum_mode="ordered",
                           dt=1.0, dv=1e-15)
    runner.step()
    with pytest.raises(RuntimeError, match="delta_mr > env_mixing_ratio"):
        runner.check()


def test_nothing_to_do_keeps_every_bit_on_hip(hip_engine):
    case = cc.counted_case(6, [0, 0, 0], unflagged=500)
    for sum_mode in SUMS:
        moles, ratios, n_negative, n_exceeded = cc.call_dissolution(hip_engine, case, "closed",
                                                                    sum_mode)
        cc.assert_same_bits(moles, case["moles"], "amounts")
        cc.assert_same_bits(ratios, case["mixing_ratio"], "mixing ratios")
        assert (n_negative, n_exceeded) == (0, 0)
    case = cc.counted_case(7, [0, 0], unflagged=0)
    _, ratios, _, _ = cc.call_dissolution(hip_engine, case, "closed")
    cc.assert_same_bits(ratios, case["mixing_ratio"], "no rows")
    # open system: the mixing ratios are not written
    case = cc.counted_case(8, [300, 5])
    moles, ratios, _, _ = cc.call_dissolution(hip_engine, case, "open")
    cc.assert_same_bits(ratios, case["mixing_ratio"], "open system")
    assert (moles != case["moles"]).any()


def test_backend_class_on_hip(hip_backend_class, hip_engine):
    from tests.test_chemistry_checker import backend_dissolution  # pylint: disable=import-outside-toplevel

    case = cc.methods_dissolution_case(METHODS)
    moles, ratios = backend_dissolution(hip_backend_class, case, "closed")
    want = cc.call_dissolution(hip_engine, case, "closed")
    cc.assert_same_bits(moles, want[0], "amounts")
    cc.assert_same_bits(ratios, want[1], "mixing ratios")

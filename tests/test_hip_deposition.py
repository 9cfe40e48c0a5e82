"""Vapour deposition on ice on the MI355X: include/sdm_deposition.h through libsdm_hip.so.

Every comparison is HIP against the CPU checker, bit for bit, in both sum modes: masses, both
predicted columns and n_exceeded.  The shapes are the smallest at which the kernels can still go
wrong: 1 to 4099 rows (the scalar tail, one row over a workgroup's 1024), a mass column that is
8- but not 16-byte aligned, 1 / 7 / 1025 cells with empty cells and a cell that has ice at S_ice
== 1, cells with 0, 1, 255, 256, 257 and 3000 contributing rows (the block edges of the blocked
sum, several LDS chunks of the ordered walk), cell ids sorted and shuffled (the sort's stability),
and 2^16 rows in 1 and in 3 cells (a cell over many workgroups / many chunks).  Then every
formulae combination, the goldens with the CPU tolerances, PySDM's Builder where importable, and
run-to-run equality of the blocked sum."""
import numpy as np
import pytest

from tests import deposition_cases as dc
from tests.test_deposition_checker import METHODS, STEPS, run_pysdm_builder

pytestmark = pytest.mark.gpu
SUMS = ("ordered", "blocked")


@pytest.fixture(scope="module", name="checker")
def checker_engine():
    from tests.deposition_checker import DepositionCheckerEngine  # pylint: disable=import-outside-toplevel

    return DepositionCheckerEngine.get()


def same(hip_engine, checker, case, formulae=None, what="", **options):
    formulae = formulae or dc.formulae_for()
    for sum_mode in SUMS:
        got = dc.call_engine(hip_engine, case, formulae, sum_mode, **options)
        want = dc.call_engine(checker, case, formulae, sum_mode)
        for name, a, b in zip(("mass", "predicted qv", "predicted thd"), got, want):
            dc.assert_same_bits(a, b, f"{what} {sum_mode} {name}")
        assert got[3] == want[3], f"{what} {sum_mode} n_exceeded"


@pytest.mark.parametrize("n_sd", [1, 3, 255, 1024, 1025, 4099])
@pytest.mark.parametrize("n_cell", [1, 7, 1025])
def test_hip_equals_checker_bitwise(hip_engine, checker, n_sd, n_cell):
    s_one, empty = ((), ()) if n_cell == 1 else ((2,), (4, n_cell - 1))
    for sort in (False, True):
        case = dc.seeded_case(1000 * n_cell + n_sd, n_sd, n_cell, sort=sort, s_one=s_one,
                              empty=empty)
        same(hip_engine, checker, case, what=f"n_sd={n_sd} n_cell={n_cell} sorted={sort}")
    assert n_sd < 255 or dc.contributing_rows(case).any()


def test_misaligned_mass_column(hip_engine, checker):
    for n_sd in (1025, 4099):
        case = dc.seeded_case(77 + n_sd, n_sd, 7, s_one=(2,))
        same(hip_engine, checker, case, what=f"misaligned n_sd={n_sd}", misaligned=True)


@pytest.mark.parametrize("sort", [False, True])
def test_contributing_rows_per_cell_at_the_block_and_chunk_edges(hip_engine, checker, sort):
    counts = [0, 1, 255, 256, 257, 3000, 40, 1024, 2048, 2049]
    case = dc.counted_case(5, counts, liquid=700, sort=sort, s_one=(6,))
    n_c = np.bincount(case["cell_id"][dc.contributing_rows(case)], minlength=len(counts))
    np.testing.assert_array_equal(n_c, [0, 1, 255, 256, 257, 3000, 0, 1024, 2048, 2049])
    same(hip_engine, checker, case, what=f"counts sorted={sort}")


@pytest.mark.parametrize("n_cell", [1, 3])
def test_a_cell_over_many_workgroups_and_chunks(hip_engine, checker, n_cell):
    case = dc.seeded_case(31 + n_cell, 2 ** 16, n_cell, ice=0.7)
    same(hip_engine, checker, case, what=f"2^16 rows in {n_cell} cell(s)")
    assert dc.contributing_rows(case).sum() > 40000


@pytest.mark.parametrize("coordinate,capacity,kinetics", dc.COMBINATIONS)
def test_every_formulae_combination(hip_engine, checker, coordinate, capacity, kinetics):
    case = dc.seeded_case(41, 1025, 7, s_one=(2,), empty=(4,))
    if coordinate == "WaterMass":
        case["time_step"] = 0.5  # some sublimating crystals pass through zero
    formulae = dc.formulae_for(coordinate, capacity, kinetics)
    same(hip_engine, checker, case, formulae, f"{coordinate} {capacity} {kinetics}")
    out = dc.call_engine(checker, case, formulae)[0]
    assert (out != case["signed_water_mass"]).any()
    if coordinate == "WaterMass":
        assert ((case["signed_water_mass"] < 0) & (out > 0)).any()


def test_n_exceeded_on_hip(hip_engine, checker):
    case, expected = dc.exceeding_case(7)
    same(hip_engine, checker, case, what="exceeding")
    for sum_mode in SUMS:
        assert dc.call_engine(hip_engine, case, dc.formulae_for(), sum_mode)[3] == expected
    dc.call_engine(hip_engine, case, dc.formulae_for(), with_count=False)


def test_nothing_to_do_keeps_every_bit_on_hip(hip_engine):
    formulae = dc.formulae_for()
    for case in (dc.seeded_case(4, 700, 5, ice=0.0), dc.seeded_case(5, 700, 5, s_one=range(5)),
                 dc.seeded_case(6, 0, 5)):
        for sum_mode in SUMS:
            mass, pqv, pthd, _ = dc.call_engine(hip_engine, case, formulae, sum_mode)
            dc.assert_same_bits(mass, case["signed_water_mass"])
            dc.assert_same_bits(pqv, case["predicted_qv"])
            dc.assert_same_bits(pthd, case["predicted_thd"])


def test_hip_refuses_aliased_arrays(hip_engine):
    case = dc.seeded_case(8, 100, 2)
    with pytest.raises(RuntimeError, match=r"error -"):
        formulae = dc.formulae_for()
        from pysdm_amd import deposition as dep  # pylint: disable=import-outside-toplevel

        up = hip_engine.upload
        arrays = {k: up(np.array(case[k])) for k in dc.AMBIENT}
        hip_engine.call_deposition(
            "sdm_deposition", dep.deposition_cfg(formulae, 0.01, 1.0), 100, 2,
            up(case["multiplicity"]), up(case["signed_water_mass"]), up(case["cell_id"]),
            *(arrays[k] for k in dc.AMBIENT), arrays["qv"], up(np.array(case["thd"])), None,
            dep.constants_of(formulae))


def test_hip_replays_the_goldens_with_the_cpu_tolerances(hip_engine, hip_backend_class):
    for number in range(int(METHODS["n_calls"])):
        case, formulae, want = dc.golden_case(METHODS, number)
        got = dc.call_backend(hip_backend_class, case, formulae)
        dc.assert_within_reference_tolerance(case, got, want, f"call {number}")
    for step, (case, got, want, ambient, after) in enumerate(dc.replay_steps(hip_engine, STEPS)):
        dc.assert_within_reference_tolerance(case, got, want, f"step {step}")
        for key, value in ambient.items():
            np.testing.assert_allclose(value, after[key], rtol=1e-12, atol=0,
                                       err_msg=f"step {step} {key}")


def test_pysdm_builder_runs_on_the_hip_class(hip_backend_class):
    run_pysdm_builder(hip_backend_class)


def test_blocked_sum_returns_equal_bits_run_to_run(hip_engine):
    case = dc.counted_case(6, [3000, 0, 700, 257], liquid=300)
    formulae = dc.formulae_for()
    first = dc.call_engine(hip_engine, case, formulae, "blocked")
    second = dc.call_engine(hip_engine, case, formulae, "blocked")
    for a, b in zip(first[:3], second[:3]):
        dc.assert_same_bits(a, b)
    assert first[3] == second[3]

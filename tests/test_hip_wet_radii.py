"""The initialisation path on the device (pysdm_amd/csrc/initialisation.hip) against the CPU checker
of include/sdm_initialisation.h: r_wet and iters bit for bit (both sides compile the same
condensation_formulae.h, toms748.h and sdm_math.h without contraction), the status words equal.

On every set of tests/golden/wet_radii.npz and on the failing searches of wet_radii_fail.npz (out
of iterations, and no sign change in the bracket: the search's own -1), at
n = 1, 255, 256, 257 (around one workgroup) and at one row past a full pass of the capped grid; for
that size the golden's rows are tiled and each repetition shifts the cells, so the checker only has
to run every (row, cell) combination once.  Also: cell_id = NULL and f_org = NULL, the drop-in of
pysdm_amd.pysdm_plugin on HIP storages, and `wet_aerosol` followed by one condensation step.
Nothing here faults or times out: the failing searches return normally with status words."""
import numpy as np
import pytest

from tests import condensation_cases as cc
from tests import wet_radii_cases as wc

pytestmark = pytest.mark.gpu

GRID_PASS = wc.GRID_PASS
CASES = [*wc.SETS, "fail/1", "fail/2", *(f"nosign/{n}" for n in wc.NO_SIGN_CHANGE_SETS)]


@pytest.fixture(scope="module", name="checker")
def checker_engine():
    from tests.initialisation_checker import InitialisationCheckerEngine  # pylint: disable=import-outside-toplevel

    return InitialisationCheckerEngine.get()


def case(name):
    """(formulae, rows, T, RH, rtol, max_iters) of a set of wet_radii.npz or of a failing run"""
    if name.startswith("fail/"):
        data = cc.gold("wet_radii_fail")
        rows = {k: np.array(data[k]) for k in ("r_dry", "kappa_times_dry_volume", "cell_id")}
        rows["f_org"] = np.zeros(len(rows["r_dry"]))
        return (wc.formulae_of("fail"), rows, data["T"], data["RH"], float(data["rtol"]),
                int(name[len("fail/"):]))
    if name.startswith("nosign/"):  # rows on which the search itself returns (NaN, -1)
        data, name = cc.gold("wet_radii_fail"), name[len("nosign/"):]
        return (wc.formulae_of(name), wc.no_sign_change_rows(data, name), data["T"], data["RH"],
                wc.RTOL, wc.MAX_ITERS)
    data = cc.gold("wet_radii")
    return (wc.formulae_of(name), wc.set_arrays(data, name), data["T"], data["RH"], wc.RTOL,
            wc.MAX_ITERS)


def same(got, want, what):
    for g, w, part in zip(got, want, ("r_wet", "iters", "status")):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {part}")  # (NaN == NaN here)
    if got[0].size:
        finite = ~np.isnan(want[0])
        np.testing.assert_array_equal(got[0][finite].view(np.int64),
                                      want[0][finite].view(np.int64), err_msg=what)


@pytest.mark.parametrize("n", (1, 255, 256, 257))
@pytest.mark.parametrize("name", CASES)
def test_hip_equals_checker(hip_engine, checker, name, n):
    formulae, rows, T, RH, rtol, max_iters = case(name)
    index = np.arange(n) % len(rows["r_dry"])
    options = dict(index=index, rtol=rtol, max_iters=max_iters)
    want = wc.call_set(checker, formulae, rows, T, RH, **options)
    got = wc.call_set(hip_engine, formulae, rows, T, RH, **options)
    same(got, want, f"{name}, n = {n}")
    assert list(want[2][:3]) == wc.expected_status(want[1], max_iters)
    if n == 257 and name.startswith("fail/"):
        assert want[2][0] + want[2][1] >= 8
    if n == 257 and name.startswith("nosign/"):
        assert want[2][0] >= 25 and want[2][2] == 3  # (the failing rows, tiled)


@pytest.mark.parametrize("name", CASES)
def test_one_row_past_a_pass_of_the_capped_grid(hip_engine, checker, name):
    formulae, rows, T, RH, rtol, max_iters = case(name)
    m, n_cell, n = len(rows["r_dry"]), len(T), GRID_PASS + 1
    # every (row, cell shift) once on the checker ...
    unique = np.arange(m * n_cell)
    shifted = (rows["cell_id"][unique % m] + unique // m) % n_cell
    r_wet, iters, _ = wc.call_set(checker, formulae, rows, T, RH, index=unique % m,
                                  cell_id=shifted, rtol=rtol, max_iters=max_iters)
    # ... and the tiled rows, the cells shifted by the repetition, on the device
    i = np.arange(n)
    at = (i // m % n_cell) * m + i % m
    got = wc.call_set(hip_engine, formulae, rows, T, RH, index=i % m,
                      cell_id=np.ascontiguousarray(shifted[at]), rtol=rtol, max_iters=max_iters)
    status = [*wc.expected_status(iters[at], max_iters), 0]
    same(got, (r_wet[at], iters[at], status), f"{name}, n = {n}")


@pytest.mark.parametrize("name", ("Constant_KappaKoehlerLeadingTerms", "Constant_KappaKoehler"))
def test_without_cell_id_and_f_org(hip_engine, checker, name):
    formulae, rows, T, RH, rtol, max_iters = case(name)
    options = dict(cell_id=None, f_org=None, rtol=rtol, max_iters=max_iters)
    want = wc.call_set(checker, formulae, rows, T[3:], RH[3:], **options)
    got = wc.call_set(hip_engine, formulae, rows, T[3:], RH[3:], **options)
    same(got, want, name)
    assert (want[1] > 0).any()


def test_out_of_range_cells_and_no_rows(hip_engine, checker):
    formulae, rows, T, RH, rtol, max_iters = case("Constant_KappaKoehlerLeadingTerms")
    cells = rows["cell_id"].copy()
    cells[[5, 17, 300]] = (len(T), -1, 2 ** 40)
    options = dict(cell_id=cells, rtol=rtol, max_iters=max_iters)
    want = wc.call_set(checker, formulae, rows, T, RH, **options)
    got = wc.call_set(hip_engine, formulae, rows, T, RH, **options)
    same(got, want, "cells out of range")
    assert list(got[2]) == [3, 0, 5, 0] and np.isnan(got[0][[5, 17, 300]]).all()
    empty = wc.call_set(hip_engine, formulae, rows, T, RH, index=np.zeros(0, dtype=np.int64))
    assert empty[0].shape == (0,) and list(empty[2]) == [0, 0, 0, 0]


@pytest.mark.parametrize("name", ("Constant_KappaKoehlerLeadingTerms",
                                  "CompressedFilmRuehl_KappaKoehler"))
def test_drop_in_on_hip_storages(hip_backend_class, checker, name):
    from pysdm_amd.pysdm_plugin import equilibrate_wet_radii  # pylint: disable=import-outside-toplevel

    formulae, rows, T, RH, _, _ = case(name)
    environment = wc.StubEnvironment(hip_backend_class, formulae, T, RH)
    assert environment["T"].data.is_cuda
    got = equilibrate_wet_radii(
        r_dry=rows["r_dry"], environment=environment, f_org=rows["f_org"],
        kappa_times_dry_volume=rows["kappa_times_dry_volume"], cell_id=rows["cell_id"])
    want, _, _ = wc.call_set(checker, formulae, rows, T, RH)
    assert isinstance(got, np.ndarray)
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))


def test_wet_aerosol_and_one_condensation_step(hip_engine, checker):
    gold = cc.gold("wet_radii")
    got, got_after, _, _ = wc.aerosol_step(hip_engine, gold)
    want, want_after, _, _ = wc.aerosol_step(checker, gold)
    for key, value in want.items():
        np.testing.assert_array_equal(got[key], value, err_msg=key)
    np.testing.assert_array_equal(got_after.view(np.int64), want_after.view(np.int64))

"""The initialisation path (include/sdm_initialisation.h, pysdm_amd/initialisation.py, the spectra
of pysdm_amd/spectra.py and the drop-in of pysdm_amd/pysdm_plugin.py) on the CPU checker
(tests/initialisation_checker/), against what the reference itself returned
(tests/golden/wet_radii.npz, wet_radii_fail.npz, lognormal_sampling.npz; generator:
tests/golden/gen_wet_radii_golden.py).

Bounds.  Early-exit rows are exact.  On solved rows the worst relative difference per set is
MEASURED (tests/golden/wet_radii_measured.json, rewritten by this file when the environment variable
SDM_REGENERATE_WET_RADII_MEASURED is 1) and the bound is four times it: the reference ran with
NumPy's exp / log / power, sdm_math.h rounds correctly, and a last bit can turn into one bracket
step more or fewer.  No recorded value may exceed the search's own rtol (1e-5): two roots further
apart than that would be different brackets.  The spectra are bounded the same way (equality where
the measurement is 0).
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from pysdm_amd import abi, initialisation as init, spectra
from pysdm_amd.condensation import CONSTANT_NAMES, check_formulae
from pysdm_amd.formulae import Formulae
from tests import condensation_cases as cc
from tests import wet_radii_cases as wc

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("PYSDM_REFERENCE", "")
REGENERATE = os.environ.get(wc.REGENERATE) == "1"
SAMPLERS = {"constant_multiplicity": spectra.sample_constant_multiplicity,
            "logarithmic": spectra.sample_logarithmic}


@pytest.fixture(scope="module", name="engine")
def _engine():
    from tests.initialisation_checker import InitialisationCheckerEngine  # pylint: disable=import-outside-toplevel

    return InitialisationCheckerEngine.get()


@pytest.fixture(scope="module", name="gold")
def _gold():
    return cc.gold("wet_radii")


def worst(got, ref):
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(got == ref, 0.0, np.abs(got - ref) / np.abs(ref))
    return float(np.max(rel)) if rel.size else 0.0


def record(key, value):
    """prints the measurement; with the regenerate switch also writes it to the json"""
    print("measured", key, value)
    if REGENERATE:
        try:
            table = wc.measured()
        except FileNotFoundError:
            table = {}
        table["_about"] = ("worst relative differences checker vs reference, written by "
                           "tests/test_wet_radii_checker.py; the tests bound each at 4x")
        table[key] = value
        with open(wc.MEASURED_PATH, "w", encoding="utf-8") as file:
            json.dump(table, file, indent=1, sort_keys=True)
            file.write("\n")


def bounded(key, value):
    """value <= 4 x the recorded measurement (equality with the golden where that is 0)"""
    record(key, value)
    assert value <= 4 * wc.measured()[key], (key, value, wc.measured()[key])


# ---- the goldens -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(wc.SETS))
def test_checker_reproduces_the_reference(engine, gold, name):
    rows = wc.set_arrays(gold, name)
    r_wet, iters, status = wc.call_set(engine, wc.formulae_of(name), rows, gold["T"], gold["RH"])
    early = (rows["label"] & (wc.NOT_A_LT_B | wc.FA_NEGATIVE)) != 0
    assert early.any() and (rows["iters"][early] == 0).all()
    np.testing.assert_array_equal(iters[early], 0)
    np.testing.assert_array_equal(r_wet[early], rows["r_dry"][early])
    np.testing.assert_array_equal(r_wet[early], rows["r_wet"][early])
    solved = (rows["label"] & wc.SOLVED) != 0
    assert (iters[solved] > 0).all() and (iters[solved] < wc.MAX_ITERS).all()
    # (neither early nor solved: the search returned at once, e.g. minfun(a) == 0)
    rest = ~early & ~solved
    np.testing.assert_array_equal(iters[rest], 0)
    np.testing.assert_array_equal(r_wet[rest], rows["r_wet"][rest])
    assert list(status) == [0, 0, len(r_wet), 0]
    bounded(f"wet_radii/{name}", worst(r_wet[solved], rows["r_wet"][solved]))


def test_no_measured_difference_exceeds_the_rtol_of_the_search():
    table = wc.measured()
    assert {k for k in table if k.startswith("wet_radii/")} == {f"wet_radii/{n}" for n in wc.SETS}
    for key, value in table.items():
        if key.startswith("wet_radii"):
            assert value <= wc.RTOL, (key, value)


@pytest.mark.parametrize("name", [n for n, o in wc.SETS.items()
                                  if o["surface_tension"] == "Constant"])
def test_solved_rows_bracket_a_sign_change_of_minfun(engine, gold, name):
    """independent of the golden: a NumPy restatement of minfun changes sign within 2 rtol of the
    root, which lies between r_dry and r_cr"""
    rows = wc.set_arrays(gold, name)
    formulae = wc.formulae_of(name)
    r_wet, _, _ = wc.call_set(engine, formulae, rows, gold["T"], gold["RH"])
    solved = (rows["label"] & wc.SOLVED) != 0
    k = formulae.constants
    r_dry, T, RH = (rows["r_dry"][solved], gold["T"][rows["cell_id"]][solved],
                    gold["RH"][rows["cell_id"]][solved])
    kappa = rows["kappa_times_dry_volume"][solved] / (k.PI_4_3 * r_dry ** 3)
    r_cr = np.sqrt(3 * kappa * r_dry ** 3 / (2 * k.sgm_w / k.Rv / T / k.rho_w))
    root = r_wet[solved]
    assert (r_dry <= root).all() and (root <= r_cr).all()
    hygro = wc.SETS[name]["hygroscopicity"]
    below = wc.minfun_constant_sgm(formulae, hygro, root * (1 - 2 * wc.RTOL), T, RH, kappa,
                                   r_dry ** 3)
    above = wc.minfun_constant_sgm(formulae, hygro, root * (1 + 2 * wc.RTOL), T, RH, kappa,
                                   r_dry ** 3)
    assert (below * above <= 0).all(), np.flatnonzero(below * above > 0)


@pytest.mark.parametrize("max_iters", (1, 2))
def test_failing_searches_are_counted_and_raised(engine, max_iters):
    data = cc.gold("wet_radii_fail")
    formulae = wc.formulae_of("fail")
    rows = {k: np.array(data[k]) for k in ("r_dry", "kappa_times_dry_volume", "cell_id")}
    rows["f_org"] = None
    ref_iters = data[f"iters/{max_iters}"]
    assert data[f"asserted/{max_iters}"].sum() >= 8
    r_wet, iters, status = wc.call_set(engine, formulae, rows, data["T"], data["RH"], f_org=None,
                                       rtol=float(data["rtol"]), max_iters=max_iters)
    np.testing.assert_array_equal(iters, ref_iters)
    assert list(status[:3]) == wc.expected_status(ref_iters, max_iters) and status[3] == 0
    bounded(f"wet_radii_fail/{max_iters}", worst(r_wet, data[f"r_wet/{max_iters}"]))
    with pytest.raises(init.WetRadiusError) as error:
        init.equilibrate_wet_radii(
            engine, formulae, r_dry=rows["r_dry"], cell_id=rows["cell_id"],
            kappa_times_dry_volume=rows["kappa_times_dry_volume"], T=np.array(data["T"]),
            RH=np.array(data["RH"]), rtol=float(data["rtol"]), max_iters=max_iters)
    assert isinstance(error.value, AssertionError)
    first = wc.expected_status(ref_iters, max_iters)[2]
    assert error.value.status[:3] == wc.expected_status(ref_iters, max_iters)
    assert f"i={first}, r_d={float(rows['r_dry'][first])!r}" in str(error.value)
    for word in ("T=", "RH=", "kappa=", "f_org="):
        assert word in str(error.value)


def test_the_sets_with_rows_without_a_sign_change_are_the_goldens():
    data = cc.gold("wet_radii_fail")
    names = {k.split("/")[1] for k in data.files if k.startswith("no_sign_change/")}
    assert names == set(wc.NO_SIGN_CHANGE_SETS)
    assert sum(int((data[f"no_sign_change/{n}/iters"] == -1).sum()) for n in names) >= 7


@pytest.mark.parametrize("name", wc.NO_SIGN_CHANGE_SETS)
def test_rows_without_a_sign_change_fail_as_in_the_reference(engine, name):
    """the search's own (NaN, -1): where the reference's TOMS748 finds no sign change between
    r_dry and r_cr, so does this one, on the same rows, and SDM_INIT_STATUS_FAILED counts them"""
    data = cc.gold("wet_radii_fail")
    rows, formulae = wc.no_sign_change_rows(data, name), wc.formulae_of(name)
    failed = rows["iters"] == -1
    assert failed.any() and np.isnan(rows["r_wet"][failed]).all()
    r_wet, iters, status = wc.call_set(engine, formulae, rows, data["T"], data["RH"])
    np.testing.assert_array_equal(iters == -1, failed)
    np.testing.assert_array_equal(np.isnan(r_wet), failed)
    assert (iters[~failed] > 0).all()
    np.testing.assert_allclose(r_wet[~failed], rows["r_wet"][~failed], atol=0,
                               rtol=4 * wc.measured()[f"wet_radii/{name}"])
    assert list(status) == [int(failed.sum()), 0, 3, 0]
    with pytest.raises(init.WetRadiusError, match=f"for {int(failed.sum())} particle") as error:
        init.equilibrate_wet_radii(
            engine, formulae, r_dry=rows["r_dry"], f_org=rows["f_org"], cell_id=rows["cell_id"],
            kappa_times_dry_volume=rows["kappa_times_dry_volume"], T=np.array(data["T"]),
            RH=np.array(data["RH"]))
    assert "i=3, " in str(error.value)


def test_an_inner_search_out_of_iterations_is_counted(engine, gold, tmp_path):
    """where the reference's CompressedFilmRuehl asserts `iters != max_iters` the row is counted
    in SDM_INIT_STATUS_SIGMA_FAILED.  100 iterations are out of reach of the isotherm's search, so
    the checker is built once more with a cap of 2 (as test_condensation_formulae_checker.py does):
    the set that is clean with the real cap is not with this one, and nothing traps"""
    import subprocess  # pylint: disable=import-outside-toplevel

    from oracle import engine as oracle_engine  # pylint: disable=import-outside-toplevel
    from tests import initialisation_checker as checker  # pylint: disable=import-outside-toplevel

    name = "CompressedFilmRuehl_KappaKoehlerLeadingTerms"
    rows, formulae = wc.set_arrays(gold, name), wc.formulae_of(name)
    assert wc.call_set(engine, formulae, rows, gold["T"], gold["RH"])[2][3] == 0
    lib = str(tmp_path / "libcapped.so")
    subprocess.check_call(["gcc", *oracle_engine._FLAGS, "-DCF_RUEHL_MAX_ITERS=2", "-o", lib,  # pylint: disable=protected-access
                           checker.SOURCE, "-lm"])
    real = engine.initialisation_library
    engine.initialisation_library = abi.Library(
        lib, "the initialisation checker with a capped isotherm search",
        header=abi.INITIALISATION_HEADER_PATH)
    try:
        r_wet, _, status = wc.call_set(engine, formulae, rows, gold["T"], gold["RH"])
        with pytest.raises(init.WetRadiusError, match="inner search used up its iterations"):
            init.equilibrate_wet_radii(
                engine, formulae, r_dry=rows["r_dry"], f_org=rows["f_org"],
                kappa_times_dry_volume=rows["kappa_times_dry_volume"], cell_id=rows["cell_id"],
                T=np.array(gold["T"]), RH=np.array(gold["RH"]))
    finally:
        engine.initialisation_library = real
    searched = ((rows["label"] & wc.NOT_A_LT_B) == 0) & (rows["f_org"] > 0) & (rows["f_org"] < 1)
    assert 0 < status[3] <= searched.sum()
    assert r_wet.shape == rows["r_dry"].shape


# ---- spectra and multiplicities ---------------------------------------------------------------------
def _spectrum(data, name):
    if name == "single":
        return spectra.Lognormal(*data["single/params"])
    return spectra.Sum([spectra.Lognormal(*mode) for mode in data["sum/params"]])


@pytest.mark.parametrize("name", ("single", "sum"))
def test_lognormal_spectra_reproduce_the_reference(name):
    data = cc.gold("lognormal_sampling")
    spectrum = _spectrum(data, name)
    bounded(f"sampling/{name}/cumulative",
            worst(spectrum.cumulative(data[f"{name}/probe"]), data[f"{name}/cumulative"]))
    bounded(f"sampling/{name}/percentiles",
            worst(spectrum.percentiles(data[f"{name}/quantiles"]), data[f"{name}/percentiles"]))
    for sampler_name, sampler in SAMPLERS.items():
        for n_sd in (2 ** 6, 2 ** 10):
            x, counts = sampler(spectrum, n_sd)
            key = f"{name}/{sampler_name}/{n_sd}"
            assert x.shape == counts.shape == (n_sd,)
            bounded(f"sampling/{key}/x", worst(x, data[f"{key}/x"]))
            bounded(f"sampling/{key}/counts", worst(counts, data[f"{key}/counts"]))


def test_discretise_multiplicities():
    data = cc.gold("lognormal_sampling")
    out = init.discretise_multiplicities(data["discretise/in"])
    assert out.dtype == np.int64
    np.testing.assert_array_equal(out, data["discretise/out"])
    np.testing.assert_array_equal(init.discretise_multiplicities(np.asarray([np.nan, 200.4])),
                                  [0, 200])
    with pytest.raises(ValueError, match="multiplicity of zero"):
        init.discretise_multiplicities(np.asarray([0.2, 5.0]))
    with pytest.raises(ValueError, match="error in total real-droplet number"):
        init.discretise_multiplicities(np.asarray([1.45, 1.45, 1.45]))


# ---- end to end ----------------------------------------------------------------------------------------
def test_wet_aerosol_is_the_equilibrium_the_condensation_solver_sees(engine, gold):
    aerosol, _, change, cfg = wc.aerosol_step(engine, gold)
    np.testing.assert_array_equal(aerosol["multiplicity"], cfg["multiplicity"])
    np.testing.assert_allclose(aerosol["r_dry"], cfg["r_dry"], rtol=1e-12)
    np.testing.assert_allclose(aerosol["r_wet"], cfg["r_wet"], rtol=4 * wc.RTOL)
    assert (aerosol["r_wet"] > aerosol["r_dry"]).all()
    print("largest relative change of a water mass:", change, "reference:",
          float(cfg["max_relative_change"]))
    assert change <= 4 * float(cfg["max_relative_change"])


def test_wet_aerosol_with_kappa_zero_skips_the_kernel(gold):
    class NoLibrary:  # pylint: disable=too-few-public-methods
        """an engine that can do nothing: kappa == 0 must not reach it"""

    ambient = type("Ambient", (), {"T": None, "RH": None})()
    out = init.wet_aerosol(NoLibrary(), Formulae(), ambient, n_sd=32, kappa=0,
                           spectrum=spectra.Lognormal(*gold["aerosol/spectrum"]))
    np.testing.assert_array_equal(out["r_wet"], out["r_dry"])
    assert (out["kappa_times_dry_volume"] == 0).all()


# ---- the ABI's argument checks ---------------------------------------------------------------------------
def raw_call(engine, formulae, rows=3, descriptor="own", **over):
    n = rows
    arrays = dict(r_dry=np.full(n, 5e-8), ktdv=np.full(n, 0.5 * 4 / 3 * np.pi * 5e-8 ** 3),
                  f_org=np.zeros(n), cell_id=np.zeros(n, dtype=np.int64), T=np.full(2, 280.0),
                  RH=np.full(2, 0.9), r_wet=np.zeros(n), iters=np.zeros(n, dtype=np.int64),
                  status=np.zeros(4, dtype=np.int64))
    scalars = dict(n=n, n_cell=2, rtol=1e-5, max_iters=64)
    for key, value in over.items():
        (scalars if key in scalars else arrays)[key] = value
    a = arrays
    engine.call_initialisation(
        "sdm_equilibrate_wet_radii", scalars["n"], a["r_dry"], a["ktdv"], a["f_org"],
        a["cell_id"], a["T"], a["RH"], scalars["n_cell"], scalars["rtol"], scalars["max_iters"],
        [float(getattr(formulae.constants, name)) for name in CONSTANT_NAMES],
        check_formulae(formulae) if isinstance(descriptor, str) else descriptor,
        a["r_wet"], a["iters"], a["status"])
    return a


@pytest.mark.parametrize("missing", ("r_dry", "ktdv", "T", "RH", "r_wet", "iters", "status"))
def test_null_pointers_are_refused(engine, missing):
    with pytest.raises(RuntimeError, match="error -1"):
        raw_call(engine, Formulae(), **{missing: None})


def test_bad_scalars_and_option_codes_are_refused(engine):
    formulae = Formulae()
    for over in ({"n": -1}, {"n_cell": 0}, {"max_iters": 0}):
        with pytest.raises(RuntimeError, match="error -1"):
            raw_call(engine, formulae, **over)
    descriptor = abi.CondFormulae()
    descriptor.option[5] = 4  # surface_tension has four choices
    with pytest.raises(RuntimeError, match="error -1"):
        raw_call(engine, formulae, descriptor=descriptor)
    descriptor.option[5] = -1
    with pytest.raises(RuntimeError, match="error -1"):
        raw_call(engine, formulae, descriptor=descriptor)


def test_f_org_may_be_null_only_without_a_film(engine):
    film = wc.formulae_of("CompressedFilmOvadnevaite_KappaKoehlerLeadingTerms")
    with pytest.raises(RuntimeError, match="error -1"):
        raw_call(engine, film, f_org=None)
    out = raw_call(engine, Formulae(), f_org=None, cell_id=None, descriptor=None)
    assert (out["iters"] > 0).all() and (out["r_wet"] > out["r_dry"]).all()
    # (the host layer supplies the zeros the reference supplies)
    r_wet = init.equilibrate_wet_radii(engine, film, r_dry=out["r_dry"], T=out["T"], RH=out["RH"],
                                       kappa_times_dry_volume=out["ktdv"])
    assert (engine.download(r_wet) > out["r_dry"]).all()


def test_cell_id_out_of_range_is_a_counted_failure_not_a_read(engine):
    out = raw_call(engine, Formulae(), rows=5, cell_id=np.asarray([0, 2, 1, -1, 0], dtype=np.int64))
    assert np.isnan(out["r_wet"][[1, 3]]).all() and (out["iters"][[1, 3]] == -1).all()
    assert (out["iters"][[0, 2, 4]] > 0).all()
    assert list(out["status"]) == [2, 0, 1, 0]


def test_no_rows(engine):
    out = raw_call(engine, Formulae(), rows=0, r_dry=None, ktdv=None, r_wet=None, iters=None,
                   f_org=None, cell_id=None, status=np.full(4, 7, dtype=np.int64))
    assert list(out["status"]) == [7, 7, 7, 7]  # returned before anything was written
    r_wet = init.equilibrate_wet_radii(engine, Formulae(), r_dry=np.zeros(0), T=np.full(1, 280.0),
                                       kappa_times_dry_volume=np.zeros(0), RH=np.full(1, 0.9))
    assert engine.download(r_wet).shape == (0,)


def test_an_engine_without_the_library_says_so():
    from oracle.engine import OracleEngine  # pylint: disable=import-outside-toplevel

    with pytest.raises(NotImplementedError, match="engine `.*` has no initialisation library"):
        OracleEngine.get().call_initialisation("sdm_equilibrate_wet_radii")


def test_the_header_is_bound_as_written():
    table = abi.parse_header(abi.INITIALISATION_HEADER_PATH)
    assert list(table) == ["sdm_equilibrate_wet_radii"]
    names = [p.name for p in table["sdm_equilibrate_wet_radii"][1]]
    assert names == ["ctx", "n", "r_dry", "kappa_times_dry_volume", "f_org", "cell_id", "T", "RH",
                     "n_cell", "rtol", "max_iters", "consts", "formulae", "r_wet", "iters",
                     "status"]
    assert ctypes.sizeof(abi.CondFormulae) == 40 + 72 * 8
    with open(abi.INITIALISATION_HEADER_PATH, encoding="utf-8") as header:
        assert f"#define SDM_INIT_ROWS_PER_PASS {wc.GRID_PASS}\n" in header.read()


# ---- the drop-in of pysdm_amd.pysdm_plugin --------------------------------------------------------------
@pytest.mark.parametrize("name", ("Constant_KappaKoehlerLeadingTerms",
                                  "CompressedFilmRuehl_KappaKoehler"))
def test_drop_in_equals_the_host_layer_bit_for_bit(engine, gold, name):
    from pysdm_amd.pysdm_plugin import equilibrate_wet_radii  # pylint: disable=import-outside-toplevel
    from tests.initialisation_checker import InitialisationCheckerBackend  # pylint: disable=import-outside-toplevel

    rows, formulae = wc.set_arrays(gold, name), wc.formulae_of(name)
    environment = wc.StubEnvironment(InitialisationCheckerBackend, formulae, gold["T"], gold["RH"])
    got = equilibrate_wet_radii(
        r_dry=rows["r_dry"], environment=environment, f_org=rows["f_org"],
        kappa_times_dry_volume=rows["kappa_times_dry_volume"], cell_id=rows["cell_id"])
    assert isinstance(got, np.ndarray)
    want, _, _ = wc.call_set(engine, formulae, rows, gold["T"], gold["RH"])
    np.testing.assert_array_equal(got, want)


def test_drop_in_refuses_foreign_storages_where_there_is_no_gpu(monkeypatch):
    import torch  # pylint: disable=import-outside-toplevel

    from pysdm_amd.pysdm_plugin import equilibrate_wet_radii  # pylint: disable=import-outside-toplevel

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    class Foreign:  # pylint: disable=too-few-public-methods
        @staticmethod
        def to_ndarray():
            return np.full(1, 280.0)

    environment = type("Env", (), {"__getitem__": lambda self, item: Foreign()})()
    with pytest.raises(NotImplementedError, match="another backend and there is no GPU"):
        equilibrate_wet_radii(r_dry=np.full(1, 5e-8), environment=environment,
                              kappa_times_dry_volume=np.full(1, 1e-22))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "PySDM")),
                    reason="reference tree not named by PYSDM_REFERENCE")
def test_reference_unit_test_cases_pass_with_the_drop_in(monkeypatch):
    """the reference's own tests/unit_tests/initialisation/test_equilibrate_wet_radii.py, loaded
    from its tree, with the drop-in and the checker-bound backend class in place of its imports"""
    import importlib.util  # pylint: disable=import-outside-toplevel

    os.environ.setdefault("CI", "1")
    monkeypatch.setenv("MPLBACKEND", "Agg")
    added = [os.path.join(HERE, "golden", "standins"), REFERENCE]
    sys.path[:0] = added
    try:
        path = os.path.join(REFERENCE, "tests", "unit_tests", "initialisation",
                            "test_equilibrate_wet_radii.py")
        spec = importlib.util.spec_from_file_location("reference_test_equilibrate_wet_radii", path)
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)  # (a failure to import it is a failure)
        from pysdm_amd import pysdm_plugin  # pylint: disable=import-outside-toplevel
        from tests.initialisation_checker import InitialisationCheckerBackend  # pylint: disable=import-outside-toplevel

        module.equilibrate_wet_radii = pysdm_plugin.equilibrate_wet_radii
        module.CPU = pysdm_plugin.as_pysdm_backend(InitialisationCheckerBackend)
        params = {mark.args[0]: mark.args[1]
                  for mark in module.test_equilibrate_wet_radii.pytestmark}
        radii = [p.values[0] if hasattr(p, "values") else p for p in params["r_dry"]]
        tensions = list(params["surface_tension"])
        assert len(radii) == 2 and len(tensions) == 3
        for r_dry in radii:
            for surface_tension in tensions:
                module.test_equilibrate_wet_radii(r_dry, surface_tension)
    finally:
        for path in added:
            sys.path.remove(path)

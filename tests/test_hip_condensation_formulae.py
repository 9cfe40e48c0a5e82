"""Condensation with non-default formulae on the MI355X: include/sdm_condensation_formulae.h
through libsdm_hip.so (the general instantiation of csrc/condensation_solver.h).  Sets with a
choice that `Formulae` refuses (condensation_formulae_cases.host_refused) run with an explicit
descriptor.

(i) HIP and the CPU checker (tests/condensation_formulae_checker/) agree bit for bit for every
non-default choice of every option and for the three combined sets, on seeded cells of 1, 63, 64,
65, 256, 257, 1024, 1025 and 2100 super-droplets and two empty ones (the lane stride, the limit of
the LDS-staged positions, the first and the second streamed chunk), adaptive and not, with f_org in
{0, 1, between}, Reynolds numbers 0 and > 0, multiplicity-0 and water-mass <= 0 rows; (ii) HIP
replays the reference's goldens within the bounds of the CPU test; (iii) PySDM's default formulae
through `sdm_condensation_f` equal `sdm_condensation` bit for bit; (iv) the failing bracket gives
success = 0 and the context stays usable; (v) the two `_f` ambient methods agree bit for bit."""
import numpy as np
import pytest

from pysdm_amd.formulae import Formulae
from tests import condensation_cases as cc
from tests import condensation_formulae_cases as fc

pytestmark = pytest.mark.gpu
OUT_KEYS = (*cc.OUT_INTS, *cc.OUT_FLOATS)
CELLS = [1, 63, 64, 65, 0, 256, 257, 1024, 1025, 0, 2100]


def _bitwise(a, b, where=""):
    for key in OUT_KEYS:
        np.testing.assert_array_equal(np.asarray(a[key]).view(np.uint8),
                                      np.asarray(b[key]).view(np.uint8), err_msg=f"{where} {key}")


def _checker_engine():
    from tests.condensation_formulae_checker import CheckerEngine  # pylint: disable=import-outside-toplevel

    return CheckerEngine.get()


def _checker_backend(name_or_options):
    from tests.condensation_formulae_checker import CheckerBackend  # pylint: disable=import-outside-toplevel

    return CheckerBackend(fc.formulae_for(name_or_options))


@pytest.mark.parametrize("adaptive", [True, False])
@pytest.mark.parametrize("name", list(fc.SETS))
def test_hip_equals_checker_bitwise(name, adaptive, hip_engine):
    case = fc.seeded_case(101, CELLS, fc.SETS[name]["options"])
    assert (case["f_org"] == 0).any() and (case["f_org"] == 1).any()
    assert (case["reynolds_number"] == 0).any() and (case["reynolds_number"] > 100).any()
    assert (case["multiplicity"] == 0).any() and (case["water_mass"] <= 0).any()
    a = fc.run_case(hip_engine, case, adaptive=adaptive)
    b = fc.run_case(_checker_engine(), case, adaptive=adaptive)
    _bitwise(a, b, name)
    counts = np.asarray(CELLS)
    assert (a["success"][counts > 0] == 1).all()
    assert (a["n_substeps"][counts == 0] == (-1 if adaptive else 3)).all()  # untouched
    if adaptive:
        assert a["n_substeps"].max() > 3


@pytest.mark.parametrize("name", list(fc.GOLDENS))
def test_hip_replays_recorded_calls(name, hip_backend_class, hip_engine):
    from tests.condensation_formulae_checker import CheckerBackend  # pylint: disable=import-outside-toplevel

    data = cc.gold(f"condf_{name}")
    for call in range(int(data["n_calls"])):
        out = fc.replay(hip_backend_class, hip_engine, name, data, call)
        fc.assert_matches_golden(out, data, call, name)
        _bitwise(out, fc.replay(CheckerBackend, _checker_engine(), name, data, call),
                 f"{name} call {call}")


@pytest.mark.parametrize("adaptive", [True, False])
def test_default_formulae_through_the_general_kernel_equal_the_default_kernel(adaptive,
                                                                              hip_engine):
    """pins the dispatch and the policy split: same bits from both instantiations"""
    case = cc.seeded_case(101, CELLS)
    a = fc.run_case(hip_engine, case, adaptive=adaptive, general=True)
    b = fc.run_case(hip_engine, case, adaptive=adaptive)
    _bitwise(a, b, "general vs default")
    _bitwise(a, fc.run_case(_checker_engine(), case, adaptive=adaptive, general=True),
             "general vs checker")


def test_hip_failed_brackets_give_success_zero_and_the_context_stays_usable(hip_engine,
                                                                            hip_backend_class):
    data = cc.gold("condf_bracket_fail")
    out = cc.replay(hip_backend_class(fc.formulae_for("bracket_fail")), data, 0)
    assert out["success"].tolist() == [0]
    fc.assert_matches_golden(out, data, 0, "bracket_fail")
    # failing searches in some cells of a larger state, both sides alike
    options = {"surface_tension": "CompressedFilmRuehl", "ventilation": "Froessling1938"}
    # (adaptive: small cells, since a failing cell's adaptivity runs to dt_min on the serial
    # checker too; fixed: a failure among the streamed positions beyond the first 1024 as well)
    for adaptive, cells in ((True, [20, 30, 25, 1, 7, 0, 65]),
                            (False, [20, 30, 25, 1, 7, 0, 300, 1100])):
        case = fc.seeded_case(5, cells, options, max_iters=4)
        a = fc.run_case(hip_engine, case, adaptive=adaptive)
        _bitwise(a, fc.run_case(_checker_engine(), case, adaptive=adaptive),
                 f"adaptive={adaptive}")
        assert (a["success"][np.asarray(cells) > 0] == 0).any()
        assert a["success"][-1] == 0
    # an isotherm search without a bracket (m_sigma = 0): NaN, no trap, success = 0
    case = fc.seeded_case(4, [12, 9], {"surface_tension": "CompressedFilmRuehl"}, bad_rows=False)
    case["f_org"][:] = 0.5
    case["formulae"] = Formulae(constants={**fc.CONSTANTS, "RUEHL_m_sigma": 0.0, "RUEHL_C0": 1e3},
                                surface_tension="CompressedFilmRuehl")
    a = fc.run_case(hip_engine, case, adaptive=False)
    assert a["success"].tolist() == [0, 0]
    _bitwise(a, fc.run_case(_checker_engine(), case, adaptive=False), "no isotherm bracket")
    # the context is usable afterwards
    case = fc.seeded_case(6, [10, 20], fc.SETS["lowe2019"]["options"])
    assert fc.run_case(hip_engine, case, adaptive=True)["success"].tolist() == [1, 1]


def test_hip_needs_the_reynolds_number_with_ventilation(hip_engine):
    case = fc.seeded_case(7, [5], {"ventilation": "PruppacherAndRasmussen1979"})
    with pytest.raises(RuntimeError, match="reynolds_number"):
        fc.run_case(hip_engine, {**case, "reynolds_number": None}, adaptive=False)


def _ambient(backend, g, pvs=None, sgm=None, hygro=None):
    st = lambda a: backend.Storage.from_ndarray(np.array(a))  # noqa: E731
    if pvs is not None:
        n = g["rhod"].shape[0]
        T, p, RH = st(np.zeros(n)), st(np.zeros(n)), st(np.zeros(n))
        backend.temperature_pressure_rh(rhod=st(g["rhod"]), thd=st(g["thd"]),
                                        water_vapour_mixing_ratio=st(g["qv"]), T=T, p=p, RH=RH)
        return {"T": T.to_ndarray(), "p": p.to_ndarray(), "RH": RH.to_ndarray()}
    v_cr = st(np.zeros(g["kappa"].shape[0]))
    backend.critical_volume(v_cr=v_cr, kappa=st(g["kappa"]), f_org=st(g["f_org"]),
                            v_dry=st(g["v_dry"]), v_wet=st(g["v_wet"]), T=st(g["T"]),
                            cell=st(g["cell"]))
    return {"v_cr": v_cr.to_ndarray()}


def test_hip_ambient_methods(hip_backend_class):
    g = cc.gold("condf_ambient")
    for choice in fc.PVS_CHOICES[1:]:
        options = {"saturation_vapour_pressure": choice}
        out = _ambient(hip_backend_class(fc.formulae_for(options)), g, pvs=choice)
        ref = _ambient(_checker_backend(options), g, pvs=choice)
        for key, value in out.items():
            np.testing.assert_array_equal(value.view(np.uint8), ref[key].view(np.uint8),
                                          err_msg=f"{key} {choice}")
            np.testing.assert_allclose(value, g[f"{key}/{choice}"], rtol=1e-12, atol=0)
    for sgm in fc.SGM_CHOICES:
        for hygro in fc.HYGRO_CHOICES:
            if (sgm, hygro) == (fc.SGM_CHOICES[0], fc.HYGRO_CHOICES[0]):
                continue  # (the default symbol: tests/test_hip_condensation.py)
            options = {"surface_tension": sgm, "hygroscopicity": hygro}
            out = _ambient(hip_backend_class(fc.formulae_for(options)), g)["v_cr"]
            ref = _ambient(_checker_backend(options), g)["v_cr"]
            np.testing.assert_array_equal(out.view(np.uint8), ref.view(np.uint8),
                                          err_msg=f"{sgm} {hygro}")


def test_runner_steps_a_population_with_the_ventilated_set(hip_engine):
    """CondensationRunner / AmbientColumns with f_org and the Reynolds number fed from
    sdm_reynolds_number: HIP and the checker engines leave the same bits"""
    from pysdm_amd.condensation import (  # pylint: disable=import-outside-toplevel
        AmbientColumns, CondensationRunner, CondensationSetup)
    from pysdm_amd.population import Population  # pylint: disable=import-outside-toplevel
    from pysdm_amd.terminal_velocity import RogersYau  # pylint: disable=import-outside-toplevel

    options = {**fc.SETS["ventilated"]["options"], "drop_growth": "Howell1949",
               "surface_tension": "CompressedFilmOvadnevaite"}
    case = fc.seeded_case(41, [300, 64, 1200, 37], options, bad_rows=False)
    results = []
    for engine in (hip_engine, _checker_engine()):
        formulae = fc.formulae_for(options)
        cell_id = np.empty(case["n_sd"], dtype=np.int64)
        for cell in range(case["n_cell"]):
            cell_id[case["idx"][case["cell_start"][cell]:case["cell_start"][cell + 1]]] = cell
        population = Population(engine, multiplicity=case["multiplicity"],
                                mass=case["water_mass"], cell_id=cell_id, n_cell=case["n_cell"])
        ambient = AmbientColumns(engine, formulae, rhod=case["rhod"], thd=case["thd"],
                                 qv=case["water_vapour_mixing_ratio"])
        runner = CondensationRunner(
            population, ambient, CondensationSetup(rtol_thd=1e-9), timestep=1.0, dv=1e6,
            dry_volume=case["vdry"], kappa=case["kappa"], f_org=case["f_org"],
            terminal_velocity=RogersYau())
        for sign in (1, -1):
            engine.assign(ambient.pthd, engine.upload(case["thd"] + sign * 0.1))
            runner.step()
        snapshot = runner.snapshot()
        snapshot["reynolds_number"] = engine.download(runner.reynolds_number)
        results.append(snapshot)
    assert results[0]["reynolds_number"].max() > 1
    for key, value in results[0].items():
        np.testing.assert_array_equal(np.asarray(value).view(np.uint8),
                                      np.asarray(results[1][key]).view(np.uint8), err_msg=key)

"""Condensation with non-default formulae on the CPU: the checker of
include/sdm_condensation_formulae.h (tests/condensation_formulae_checker/) behind the PySDM-shaped
backend class reproduces the goldens recorded from the reference
(tests/golden/gen_condensation_formulae_golden.py) for every choice of every option and for three
combined sets; `Formulae` accepts the choices and `check_formulae` maps them to the descriptor;
what is not served is still refused, naming the option.  No GPU needed."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from pysdm_amd import abi
from pysdm_amd.condensation import (FORMULAE_CONSTANT_NAMES, OPTION_ORDER, check_formulae,
                                    descriptor_of, is_default)
from pysdm_amd.formulae import Formulae
from pysdm_amd.physics.condensation_formulae import CHOICES, HOST_REFUSED
from tests import condensation_cases as cc
from tests import condensation_formulae_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = os.environ.get("PYSDM_REFERENCE", "")
NON_DEFAULT = [(option, choice) for option, choices in CHOICES.items() for choice in choices[1:]]
REFUSED = [(option, choice) for option, choices in HOST_REFUSED.items() for choice in choices]
SERVED = [pair for pair in NON_DEFAULT if pair not in REFUSED]


def checker_for(name_or_options):
    from tests.condensation_formulae_checker import CheckerBackend  # pylint: disable=import-outside-toplevel

    return CheckerBackend(fc.formulae_for(name_or_options))


# ---- the goldens ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.GOLDENS))
def test_checker_reproduces_recorded_calls(name):
    """every recorded call: integers exactly, floats within four times the measured difference"""
    from tests.condensation_formulae_checker import CheckerBackend, CheckerEngine  # pylint: disable=import-outside-toplevel

    data = cc.gold(f"condf_{name}")
    for call in range(int(data["n_calls"])):
        out = fc.replay(CheckerBackend, CheckerEngine.get(), name, data, call)
        print(name, call, fc.worst_relative_difference(out, data, call))
        fc.assert_matches_golden(out, data, call, name)


def test_measured_differences_are_explained():
    """a set may need more than the default path's tolerance only for the water mass (TOMS748's
    own rtol_x on x: NumPy's exp / log / power in the reference are not correctly rounded) and
    for what the masses feed back into"""
    assert set(fc.MEASURED) - {"_about"} == set(fc.GOLDENS)
    for name in fc.GOLDENS:
        assert fc.golden_rtol(name, "water_mass") <= 4 * cc.GOLDEN_RTOL["water_mass"], name
        for key in ("pthd", "predicted_water_vapour_mixing_ratio", "RH_max"):
            # |ln m| ~ 35 times rtol_x on a droplet's mass, diluted by the cell's vapour budget
            assert fc.golden_rtol(name, key) <= 1e-7, (name, key)


def test_goldens_cover_what_they_are_for():
    for name in fc.SETS:
        data = cc.gold(f"condf_{name}")
        assert int(data["n_calls"]) == 2 and data["calls/adaptive"].tolist() == [1, 0]
        n_sub = data["calls/out_n_substeps"]
        assert (n_sub[0] == -1).sum() == 2, name  # the two empty cells are untouched
        assert len(set(n_sub[0].tolist())) >= 3, name  # the adaptivity does something
        f_org, re = data["calls/f_org"][0], data["calls/reynolds_number"][0]
        assert (f_org == 0).any() and (f_org == 1).any() and ((f_org > 0) & (f_org < 1)).any()
        assert (re == 0).any() and re.max() > 100
        assert data["calls/out_success"][:, n_sub[0] != -1].all(), name
    fail = cc.gold("condf_bracket_fail")
    assert fail["calls/out_success"].tolist() == [[0]]
    parcel = cc.gold("condf_parcel_lowe2019")
    assert parcel["calls/out_n_activating"].max() > 0
    assert (parcel["f_org"] > 0).all()


def test_checker_ambient_methods_match_goldens():
    """temperature_pressure_rh per saturation vapour pressure, critical_volume per surface tension
    and hygroscopicity; the default path's bound (tests/test_condensation_checker.py), except the
    compressed film of Ruehl, whose isotherm root is only known to its search's rtol = 1e-6: per
    row, what that leaves open in sigma (tests/condensation_regime_cases.py), once for either side"""
    from tests import condensation_regime_cases as rc  # pylint: disable=import-outside-toplevel

    g = cc.gold("condf_ambient")
    searched = rc.ruehl_v_cr_rtol(g["T"][g["cell"]], g["v_wet"], g["v_dry"], g["f_org"])
    assert 0 < searched.max() < 1e-6
    for choice in fc.PVS_CHOICES:
        backend = checker_for({"saturation_vapour_pressure": choice})
        st = lambda a: backend.Storage.from_ndarray(np.array(a))  # noqa: E731
        n = g["rhod"].shape[0]
        T, p, RH = st(np.zeros(n)), st(np.zeros(n)), st(np.zeros(n))
        backend.temperature_pressure_rh(rhod=st(g["rhod"]), thd=st(g["thd"]),
                                        water_vapour_mixing_ratio=st(g["qv"]), T=T, p=p, RH=RH)
        for key, value in (("T", T), ("p", p), ("RH", RH)):
            np.testing.assert_allclose(value.to_ndarray(), g[f"{key}/{choice}"], rtol=1e-12,
                                       atol=0, err_msg=f"{key} {choice}")
    for sgm in fc.SGM_CHOICES:
        for hygro in fc.HYGRO_CHOICES:
            backend = checker_for({"surface_tension": sgm, "hygroscopicity": hygro})
            st = lambda a: backend.Storage.from_ndarray(np.array(a))  # noqa: E731
            v_cr = st(np.zeros(g["kappa"].shape[0]))
            backend.critical_volume(v_cr=v_cr, kappa=st(g["kappa"]), f_org=st(g["f_org"]),
                                    v_dry=st(g["v_dry"]), v_wet=st(g["v_wet"]), T=st(g["T"]),
                                    cell=st(g["cell"]))
            ref = g[f"v_cr/{sgm}/{hygro}"]
            got = v_cr.to_ndarray()
            with np.errstate(invalid="ignore"):
                print(sgm, hygro, np.nanmax(np.abs(got - ref) / np.abs(ref)))
            # v_cr ~ sigma ** -1.5; sigma is linear in 1 / f_surf, known to 1e-6 on both sides
            rtol = 1e-12 + (2 * searched if sgm == "CompressedFilmRuehl" else 0)
            assert (np.abs(got - ref) <= rtol * np.abs(ref)).all(), f"{sgm} {hygro}"


# ---- Formulae and the descriptor ------------------------------------------------------------------
@pytest.mark.parametrize("option,choice", REFUSED)
def test_choices_refused_through_formulae_have_a_descriptor(option, choice):
    """the four choices whose refusal through `Formulae` the suite pins: still refused there,
    naming the option, and served by the library through `descriptor_of`"""
    formulae = Formulae(constants=dict(fc.CONSTANTS))
    if option != "diffusion_coordinate":  # (Formulae accepts WaterMass for deposition)
        with pytest.raises(NotImplementedError, match=option):
            Formulae(**{option: choice})
    setattr(formulae, option, SimpleNamespace(__name__=choice))
    with pytest.raises(NotImplementedError, match=option):
        check_formulae(formulae)
    descriptor = descriptor_of({option: choice}, formulae.constants)
    expected = [0] * 10
    expected[OPTION_ORDER.index(option)] = CHOICES[option].index(choice)
    assert list(descriptor.option) == expected
    with pytest.raises(NotImplementedError, match=option):
        descriptor_of({option: "NoSuchChoice"}, formulae.constants)


@pytest.mark.parametrize("option,choice", SERVED)
def test_every_choice_constructs_and_maps_to_the_descriptor(option, choice):
    formulae = Formulae(constants=dict(fc.CONSTANTS), **{option: choice})
    assert getattr(formulae, option).__name__ == choice
    descriptor = check_formulae(formulae)
    assert isinstance(descriptor, abi.CondFormulae) and not is_default(descriptor)
    expected = [0] * 10
    expected[OPTION_ORDER.index(option)] = CHOICES[option].index(choice)
    assert list(descriptor.option) == expected
    for at, name in enumerate(FORMULAE_CONSTANT_NAMES):
        assert descriptor.consts[at] == getattr(formulae.constants, name), name
    # a PySDM-style formulae object is read by `__name__` too
    foreign = Formulae(constants=dict(fc.CONSTANTS))
    setattr(foreign, option, SimpleNamespace(__name__=choice))
    assert list(check_formulae(foreign).option) == expected


def test_default_formulae_give_the_default_descriptor():
    assert is_default(check_formulae(Formulae()))
    assert len(FORMULAE_CONSTANT_NAMES) == 72 == len(abi.CondFormulae().consts)


def test_descriptor_matches_the_header():
    """option and constant indices of the header are the places of the Python tables"""
    import re  # pylint: disable=import-outside-toplevel

    with open(abi.CONDENSATION_FORMULAE_HEADER_PATH, encoding="utf-8") as header:
        text = header.read()
    defines = {k: int(v) for k, v in re.findall(r"#define (SDM_COND_\w+) (\d+)", text)}
    for at, option in enumerate(OPTION_ORDER):
        assert defines[f"SDM_COND_OPT_{option.upper()}"] == at
    assert defines["SDM_COND_N_OPTS"] == len(OPTION_ORDER)
    assert defines["SDM_COND_F_N_CONSTS"] == len(FORMULAE_CONSTANT_NAMES)
    for name, index in (("sgm_org", "SGM_ORG"), ("N_A", "N_A"), ("ARM_C1", "ARM_C1"),
                        ("B80W_G0", "B80W_G0"), ("L77W_A0", "L77W_A0"),
                        ("MK05_LIQ_C1", "MK05_LIQ_C1"), ("W76W_G0", "W76W_G0"),
                        ("one_kelvin", "ONE_KELVIN"), ("p_STP", "P_STP"),
                        ("diffusion_thermics_D_G11_A", "D_G11_A"),
                        ("diffusion_thermics_K_G11_A", "K_G11_A"), ("dv_pk05", "DV_PK05"),
                        ("PRUPPACHER_RASMUSSEN_1979_XTHRES", "PR79_XTHRES"),
                        ("ONE_HALF", "ONE_HALF")):
        assert FORMULAE_CONSTANT_NAMES.index(name) == defines[f"SDM_COND_F_{index}"], name
    enums = re.findall(r"enum sdm_cond_(\w+) \{([^}]*)\}", text)
    assert [name for name, _ in enums] == list(OPTION_ORDER)
    for option, body in enums:
        codes = [int(v) for v in re.findall(r"= (\d+)", body)]
        assert codes == list(range(len(CHOICES[option]))), option
        names = [n.split("_", 3)[3].replace("_", "").lower()
                 for n in re.findall(r"(SDM_COND_\w+) =", body)]
        assert names == [c.lower() for c in CHOICES[option]], option


@pytest.mark.parametrize("option,value", [("drop_growth", "Jeffery"),
                                          ("surface_tension", "CompressedFilm"),
                                          ("state_variable_triplet", "Other"),
                                          ("air_dynamic_viscosity", "Sutherland")])
def test_unknown_choices_are_refused(option, value):
    with pytest.raises(NotImplementedError, match=option):
        Formulae(**{option: value})
    formulae = Formulae()
    setattr(formulae, option, SimpleNamespace(__name__=value))
    with pytest.raises(NotImplementedError, match=option):
        check_formulae(formulae)


def test_mixed_phase_and_bad_constants_are_refused():
    with pytest.raises(NotImplementedError, match="particle_shape_and_density"):
        check_formulae(Formulae(particle_shape_and_density="MixedPhaseSpheres",
                                surface_tension="CompressedFilmOvadnevaite",
                                constants=dict(fc.CONSTANTS)))
    with pytest.raises(NotImplementedError, match="surface_tension.*delta_min"):
        Formulae(surface_tension="CompressedFilmOvadnevaite",
                 constants={**fc.CONSTANTS, "delta_min": math.inf})
    with pytest.raises(NotImplementedError, match="surface_tension.*sgm_org"):
        Formulae(surface_tension="CompressedFilmOvadnevaite")
    with pytest.raises(NotImplementedError, match="RUEHL_m_sigma"):
        Formulae(surface_tension="CompressedFilmRuehl",
                 constants={**fc.CONSTANTS, "RUEHL_m_sigma": math.nan})
    Formulae(surface_tension="SzyszkowskiLangmuir",  # (does not read m_sigma)
             constants={**fc.CONSTANTS, "RUEHL_m_sigma": math.nan})
    with pytest.raises(ValueError, match="dv_pk05"):
        Formulae(diffusion_kinetics="LoweEtAl2019", constants={"dv_pk05": 1e-7})
    odd = Formulae()
    odd.constants.dv_pk05 = 1e-7
    odd.diffusion_kinetics = SimpleNamespace(__name__="LoweEtAl2019")
    with pytest.raises(ValueError, match="dv_pk05"):
        check_formulae(odd)


def test_constants_override_reaches_the_library():
    from tests.condensation_formulae_checker import CheckerEngine  # pylint: disable=import-outside-toplevel

    options = {"surface_tension": "CompressedFilmOvadnevaite"}
    case = fc.seeded_case(3, [40, 0, 33], options)
    plain = cc.run_case(CheckerEngine.get(), case, adaptive=True)
    case["formulae"] = Formulae(constants={**fc.CONSTANTS, "sgm_org": 0.03}, **options)
    other = cc.run_case(CheckerEngine.get(), case, adaptive=True)
    assert (plain["water_mass"] != other["water_mass"]).any()


def test_host_side_formulae_agree_with_the_reference():
    """surface_tension.sigma, hygroscopicity.r_cr and saturation_vapour_pressure.pvs_water of the
    option objects, against what the reference's critical_volume / RH were computed from"""
    from tests import condensation_regime_cases as rc  # pylint: disable=import-outside-toplevel

    g = cc.gold("condf_ambient")
    base = Formulae()
    pv = g[f"RH/{fc.PVS_CHOICES[0]}"] * base.saturation_vapour_pressure.pvs_water(g["T"])
    for choice in fc.PVS_CHOICES:
        formulae = Formulae(saturation_vapour_pressure=choice)
        np.testing.assert_allclose(pv / formulae.saturation_vapour_pressure.pvs_water(g["T"]),
                                   g[f"RH/{choice}"], rtol=1e-12, err_msg=choice)
    T = g["T"][g["cell"]]
    for sgm in fc.SGM_CHOICES:
        formulae = fc.formulae_for({"surface_tension": sgm})
        sigma = formulae.surface_tension.sigma(T, g["v_wet"], g["v_dry"], g["f_org"])
        r_cr = formulae.hygroscopicity.r_cr(g["kappa"], g["v_dry"] / formulae.constants.PI_4_3,
                                            T, sigma)
        ref = g[f"v_cr/{sgm}/KappaKoehlerLeadingTerms"]
        # (the host side bisects the isotherm to the last bit: only the reference's search is open)
        rtol = 1e-10 + (rc.ruehl_v_cr_rtol(T, g["v_wet"], g["v_dry"], g["f_org"])
                        if sgm == "CompressedFilmRuehl" else 0)
        assert (np.abs(formulae.trivia.volume(r_cr) - ref) <= rtol * np.abs(ref)).all(), sgm


# ---- the solver's own edge ------------------------------------------------------------------------
def _ruehl_case():
    case = fc.seeded_case(4, [12, 9], {"surface_tension": "CompressedFilmRuehl"}, bad_rows=False)
    case["f_org"][:] = 0.5
    return case


def test_ruehl_search_without_a_bracket_fails_the_cell_and_does_not_trap():
    """m_sigma = 0 (finite: the constructor's check passes) makes the isotherm's right-hand side 1
    for every f_surf, so its search has no sign change: NaN from TOMS748, through np.maximum /
    np.minimum into RH_eq, and the droplet's own bracket search gives up (success = 0)"""
    from tests.condensation_formulae_checker import CheckerEngine  # pylint: disable=import-outside-toplevel

    case = _ruehl_case()
    case["formulae"] = Formulae(constants={**fc.CONSTANTS, "RUEHL_m_sigma": 0.0,
                                           "RUEHL_C0": 1e3},
                                surface_tension="CompressedFilmRuehl")
    before = case["water_mass"].copy()
    out = cc.run_case(CheckerEngine.get(), case, adaptive=False)
    assert out["success"].tolist() == [0, 0]
    np.testing.assert_array_equal(out["water_mass"], before)


def test_ruehl_search_running_out_of_iterations_fails_the_cell(tmp_path):
    """where the reference's CompressedFilmRuehl asserts `iters != max_iters` the droplet counts as
    failed.  100 iterations are out of reach of a superlinear search on this isotherm, so the
    checker is built once more with a cap of 2: the same case that succeeds with the real cap
    fails with this one, and nothing traps"""
    import subprocess  # pylint: disable=import-outside-toplevel

    from oracle import engine as oracle_engine  # pylint: disable=import-outside-toplevel
    from tests import condensation_formulae_checker as checker  # pylint: disable=import-outside-toplevel

    case = _ruehl_case()
    engine = checker.CheckerEngine.get()
    assert cc.run_case(engine, case, adaptive=False)["success"].tolist() == [1, 1]
    lib = str(tmp_path / "libcapped.so")
    subprocess.check_call(["gcc", *oracle_engine._FLAGS, "-DCF_RUEHL_MAX_ITERS=2", "-o", lib,  # pylint: disable=protected-access
                           checker.SOURCE, "-lm"])
    real = engine.condensation_formulae_library
    engine.condensation_formulae_library = abi.Library(
        lib, "the formulae checker with a capped isotherm search",
        header=abi.CONDENSATION_FORMULAE_HEADER_PATH)
    try:
        before = case["water_mass"].copy()
        out = cc.run_case(engine, case, adaptive=False)
    finally:
        engine.condensation_formulae_library = real
    assert out["success"].tolist() == [0, 0]
    np.testing.assert_array_equal(out["water_mass"], before)
    assert out["n_activating"].tolist() == [0, 0]


# ---- an unmodified PySDM on the plug-in class -------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "PySDM")),
                    reason="reference tree not named by PYSDM_REFERENCE")
def test_pysdm_parcel_with_the_lowe2019_set_runs_on_the_checker_class():
    """an unmodified PySDM Parcel + AmbientThermodynamics + Condensation under
    Formulae(surface_tension=..., ...) on the checker-bound class reproduces the recorded run"""
    os.environ.setdefault("CI", "1")
    added = [os.path.join(HERE, "golden", "standins"), REFERENCE]
    sys.path[:0] = added
    try:
        from PySDM import Builder  # pylint: disable=import-outside-toplevel,import-error
        from PySDM import Formulae as PySDMFormulae  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.dynamics import AmbientThermodynamics, Condensation  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.environments import Parcel  # pylint: disable=import-outside-toplevel,import-error
    except Exception as error:  # pylint: disable=broad-except
        pytest.skip(f"PySDM not importable here: {error}")
    finally:
        for path in added:
            sys.path.remove(path)
    from pysdm_amd.pysdm_plugin import as_pysdm_backend  # pylint: disable=import-outside-toplevel
    from tests.condensation_formulae_checker import CheckerBackend  # pylint: disable=import-outside-toplevel

    gold = cc.gold("condf_parcel_lowe2019")
    cfg = {k[len("parcel/"):]: gold[k] for k in gold.files if k.startswith("parcel/")}
    formulae = PySDMFormulae(constants=dict(fc.CONSTANTS), **fc.GOLDENS["parcel_lowe2019"])
    backend = as_pysdm_backend(CheckerBackend)(formulae)
    env = Parcel(dt=float(cfg["dt"]), mass_of_dry_air=float(cfg["mass_of_dry_air"]),
                 p0=float(cfg["p0"]), initial_water_vapour_mixing_ratio=float(cfg["qv0"]),
                 T0=float(cfg["T0"]), w=float(cfg["w"]))
    builder = Builder(n_sd=int(cfg["n_sd"]), backend=backend, environment=env)
    builder.add_dynamic(AmbientThermodynamics())
    builder.add_dynamic(Condensation())
    attributes = {k[len("init/"):]: np.array(gold[k]) for k in gold.files
                  if k.startswith("init/")}
    particulator = builder.build(attributes=attributes, products=())
    for call in range(int(cfg["n_steps"])):
        particulator.run(steps=1)
        cond = particulator.dynamics["Condensation"]
        for key in cc.COUNTERS:
            np.testing.assert_array_equal(cond.counters[key].to_ndarray(),
                                          gold[f"calls/out_{key}"][call], err_msg=key)
        mass = particulator.attributes["signed water mass"].to_ndarray(raw=True)
        np.testing.assert_allclose(mass, gold["calls/out_water_mass"][call],
                                   rtol=fc.golden_rtol("parcel_lowe2019", "water_mass"), atol=0)

"""The condensation path on the CPU: the checker of include/sdm_condensation.h
(tests/checker/condensation_checker.c) behind the PySDM-shaped backend class reproduces the
goldens recorded from the reference (tests/golden/gen_condensation_golden.py); non-default
formulae are refused.  No GPU needed."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from pysdm_amd.condensation import CondensationSetup, check_formulae
from pysdm_amd.formulae import Formulae
from tests import condensation_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"


@pytest.fixture(scope="module", name="checker")
def checker_backend():
    from tests.checker import CheckerBackend  # pylint: disable=import-outside-toplevel

    return CheckerBackend()


@pytest.mark.parametrize("name", ["cond_box", "cond_parcel_a1", "cond_parcel_a0"])
def test_checker_reproduces_recorded_calls(checker, name):
    data = cc.gold(name)
    for call in range(int(data["n_calls"])):
        cc.assert_matches_golden(cc.replay(checker, data, call), data, call)


def test_goldens_cover_activation_substeps_and_empty_cells():
    parcel = cc.gold("cond_parcel_a1")
    assert parcel["calls/out_n_activating"].max() > 0
    assert parcel["calls/out_n_substeps"].max() > 1
    box = cc.gold("cond_box")
    assert (box["calls/out_n_substeps"] == -1).any()  # empty cells untouched
    assert len(set(box["calls/out_n_substeps"][0].tolist())) > 3


def _ambient(backend):
    g = cc.gold("cond_ambient")
    S = backend.Storage
    st = lambda a: S.from_ndarray(np.array(a))  # noqa: E731
    n = g["rhod"].shape[0]
    T, p, RH = st(np.zeros(n)), st(np.zeros(n)), st(np.zeros(n))
    backend.temperature_pressure_rh(rhod=st(g["rhod"]), thd=st(g["thd"]),
                                    water_vapour_mixing_ratio=st(g["qv"]), T=T, p=p, RH=RH)
    rho, eta = st(np.zeros(n)), st(np.zeros(n))
    backend.air_density(output=rho, rhod=st(g["rhod"]), water_vapour_mixing_ratio=st(g["qv"]))
    backend.air_dynamic_viscosity(output=eta, temperature=T)
    m = g["kappa"].shape[0]
    v_cr, re = st(np.zeros(m)), st(np.zeros(m))
    backend.critical_volume(v_cr=v_cr, kappa=st(g["kappa"]), f_org=st(g["f_org"]),
                            v_dry=st(g["v_dry"]), v_wet=st(g["v_wet"]), T=T, cell=st(g["cell"]))
    backend.reynolds_number(output=re, cell_id=st(g["cell"]), dynamic_viscosity=eta,
                            density=rho, radius=st(g["radius"]),
                            velocity_wrt_air=st(g["velocity_wrt_air"]))
    y = st(g["euler_y0"])
    backend.explicit_euler(y, float(g["euler_dt"]), float(g["euler_dy_dt"]))
    out = {"T": T, "p": p, "RH": RH, "air_density": rho, "air_dynamic_viscosity": eta,
           "v_cr": v_cr, "reynolds_number": re, "euler_y": y}
    return g, {k: v.to_ndarray() for k, v in out.items()}


def test_checker_ambient_methods_match_goldens(checker):
    g, out = _ambient(checker)
    for key, value in out.items():
        np.testing.assert_allclose(value, g[key], rtol=1e-12, atol=0, err_msg=key)


@pytest.mark.parametrize("option,value", [("drop_growth", "Fick"),
                                          ("ventilation", "Froessling1938"),
                                          ("diffusion_kinetics", "Neglect"),
                                          ("surface_tension", "CompressedFilmOvadnevaite")])
def test_non_default_formulae_are_refused(option, value):
    with pytest.raises(NotImplementedError, match=option):
        Formulae(**{option: value})
    formulae = Formulae()
    setattr(formulae, option, SimpleNamespace(__name__=value))
    with pytest.raises(NotImplementedError, match=option):
        check_formulae(formulae)


def test_solver_refuses_what_the_reference_refuses(checker):
    with pytest.raises(NotImplementedError):
        checker.make_condensation_solver(1.0, 1, dt_range=(0, 1.0), adaptive=True, fuse=32,
                                         multiplier=2, RH_rtol=1e-7, max_iters=16)
    with pytest.raises(ValueError):
        checker.make_condensation_solver(1.0, 1, dt_range=(1e-4, 1.0), adaptive=True, fuse=32,
                                         multiplier=2.0, RH_rtol=1e-7, max_iters=16)
    with pytest.raises(ValueError):
        CondensationSetup(adaptive=True, substeps=3)


def test_checker_bracket_failure_sets_success_zero():
    from tests.checker import CheckerEngine  # pylint: disable=import-outside-toplevel

    case = cc.seeded_case(5, [20, 30, 25, 1, 7], max_iters=4)
    out = cc.run_case(CheckerEngine.get(), case, adaptive=True)
    assert out["success"].tolist() == [0, 1, 0, 1, 1]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "PySDM")),
                    reason="reference tree not present")
def test_pysdm_parcel_runs_on_the_checker_class(checker):  # pylint: disable=unused-argument
    """an unmodified PySDM Parcel + AmbientThermodynamics + Condensation on the checker-bound
    class reproduces the recorded run"""
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
    from tests.checker import CheckerBackend  # pylint: disable=import-outside-toplevel

    gold = cc.gold("cond_parcel_a1")
    cfg = {k[len("parcel/"):]: gold[k] for k in gold.files if k.startswith("parcel/")}
    backend = as_pysdm_backend(CheckerBackend)(PySDMFormulae())
    env = Parcel(dt=float(cfg["dt"]), mass_of_dry_air=float(cfg["mass_of_dry_air"]),
                 p0=float(cfg["p0"]), initial_water_vapour_mixing_ratio=float(cfg["qv0"]),
                 T0=float(cfg["T0"]), w=float(cfg["w"]))
    builder = Builder(n_sd=int(cfg["n_sd"]), backend=backend, environment=env)
    builder.add_dynamic(AmbientThermodynamics())
    builder.add_dynamic(Condensation(adaptive=True))
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
                                   rtol=cc.GOLDEN_RTOL["water_mass"], atol=0)

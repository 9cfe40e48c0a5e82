"""The condensation path on the MI355X: include/sdm_condensation.h through libsdm_hip.so.

(i) the recorded `backend.condensation` calls of a PySDM Parcel run and of a 4 x 4-cell box,
replayed through the HIP class, reproduce what the reference returned (integers exactly, floats
within condensation_cases.GOLDEN_RTOL), (ii) HIP and the CPU checker agree bit for bit on the same
calls and on seeded multi-cell states (cells of 1, 63, 64, 65, 1024 and 4096 super-droplets, a
cell larger than one register chunk, empty cells, multiplicity-0 and water-mass <= 0 rows, failing
bracket searches), (iii) the six ambient methods agree bit for bit."""
import numpy as np
import pytest

from tests import condensation_cases as cc

pytestmark = pytest.mark.gpu
OUT_KEYS = (*cc.OUT_INTS, *cc.OUT_FLOATS)


@pytest.fixture(scope="module", name="hip")
def hip_backend(hip_backend_class):
    return hip_backend_class()


@pytest.fixture(scope="module", name="checker")
def checker_backend():
    from tests.checker import CheckerBackend  # pylint: disable=import-outside-toplevel

    return CheckerBackend()


def _bitwise(a, b, where=""):
    for key in OUT_KEYS:
        np.testing.assert_array_equal(np.asarray(a[key]).view(np.uint8),
                                      np.asarray(b[key]).view(np.uint8), err_msg=f"{where} {key}")


@pytest.mark.parametrize("name", ["cond_box", "cond_parcel_a1", "cond_parcel_a0"])
def test_hip_replays_recorded_calls(hip, checker, name):
    data = cc.gold(name)
    for call in range(int(data["n_calls"])):
        out = cc.replay(hip, data, call)
        cc.assert_matches_golden(out, data, call)
        _bitwise(out, cc.replay(checker, data, call), f"{name} call {call}")


CELLS = {
    "sizes": [1, 63, 64, 65, 0, 1024, 4096, 0, 1500, 2100, 7, 1025],
    "small": [3, 0, 5, 1, 2, 0, 9],
    "one_big": [5000],
}


@pytest.mark.parametrize("adaptive", [True, False])
@pytest.mark.parametrize("layout", sorted(CELLS))
def test_hip_equals_checker_bitwise(adaptive, layout, hip_engine):
    from tests.checker import CheckerEngine  # pylint: disable=import-outside-toplevel

    case = cc.seeded_case(17 + len(layout), CELLS[layout])
    a = cc.run_case(hip_engine, case, adaptive=adaptive)
    b = cc.run_case(CheckerEngine.get(), case, adaptive=adaptive)
    _bitwise(a, b, layout)
    counts = np.asarray(CELLS[layout])
    assert (a["success"][counts > 0] == 1).all()
    assert (a["n_substeps"][counts == 0] == (-1 if adaptive else 3)).all()  # untouched


def test_hip_failed_brackets_give_success_zero_and_no_fault(hip_engine):
    from tests.checker import CheckerEngine  # pylint: disable=import-outside-toplevel

    for adaptive in (True, False):
        case = cc.seeded_case(5, [20, 30, 25, 1, 7, 0, 300, 1100], max_iters=4)
        a = cc.run_case(hip_engine, case, adaptive=adaptive)
        b = cc.run_case(CheckerEngine.get(), case, adaptive=adaptive)
        _bitwise(a, b, f"adaptive={adaptive}")
        assert (a["success"][[0, 1, 2, 3, 4, 6, 7]] == 0).any()
    # the context is usable afterwards
    case = cc.seeded_case(6, [10, 20])
    assert cc.run_case(hip_engine, case, adaptive=True)["success"].tolist() == [1, 1]


def test_hip_keeps_calling_with_the_previous_substep_counts(hip_engine):
    """n_substeps is read as the previous call's count (adapt_substeps starts from n // 2)"""
    from tests.checker import CheckerEngine  # pylint: disable=import-outside-toplevel

    case = cc.seeded_case(23, [40, 70, 0, 130])
    n_in = np.asarray([64, 3, 7, 1000], dtype=np.int64)
    a = cc.run_case(hip_engine, case, adaptive=True, n_substeps_in=n_in)
    b = cc.run_case(CheckerEngine.get(), case, adaptive=True, n_substeps_in=n_in)
    _bitwise(a, b)


def test_hip_ambient_methods(hip, checker):
    from tests.test_condensation_checker import _ambient  # pylint: disable=import-outside-toplevel

    g, out = _ambient(hip)
    _, ref = _ambient(checker)
    for key, value in out.items():
        np.testing.assert_array_equal(value.view(np.uint8), ref[key].view(np.uint8), err_msg=key)
        np.testing.assert_allclose(value, g[key], rtol=1e-12, atol=0, err_msg=key)


def _flow_run(engine, n_steps=3):
    """the 2-D kinematic population (pysdm_amd.cases.make_kinematic_flow): per time step
    condensation, then displacement, then collision"""
    from pysdm_amd.cases import make_kinematic_flow  # pylint: disable=import-outside-toplevel
    from pysdm_amd.condensation import (  # pylint: disable=import-outside-toplevel
        AmbientColumns, CondensationRunner, CondensationSetup)
    from pysdm_amd.formulae import Formulae  # pylint: disable=import-outside-toplevel

    grid, size, dt = (4, 4), (1500.0, 1500.0), 5.0
    displacement, collisions = make_kinematic_flow(engine, n_sd=4096, grid=grid, size=size, dt=dt)
    population = collisions.population
    n_cell, n_sd = population.n_cell, population.n_sd
    case = cc.seeded_case(31, np.full(n_cell, n_sd // n_cell))
    rng = np.random.default_rng(3)
    ambient = AmbientColumns(engine, Formulae(), rhod=case["rhod"], thd=case["thd"],
                             qv=case["water_vapour_mixing_ratio"])
    runner = CondensationRunner(
        population, ambient, CondensationSetup(rtol_thd=1e-9), timestep=dt,
        dv=float(np.prod(np.asarray(size) / np.asarray(grid))),
        dry_volume=cc.const.PI_4_3 * (0.05e-6 * rng.uniform(0.5, 2, n_sd)) ** 3,
        kappa=rng.uniform(0.5, 1.3, n_sd))
    snapshots = []
    for step in range(n_steps):
        # the Eulerian step's predictions (prescribed here): a warming / drying or the opposite
        sign = 1 if step % 2 else -1
        engine.assign(ambient.pthd, engine.upload(case["thd"] + sign * 0.3))
        engine.assign(ambient.pqv, engine.upload(case["water_vapour_mixing_ratio"]
                                                 * (1 - sign * 2e-3)))
        runner.step()
        displacement.run()
        collisions.run(1)
        snapshots.append({**{f"cond/{k}": v for k, v in runner.snapshot().items()},
                          **population.snapshot()})
    return snapshots


def test_condensation_displacement_collision_flow(hip_engine):
    from tests.checker import CheckerEngine  # pylint: disable=import-outside-toplevel

    hip, ref = _flow_run(hip_engine), _flow_run(CheckerEngine.get())
    for step, (a, b) in enumerate(zip(hip, ref)):
        length = int(a["length"])
        assert length == int(b["length"])
        for key, value in a.items():
            other = b[key]
            if key == "idx":
                value, other = value[:length], other[:length]
            np.testing.assert_array_equal(np.atleast_1d(value).view(np.uint8),
                                          np.atleast_1d(other).view(np.uint8),
                                          err_msg=f"step {step}: {key}")
    assert hip[-1]["cond/success"].all()

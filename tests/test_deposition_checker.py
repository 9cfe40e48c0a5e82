"""Vapour deposition on ice on the CPU: the checker of include/sdm_deposition.h
(tests/deposition_checker) behind the very host code the HIP backend runs.

(i) the checker-bound backend class replays the 8 recorded calls of dep_methods.npz within the
tolerances of tests/deposition_cases.py, rows and cells the reference left alone bit for bit,
(ii) the 20 recorded consecutive calls of dep_steps.npz are reproduced by `DepositionRunner`, call
by call, (iii) the blocked sum stays within the summation bound of the ordered one with identical
masses, (iv) no-op inputs keep every bit, (v) the rows for which the reference asserts are counted
and reported, (vi) aliased predicted arrays are refused, (vii) `Formulae` accepts the new options
and refuses others by name, (viii) an unmodified PySDM `Builder` + `VapourDepositionOnIce()`
runs on the class where PySDM is importable."""
import ctypes

import numpy as np
import pytest

from pysdm_amd import deposition as dep
from pysdm_amd.condensation import check_formulae as condensation_check_formulae
from pysdm_amd.formulae import Formulae
from tests import deposition_cases as dc

METHODS = dc.gold("dep_methods")
STEPS = dc.gold("dep_steps")


@pytest.fixture(scope="module", name="backend_class")
def checker_backend_class():
    from tests.deposition_checker import DepositionCheckerBackend  # pylint: disable=import-outside-toplevel

    return DepositionCheckerBackend


@pytest.fixture(scope="module", name="engine")
def checker_engine():
    from tests.deposition_checker import DepositionCheckerEngine  # pylint: disable=import-outside-toplevel

    return DepositionCheckerEngine.get()


def test_binding_struct_has_the_layout_of_the_header(engine):
    from pysdm_amd.abi import DepositionCfg  # pylint: disable=import-outside-toplevel

    assert (ctypes.sizeof(DepositionCfg)
            == engine.deposition_library.cdll.deposition_checker_cfg_size())
    assert len(dep.CONSTANT_NAMES) == 39
    assert len(dep.constants_of(dc.formulae_for())) == 39


def test_golden_state_is_what_the_generator_promises():
    case, _, _ = dc.golden_case(METHODS, 0)
    s_ice = case["RH"] / case["a_w_ice"]
    ice = ~(case["signed_water_mass"] > 0)
    assert (s_ice > 1).any() and (s_ice < 1).any() and s_ice[2] == 1
    assert ice[case["cell_id"] == 2].any()       # ice in the cell at S_ice == 1
    assert not ice[case["cell_id"] == 3].any() and (case["cell_id"] == 3).any()  # no ice
    assert not (case["cell_id"] == 4).any()      # an empty cell
    assert 0.5 < ice.mean() < 0.7 and 0.02 < (case["multiplicity"] == 0).mean() < 0.08


@pytest.mark.parametrize("number", range(int(METHODS["n_calls"])))
def test_checker_replays_recorded_method_calls(backend_class, number):
    case, formulae, want = dc.golden_case(METHODS, number)
    got = dc.call_backend(backend_class, case, formulae)
    what = " ".join(str(METHODS[f"calls/{number}/{k}"])
                    for k in ("coordinate", "capacity", "kinetics"))
    worst = dc.assert_within_reference_tolerance(case, got, want, what)
    print(f"{what}: largest relative difference: masses {worst[0]:.3g}, increments "
          f"{worst[1]:.3g}")
    assert (want[0] != case["signed_water_mass"]).any()
    if "WaterMass " in what + " " and "Logarithm" not in what:  # recorded sign changes
        flipped = (case["signed_water_mass"] < 0) & (want[0] > 0)
        assert 1 <= flipped.sum() <= 20
        np.testing.assert_array_equal(got[0] > 0, want[0] > 0)


def test_runner_reproduces_recorded_consecutive_calls(engine):
    signs = []
    for step, (case, got, want, ambient, after) in enumerate(dc.replay_steps(engine, STEPS)):
        worst = dc.assert_within_reference_tolerance(case, got, want, f"step {step}")
        print(f"step {step}: masses {worst[0]:.3g}, increments {worst[1]:.3g}")
        # accept_predictions(): this project's ambient methods against the reference's (1e-12: the
        # bound of tests/test_condensation_checker.py)
        for key, value in ambient.items():
            np.testing.assert_allclose(value, after[key], rtol=1e-12, atol=0,
                                       err_msg=f"step {step} {key}")
        signs.append(np.sign(case["RH"] / case["a_w_ice"] - 1))
    signs = np.stack(signs)
    assert ((signs[1:] * signs[:-1]) < 0).any()  # a cell crosses between growth and sublimation


@pytest.mark.parametrize("seed,counts", [(1, [0, 1, 255, 256, 257, 3000, 40]),
                                         (2, [5000]), (3, [513, 0, 1024])])
def test_blocked_sum_is_within_the_summation_bound_of_the_ordered(engine, seed, counts):
    s_one = (6,) if len(counts) == 7 else ()
    case = dc.counted_case(seed, counts, liquid=500, s_one=s_one)
    formulae = dc.formulae_for()
    ordered = dc.call_engine(engine, case, formulae, "ordered")
    blocked = dc.call_engine(engine, case, formulae, "blocked")
    dc.assert_same_bits(blocked[0], ordered[0], "masses")
    assert blocked[3] == ordered[3] == 0
    n_c = np.array([0 if c in s_one else n for c, n in enumerate(counts)])
    for b, o, before in ((blocked[1], ordered[1], case["predicted_qv"]),
                         (blocked[2], ordered[2], case["predicted_thd"])):
        # twice gamma_n sum|terms|: the contributions of a cell share a sign, so sum|delta| =
        # |sum delta| up to that same rounding
        bound = 4 * n_c * 2.0 ** -53 * (np.abs(before) + np.abs(o - before))
        assert (np.abs(b - o) <= bound).all(), (np.abs(b - o), bound)
        dc.assert_same_bits(b[n_c == 0], before[n_c == 0], "cells nothing contributes to")
        assert (o[n_c > 0] != before[n_c > 0]).all()
    # up to one block the two shapes can only differ by the association inside the block
    assert (blocked[1] != ordered[1]).any() or (blocked[2] != ordered[2]).any()


@pytest.mark.parametrize("sum_mode", ["ordered", "blocked"])
def test_nothing_to_do_keeps_every_bit(engine, sum_mode):
    formulae = dc.formulae_for()
    no_ice = dc.seeded_case(4, 700, 5, ice=0.0)
    all_one = dc.seeded_case(5, 700, 5, s_one=range(5))
    assert not dc.contributing_rows(no_ice).any() and not dc.contributing_rows(all_one).any()
    assert (all_one["signed_water_mass"] < 0).any()
    empty = dc.seeded_case(6, 0, 5)
    for case in (no_ice, all_one, empty):
        mass, pqv, pthd, count = dc.call_engine(engine, case, formulae, sum_mode)
        dc.assert_same_bits(mass, case["signed_water_mass"])
        dc.assert_same_bits(pqv, case["predicted_qv"])
        dc.assert_same_bits(pthd, case["predicted_thd"])
        # (n_sd == 0 touches nothing: the count keeps what the caller put there)
        assert count == (-7 if case is empty else 0)


def test_rows_that_exceed_their_cells_vapour_are_counted_and_reported(engine, backend_class):
    case, expected = dc.exceeding_case(7)
    assert expected > 10
    formulae = dc.formulae_for()
    for sum_mode in ("ordered", "blocked"):
        assert dc.call_engine(engine, case, formulae, sum_mode)[3] == expected
    # every row is processed as if the assertion were absent
    calm = dict(case, qv=np.where(np.arange(3) == 1, 1.0, case["qv"]))
    quiet, loud = (dc.call_engine(engine, c, formulae) for c in (calm, case))
    assert quiet[3] == 0
    for a, b in zip(quiet[:3], loud[:3]):
        dc.assert_same_bits(a, b)
    dc.call_engine(engine, case, formulae, with_count=False)  # n_exceeded may be NULL
    with pytest.raises(RuntimeError, match=f"{expected} super-droplet"):
        dc.call_backend(backend_class, case, formulae)

    from pysdm_amd.condensation import AmbientColumns  # pylint: disable=import-outside-toplevel
    from pysdm_amd.population import Population  # pylint: disable=import-outside-toplevel

    population = Population(engine, multiplicity=np.maximum(case["multiplicity"], 1),
                            mass=case["signed_water_mass"], cell_id=case["cell_id"], n_cell=3)
    ambient = AmbientColumns(engine, formulae, rhod=case["rhod"], thd=case["thd"],
                             qv=case["qv"], mixed_phase=True)
    engine.assign(ambient.RH, engine.upload(1.1 * engine.download(ambient.a_w_ice)))
    for sum_mode in ("ordered", "blocked"):
        runner = dep.DepositionRunner(population, ambient, dt=case["time_step"], dv=1.0,
                                      sum=sum_mode)
        runner.check()
        runner.run(2)
        with pytest.raises(RuntimeError, match="super-droplet"):
            runner.check()
        with pytest.raises(RuntimeError, match="super-droplet"):
            runner.snapshot()
    liquid_only = AmbientColumns(engine, Formulae(), rhod=case["rhod"], thd=case["thd"],
                                 qv=case["qv"])
    with pytest.raises(ValueError, match="mixed_phase"):
        dep.DepositionRunner(population, liquid_only, dt=1.0, dv=1.0, formulae=formulae)


def test_aliased_predicted_and_current_arrays_are_refused(engine, backend_class):
    case = dc.seeded_case(8, 100, 2)
    formulae = dc.formulae_for()
    cfg = dep.deposition_cfg(formulae, 0.01, 1.0)
    up = engine.upload
    arrays = {k: up(np.array(case[k])) for k in dc.AMBIENT}
    mass, mult, cell = (up(np.array(case[k])) for k in ("signed_water_mass", "multiplicity",
                                                        "cell_id"))
    spare_qv, spare_thd = up(np.array(case["qv"])), up(np.array(case["thd"]))
    for pqv, pthd in ((arrays["qv"], spare_thd), (spare_qv, arrays["thd"])):
        with pytest.raises(RuntimeError, match=r"error -"):
            engine.call_deposition(
                "sdm_deposition", cfg, 100, 2, mult, mass, cell,
                *(arrays[k] for k in dc.AMBIENT), pqv, pthd, None, dep.constants_of(formulae))
    dc.assert_same_bits(engine.download(mass), case["signed_water_mass"])

    backend = backend_class(formulae)
    S = backend.Storage
    store = {k: S.from_ndarray(np.array(case[k])) for k in dc.AMBIENT}
    common = dict(
        multiplicity=S.from_ndarray(np.array(case["multiplicity"])),
        signed_water_mass=S.from_ndarray(np.array(case["signed_water_mass"])),
        current_temperature=store["T"], current_total_pressure=store["p"],
        current_relative_humidity=store["RH"], current_water_activity=store["a_w_ice"],
        current_vapour_mixing_ratio=store["qv"], current_dry_air_density=store["rhod"],
        current_dry_potential_temperature=store["thd"], cell_volume=1.0, time_step=0.01,
        cell_id=S.from_ndarray(np.array(case["cell_id"])),
        reynolds_number=S.from_ndarray(np.zeros(100)), schmidt_number=S.from_ndarray(np.zeros(2)))
    spare = S.from_ndarray(np.array(case["thd"]))
    with pytest.raises(ValueError, match="predicted"):
        backend.deposition(**common, predicted_vapour_mixing_ratio=store["qv"],
                           predicted_dry_potential_temperature=spare)
    with pytest.raises(ValueError, match="predicted"):
        backend.deposition(**common, predicted_vapour_mixing_ratio=spare,
                           predicted_dry_potential_temperature=store["thd"])


def test_engine_without_a_deposition_library_says_so(oracle_engine):
    with pytest.raises(NotImplementedError, match="deposition"):
        oracle_engine.call_deposition("sdm_deposition")


def test_formulae_accepts_the_deposition_options_and_refuses_others_by_name(backend_class):
    for coordinate, capacity, kinetics in dc.COMBINATIONS:
        formulae = dc.formulae_for(coordinate, capacity, kinetics)
        assert formulae.diffusion_coordinate.__name__ == coordinate
        assert formulae.diffusion_ice_capacity.__name__ == capacity
        assert formulae.diffusion_ice_kinetics.__name__ == kinetics
        dep.check_formulae(formulae)
    defaults = Formulae()
    assert defaults.diffusion_coordinate.__name__ == "WaterMassLogarithm"
    assert defaults.diffusion_ice_capacity.__name__ == "Spherical"
    assert defaults.diffusion_ice_kinetics.__name__ == "Standard"
    assert defaults.latent_heat_sublimation.__name__ == "MurphyKoop2005"
    for option, value in (("diffusion_ice_capacity", "Plates"),
                          ("diffusion_ice_kinetics", "FuchsSutugin"),
                          ("latent_heat_sublimation", "Constant"),
                          ("diffusion_coordinate", "WaterMassSquareRoot")):
        with pytest.raises(NotImplementedError, match=option):
            Formulae(**{option: value})
    # condensation implements the logarithm only
    water_mass = Formulae(diffusion_coordinate="WaterMass")
    with pytest.raises(NotImplementedError, match="diffusion_coordinate"):
        condensation_check_formulae(water_mass)
    condensation_check_formulae(defaults)
    # deposition needs the mixed-phase shape, through every door
    with pytest.raises(NotImplementedError, match="particle_shape_and_density"):
        dep.check_formulae(defaults)
    case = dc.seeded_case(9, 10, 1)
    with pytest.raises(NotImplementedError, match="MixedPhaseSpheres"):
        dc.call_backend(backend_class, case, defaults)
    from types import SimpleNamespace  # pylint: disable=import-outside-toplevel

    odd = dc.formulae_for()
    odd.drop_growth = SimpleNamespace(__name__="Fick")
    with pytest.raises(NotImplementedError, match="drop_growth"):
        dep.check_formulae(odd)
    with pytest.raises(ValueError, match="sum"):
        dep.deposition_cfg(dc.formulae_for(), 1.0, 1.0, sum="pairwise")


def test_constants_override_reaches_the_library(engine):
    case = dc.seeded_case(10, 200, 2)
    plain = dc.call_engine(engine, case, dc.formulae_for())
    other = dc.call_engine(engine, case, dc.formulae_for(constants={"MAC_ice": 1.0}))
    assert (plain[0] != other[0]).any()


def test_pysdm_builder_runs_on_the_checker_class(backend_class):
    """an unmodified PySDM Builder + VapourDepositionOnIce on the checker-bound class: one step
    equals a direct method call on the same state"""
    run_pysdm_builder(backend_class)


def run_pysdm_builder(backend_class):
    """(shared with tests/test_hip_deposition.py)"""
    pytest.importorskip("PySDM")
    from PySDM import Builder  # pylint: disable=import-outside-toplevel,import-error
    from PySDM import Formulae as PySDMFormulae  # pylint: disable=import-outside-toplevel,import-error
    from PySDM.dynamics import VapourDepositionOnIce  # pylint: disable=import-outside-toplevel,import-error
    from PySDM.environments import Box  # pylint: disable=import-outside-toplevel,import-error

    from pysdm_amd.pysdm_plugin import as_pysdm_backend  # pylint: disable=import-outside-toplevel

    class BoxWithPredictions(Box):
        """Box's mesh and variables, plus separate predicted arrays behind `get_predicted`"""

        def __init__(self, dt, dv):
            super().__init__(dt, dv)
            self.predicted = {}

        def set_predicted(self, key, value):
            self.predicted[key] = self.particulator.backend.Storage.from_ndarray(
                np.array([value]))

        def get_predicted(self, key):
            return self.predicted[key]

    case = dc.seeded_case(11, 64, 1)
    case["multiplicity"] = np.maximum(case["multiplicity"], 1)
    formulae = PySDMFormulae(particle_shape_and_density="MixedPhaseSpheres")
    pysdm_class = as_pysdm_backend(backend_class)
    builder = Builder(n_sd=64, backend=pysdm_class(formulae),
                      environment=BoxWithPredictions(dt=case["time_step"],
                                                     dv=case["cell_volume"]))
    builder.add_dynamic(VapourDepositionOnIce())
    particulator = builder.build(
        attributes={"multiplicity": case["multiplicity"],
                    "signed water mass": case["signed_water_mass"].copy()}, products=())
    environment = particulator.environment
    names = {"T": "T", "p": "p", "RH": "RH", "a_w_ice": "a_w_ice", "rhod": "rhod", "thd": "thd",
             "qv": "water_vapour_mixing_ratio"}
    for key, name in names.items():
        environment[name] = float(case[key][0])
    environment["Schmidt number"] = 0.6
    environment.set_predicted("water_vapour_mixing_ratio", float(case["predicted_qv"][0]))
    environment.set_predicted("thd", float(case["predicted_thd"][0]))
    particulator.run(steps=1)
    want = dc.call_backend(backend_class, case, dc.formulae_for())
    dc.assert_same_bits(
        particulator.attributes["signed water mass"].to_ndarray(raw=True), want[0])
    dc.assert_same_bits(environment.get_predicted("water_vapour_mixing_ratio").to_ndarray(),
                        want[1])
    dc.assert_same_bits(environment.get_predicted("thd").to_ndarray(), want[2])
    assert (want[0] != case["signed_water_mass"]).any()

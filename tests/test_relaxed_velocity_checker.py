"""The relaxed-fall-velocity path on the CPU: the checker of include/sdm_relaxed_velocity.h
(tests/relaxed_velocity_checker) and the oracle engine behind the very host code the HIP engine
runs.

(i) the new header parses, the symbol binds, the cfg struct has the checker's size; an engine
without the library says so, (ii) the checker replays relax_box.npz within the bounds of
tests/relaxed_velocity_cases.py, (iii) `RelaxedVelocityRunner(route="stages")` on the oracle engine
gives the checker's bits, (iv) the chain route of the collisions and both routes of the
displacement, fed from the momentum, reproduce the four recorded runs on the oracle engine -
integers equal, (v) the refusals: a radius above the table top stores nothing, PowerSeries fused,
other formulae, the fused collision step with the momentum source, sharded runs, (vi) an unmodified
PySDM `Builder` on the checker class: PySDM's own dynamics and `fuse(RelaxedVelocity)` reproduce
relax_box_coal.npz, and `fuse(<collisions>)` beside `RelaxedVelocity` refuses (it used to run and
diverge), where the reference tree is present."""
import ctypes
import warnings

import numpy as np
import pytest

from pysdm_amd import abi
from pysdm_amd import recipe as R
from pysdm_amd.collisions import CollisionRunner
from pysdm_amd.population import MOMENTUM_ROW, Population
from pysdm_amd.relaxed_velocity import ROUTES, RelaxedVelocityRunner, init_fall_momenta
from pysdm_amd.terminal_velocity import TABLE_TOP
from tests import relaxed_velocity_cases as rc

LAWS = ("GunnKinzer1949", "RogersYau")


@pytest.fixture(scope="module", name="engine")
def checker_engine():
    from tests.relaxed_velocity_checker import RelaxedVelocityCheckerEngine  # pylint: disable=import-outside-toplevel

    return RelaxedVelocityCheckerEngine.get()


@pytest.fixture(scope="module", name="backend_class")
def checker_backend_class():
    from tests.relaxed_velocity_checker import RelaxedVelocityCheckerBackend  # pylint: disable=import-outside-toplevel

    return RelaxedVelocityCheckerBackend


# ---- (i) the boundary --------------------------------------------------------------------------------
def test_header_parses_symbol_binds_and_the_cfg_has_the_checkers_size(engine, oracle_engine):
    table = abi.parse_header(abi.RELAXED_VELOCITY_HEADER_PATH)
    assert sorted(table) == ["sdm_relaxed_velocity_step"]
    assert [p.name for p in table["sdm_relaxed_velocity_step"][1]] == [
        "ctx", "cfg", "signed_water_mass", "momentum", "velocity_out", "gk_a", "gk_b", "status"]
    assert sorted(engine.relaxed_velocity_library.signatures) == sorted(table)
    # the product library is bound from the same header (cross-compiled: loads without a GPU)
    assert sorted(abi.relaxed_velocity_library().signatures) == sorted(table)
    size = engine.relaxed_velocity_library.cdll.sdm_relaxed_velocity_cfg_size
    size.restype = ctypes.c_int64
    assert ctypes.sizeof(abi.RelaxedVelocityCfg) == size()
    # the new symbol is no part of sdm_hip.h, which the oracle implements in full
    assert "sdm_relaxed_velocity_step" not in abi.parse_header()
    with pytest.raises(NotImplementedError, match="no relaxed-velocity library"):
        oracle_engine.relaxed_velocity_call("sdm_relaxed_velocity_step")
    assert oracle_engine.fused_momentum_velocity is False


# ---- (ii) the golden ---------------------------------------------------------------------------------
@pytest.mark.parametrize("constant", [False, True])
@pytest.mark.parametrize("at_c", range(len(rc.C_VALUES)))
@pytest.mark.parametrize("start", [0, 1], ids=["from zero", "from half"])
def test_checker_replays_the_recorded_relaxation(engine, constant, at_c, start):
    data = rc.gold("relax_box")
    c = float(data["c"][at_c])
    assert c == rc.C_VALUES[at_c]
    terminal = rc.terminal_momentum(engine, data["mass"])
    momentum = data["starts"][start].copy()
    worst_relative = worst_normalised = 0.0
    for step in range(data["momentum"].shape[3]):
        momentum = rc.call_step(engine, data["mass"], momentum, dt=float(data["dt"]), c=c,
                                constant=constant)["momentum"]
        want = data["momentum"][int(constant), at_c, start, step]
        worst_relative = max(worst_relative, float((np.abs(momentum - want)
                                                    / np.abs(want)).max()))
        worst_normalised = max(worst_normalised, float((np.abs(momentum - want)
                                                        / terminal).max()))
    print(f"constant {constant}, c {c:g}, start {start}: relative {worst_relative:.3e}, "
          f"over the terminal momentum {worst_normalised:.3e}")
    assert worst_normalised <= rc.NORMALISED_BOUND
    if c != rc.ILL_CONDITIONED_C:  # (see tests/relaxed_velocity_cases.py on 1 - exp(-1e-15))
        assert worst_relative <= rc.RELATIVE_BOUND


def test_the_initial_momenta_are_the_references(oracle_engine):
    """relax_box's second start is half of the reference's init_fall_momenta; the library's radius
    (volume x 1 / (4/3 pi)) and the reference's host formula (volume / (4/3 pi)) may differ in the
    last place"""
    data = rc.gold("relax_box")
    ours = 0.5 * init_fall_momenta(oracle_engine, data["mass"])
    np.testing.assert_allclose(ours, data["starts"][1], rtol=4 * 2.0 ** -52, atol=0)
    np.testing.assert_array_equal(init_fall_momenta(oracle_engine, data["mass"], zero=True),
                                  np.zeros(64))


# ---- (iii) the stage route is the checker --------------------------------------------------------------
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("constant", [False, True])
def test_stage_route_on_the_oracle_gives_the_checkers_bits(engine, oracle_engine, law, constant):
    mass, momentum = rc.planted_state(1001, seed=3)
    for c in rc.C_VALUES:
        want = rc.call_step(engine, mass, momentum, dt=2.5, c=c, constant=constant, law=law,
                            n_calls=3)
        population = rc.momentum_population(oracle_engine, mass, momentum)
        runner = RelaxedVelocityRunner(population, c=c, constant=constant, dt=2.5,
                                       terminal_velocity=law, route="stages")
        version = population.state_version
        runner.run(3)
        assert population.state_version == version + 3 and population.host_dirty
        what = f"{law}, constant {constant}, c {c:g}"
        rc.assert_same_doubles(oracle_engine.download(population.momentum), want["momentum"],
                               f"{what}: momentum")
        rc.assert_same_doubles(oracle_engine.download(population.fall_velocity(None)),
                               want["velocity"], f"{what}: velocity")


@pytest.mark.parametrize("law", LAWS)
def test_fused_route_equals_stage_route_and_fills_the_velocity_cache(engine, law):
    mass, momentum = rc.planted_state(777, seed=5)
    results = []
    for route in ROUTES:
        population = rc.momentum_population(engine, mass, momentum)
        runner = RelaxedVelocityRunner(population, c=8, dt=1.0, terminal_velocity=law,
                                       route=route)
        runner.run(2)
        if route == "fused":  # the column is there already: no launch on asking for it
            calls = []
            engine.call = lambda *args: calls.append(args)  # (shadows the method)
            try:
                velocity = population.fall_velocity(None)
            finally:
                del engine.call
            assert not calls
        else:
            velocity = population.fall_velocity(None)
        results.append((engine.download(population.momentum), engine.download(velocity)))
    rc.assert_same_doubles(results[0][0], results[1][0], "momentum")
    rc.assert_same_doubles(results[0][1], results[1][1], "velocity")
    # the velocity follows the state: a change of the momentum is seen
    population.momentum[...] = 0.0
    population.touch_state()
    live = engine.download(population.fall_velocity(None))[mass != 0]
    np.testing.assert_array_equal(live, np.zeros_like(live))


def test_power_series_runs_in_stages_and_is_refused_fused_by_name(oracle_engine):
    mass, momentum = rc.planted_state(65, seed=7)
    population = rc.momentum_population(oracle_engine, mass, momentum)
    with pytest.raises(NotImplementedError, match="PowerSeries"):
        RelaxedVelocityRunner(population, dt=1.0, terminal_velocity="PowerSeries")
    runner = RelaxedVelocityRunner(population, c=1e-12, dt=1.0, terminal_velocity="PowerSeries",
                                   route="stages")
    runner.step()  # tau -> 0: the momentum is the terminal momentum of the law
    want = init_fall_momenta(oracle_engine, mass, "PowerSeries")
    got = oracle_engine.download(population.momentum)
    np.testing.assert_allclose(got[mass != 0], want[mass != 0], rtol=4 * 2.0 ** -52)
    with pytest.raises(NotImplementedError, match="MixedPhaseSpheres"):
        RelaxedVelocityRunner(population, dt=1.0, formulae="MixedPhaseSpheres")
    with pytest.raises(ValueError, match="route"):
        RelaxedVelocityRunner(population, dt=1.0, route="eager")
    plain = Population(oracle_engine, multiplicity=np.ones(4, dtype=np.int64),
                       mass=np.full(4, 1e-9))
    with pytest.raises(ValueError, match="relative fall momentum"):
        RelaxedVelocityRunner(plain, dt=1.0)
    with pytest.raises(ValueError, match="relative fall momentum"):
        Population(oracle_engine, multiplicity=np.ones(4, dtype=np.int64), mass=np.full(4, 1e-9),
                   velocity_source="momentum")
    with pytest.raises(ValueError, match="velocity_source"):
        Population(oracle_engine, multiplicity=np.ones(4, dtype=np.int64), mass=np.full(4, 1e-9),
                   velocity_source="relaxed")


# ---- (v) a radius above the table top ------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_a_radius_above_the_table_top_is_refused_with_nothing_stored(engine, route):
    at_top, above = rc.mass_at_table_top(engine)
    mass, momentum = rc.planted_state(300, seed=9)
    mass[123] = at_top
    population = rc.momentum_population(engine, mass, momentum)
    runner = RelaxedVelocityRunner(population, dt=1.0, route=route)
    runner.step()  # the top itself is served
    assert np.isfinite(engine.download(population.momentum)[123])
    mass[123], mass[7] = above, -above
    population = rc.momentum_population(engine, mass, momentum)
    runner = RelaxedVelocityRunner(population, dt=1.0, route=route)
    version = population.state_version
    with pytest.raises(ValueError, match=f"Radii can be interpolated up to {TABLE_TOP} m"):
        runner.step()
    np.testing.assert_array_equal(rc.bits(engine.download(population.momentum)),
                                  rc.bits(momentum))
    assert population.state_version == version
    out = rc.call_step(engine, mass, momentum)
    np.testing.assert_array_equal(out["status"], [2, 0])
    np.testing.assert_array_equal(rc.bits(out["momentum"]), rc.bits(momentum))
    np.testing.assert_array_equal(out["velocity"], np.full(300, -7.0))
    # Rogers-Yau has no top
    out = rc.call_step(engine, mass, momentum, law="RogersYau")
    np.testing.assert_array_equal(out["status"], [0, 0])
    assert (out["momentum"] != momentum).any()


# ---- (iv) the recorded runs on the oracle engine ---------------------------------------------------------
@pytest.mark.parametrize("name", ["relax_box_coal", "relax_box_breakup", "relax_4x4"])
def test_chain_route_fed_from_the_momentum_reproduces_the_recorded_run(oracle_engine, name):
    data = rc.gold(name)
    lengths = []
    for step, snap in rc.run_collisions(oracle_engine, name, collision_route="chain",
                                        relax_route="stages"):
        rc.assert_collision_step(snap, data, step, name)
        lengths.append(int(snap["length"]))
    assert step == int(data["steps"])
    if int(data["breakup"]):
        assert snap["breakup_rate"].sum() > 0
    else:
        assert lengths[-1] < lengths[0] <= len(data["init/mass"])  # deaths


@pytest.mark.parametrize("route", ["fused", "chain"])
def test_displacement_sediments_with_the_relaxed_velocity(oracle_engine, route):
    rc.run_displacement(oracle_engine, route=route, relax_route="stages")


def test_the_terminal_velocity_does_not_reproduce_the_recorded_run(oracle_engine):
    """the check of the checks: with the fall velocity taken from the radius - what the fused step
    did beside RelaxedVelocity before it refused - the recorded run is NOT reproduced"""
    data = rc.gold("relax_box_coal")
    population = Population(oracle_engine, multiplicity=data["init/multiplicity"],
                            mass=data["init/mass"],
                            more_extensive={MOMENTUM_ROW: data["init/momentum"]})
    collisions = CollisionRunner(population, rc.collision_setup(data), dt=float(data["dt"]),
                                 dv=float(data["dv"]), route="chain")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        collisions.run(int(data["steps"]))
    population.compact()
    want = data[f"step{int(data['steps'])}/multiplicity"]
    assert (oracle_engine.download(population.multiplicity) != want).any()


# ---- (v) refusals of the collision runner ----------------------------------------------------------------
def test_collision_runner_refuses_what_it_cannot_do(oracle_engine):
    data = rc.gold("relax_box_coal")
    population = rc.population_from(oracle_engine, data)
    setup = rc.collision_setup(data)
    with pytest.raises(NotImplementedError, match="relative fall momentum"):
        CollisionRunner(population, setup, dt=1.0, dv=1.0, route="fused", velocity="momentum")
    with pytest.raises(ValueError, match="velocity source"):
        CollisionRunner(population, setup, dt=1.0, dv=1.0, route="chain")  # "terminal"
    with pytest.raises(ValueError, match="velocity="):
        CollisionRunner(population, setup, dt=1.0, dv=1.0, velocity="relaxed")
    runner = CollisionRunner(population, setup, dt=1.0, dv=1.0, route="chain",
                             velocity="momentum")
    runner.route = "fused"  # (sharding drives the fused route: the refusal by name comes first)
    from pysdm_amd import sharding  # pylint: disable=import-outside-toplevel

    with pytest.raises(NotImplementedError, match="[Ss]harded"):
        sharding._sharded(runner)  # pylint: disable=protected-access
    plain = Population(oracle_engine, multiplicity=data["init/multiplicity"],
                       mass=data["init/mass"])
    with pytest.raises(ValueError, match="velocity source"):
        CollisionRunner(plain, R.CollisionSetup.coalescence(R.Geometric(), seed=1), dt=1.0,
                        dv=1.0, route="chain", velocity="momentum")


# ---- (vi) the unmodified PySDM front-end -----------------------------------------------------------------
@pytest.fixture(scope="module", name="ref")
def reference_modules():
    return rc.import_reference()


@pytest.mark.parametrize("fuse_relaxation", [False, True], ids=["methods", "fuse"])
def test_pysdm_box_on_the_checker_class_reproduces_the_recorded_run(ref, backend_class,
                                                                    fuse_relaxation):
    data = rc.gold("relax_box_coal")
    for step, snap in rc.run_pysdm_box(ref, backend_class, data, fuse_relaxation=fuse_relaxation,
                                    fuse_collisions=False):
        rc.assert_collision_step(snap, data, step, "PySDM front-end")
    assert step == int(data["steps"])


def test_fused_collisions_beside_relaxed_velocity_refuse(ref, oracle_backend_class):
    """before: ran, with the fall velocity of the radius, and left the reference without any error"""
    data = rc.gold("relax_box_coal")
    with pytest.raises(NotImplementedError, match="RelaxedVelocity"):
        for _ in rc.run_pysdm_box(ref, oracle_backend_class, data, fuse_relaxation=False,
                               fuse_collisions=True):
            pass


def test_fused_relaxation_forwards_to_the_wrapped_dynamic_and_refuses_by_name(ref,
                                                                              backend_class):
    from pysdm_amd.pysdm_plugin import (FusedRelaxedVelocity, as_pysdm_backend,  # pylint: disable=import-outside-toplevel
                                        fuse)

    inner = ref["RelaxedVelocity"](c=3.0, constant=True)
    fused = fuse(inner)
    assert isinstance(fused, FusedRelaxedVelocity)
    assert [cls.__name__ for cls in type(fused).__mro__][-2] == "RelaxedVelocity"
    assert fused.c == 3.0 and fused.constant is True
    assert fused.calculate_tau.__self__ is inner and fused.calculate_scale_factor.__self__ is inner
    fused.c = 5.0
    assert inner.c == 5.0
    for option, value in (("terminal_velocity", "PowerSeries"),
                          ("particle_shape_and_density", "MixedPhaseSpheres")):
        formulae = ref["PySDM"].Formulae(**{option: value})
        builder = ref["PySDM"].Builder(n_sd=4, backend=as_pysdm_backend(backend_class)(formulae),
                                       environment=ref["Box"](dt=1.0, dv=1.0))
        builder.add_dynamic(fuse(ref["RelaxedVelocity"]()))
        with pytest.raises(NotImplementedError, match=value):  # (dynamics register at build)
            builder.build(attributes={"multiplicity": np.ones(4), "water mass": np.full(4, 1e-9),
                                      "relative fall momentum": np.zeros(4)}, products=())

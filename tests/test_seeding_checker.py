"""The seeding path on the CPU: the checker of include/sdm_seeding.h (tests/seeding_checker)
behind the very host code the HIP backend runs.

(i) the new header parses and both symbols bind; an engine without a seeding library says so,
(ii) the checker-bound backend class replays every recorded call of seed_methods.npz to the bit,
the -1 entries of idx included, (iii) `SeedingRunner` reproduces the two recorded Box runs on its
fused and on its stage route - in the box with coalescence interleaved with a `CollisionRunner` on
the same population, on both of its routes -, (iv) the fused step equals the stage sequence and a
shortfall stores nothing, (v) an unmodified PySDM `Builder` + `Box` + `Seeding` on the checker
class reproduces seed_box.npz method by method and through `fuse()` and raises the reference's
three refusals (where the reference tree is present), (vi) the host logic: rate 0, a reservoir of
one seed, row names.  Equality everywhere: integers with ==, doubles as uint64."""
import os
import sys

import numpy as np
import pytest

from pysdm_amd import abi
from pysdm_amd import seeding as sd
from pysdm_amd.population import MASS_ROW, Population
from tests import seeding_cases as sc

METHODS = sc.gold("seed_methods")
BOXES = ("seed_box", "seed_box_coal")
HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"


@pytest.fixture(scope="module", name="backend_class")
def checker_backend_class():
    from tests.seeding_checker import SeedingCheckerBackend  # pylint: disable=import-outside-toplevel

    return SeedingCheckerBackend


@pytest.fixture(scope="module", name="engine")
def checker_engine():
    from tests.seeding_checker import SeedingCheckerEngine  # pylint: disable=import-outside-toplevel

    return SeedingCheckerEngine.get()


def test_header_parses_and_every_symbol_binds(engine, oracle_engine):
    table = abi.parse_header(abi.SEEDING_HEADER_PATH)
    assert sorted(table) == ["sdm_seeding", "sdm_seeding_step"]
    assert [p.name for p in table["sdm_seeding"][1]][-2:] == ["number_to_inject", "status"]
    assert table["sdm_seeding_step"][1][-3].kind == "host_array"  # rng_state_inc[4]
    assert sorted(engine.seeding_library.signatures) == sorted(table)
    # the product library is bound from the same header (cross-compiled: loads without a GPU)
    assert sorted(abi.seeding_library().signatures) == sorted(table)
    with pytest.raises(NotImplementedError, match="no seeding library"):
        oracle_engine.seeding_call("sdm_seeding")


@pytest.mark.parametrize("number", range(int(METHODS["n_calls"])))
def test_checker_replays_recorded_method_calls(backend_class, number):
    got, expected = sc.replay_method_call(backend_class, METHODS, number)
    assert (expected["idx"] == -1).sum() == int(METHODS["k"][number])
    for key, value in expected.items():
        sc.assert_same_bits(got[key], value, f"{METHODS['kind'][number]}: {key}")


@pytest.mark.parametrize("route", sd.ROUTES)
@pytest.mark.parametrize("name", BOXES)
def test_runner_reproduces_recorded_box_run(engine, name, route):
    data = sc.gold(name)
    for step, got in enumerate(sc.run_box(engine, data, route)):
        sc.assert_box_step(got, data, step, f"{name} ({route})")
    assert step == len(data["rates"]) - 1
    assert len({tuple(index) for index in data["seed_index"]}) > 3  # the index is reshuffled


def test_box_with_coalescence_on_the_chain_route_of_the_collisions(engine):
    data = sc.gold("seed_box_coal")
    lengths = data["length"]
    assert (np.diff(lengths) < 0).any() and (np.diff(lengths) > 0).any()  # deaths and refills
    for step, got in enumerate(sc.run_box(engine, data, "fused", collision_route="chain")):
        sc.assert_box_step(got, data, step, "seed_box_coal (chain)")


@pytest.mark.parametrize("n_sd, n_seeds, k, n_attr, index", [
    (1, 1, 1, 1, "identity"), (65, 2, 1, 5, "reversed"), (1000, 10, 5, 1, "equal"),
    (4097, 1000, 1000, 5, "reversed"), (1025, 10, 10, 1, "identity")])
@pytest.mark.parametrize("offset", [0, 2 ** 33 + 5])
def test_fused_step_equals_stage_sequence(engine, n_sd, n_seeds, k, n_attr, index, offset):
    state = sc.seeded_state(n_sd, n_seeds=n_seeds, k=k, n_attr=n_attr, index=index)
    free = int((state["multiplicity"] == 0).sum())
    calls = 3 if free >= 3 * k else 1
    got = sc.call_step(engine, state, shuffle=True, offset=offset, n_calls=calls)
    want = sc.stage_sequence(engine, state, shuffle=True, offset=offset, n_calls=calls)
    assert got["error"] is None and len(got["lengths"]) == calls
    sc.assert_same_step(got, want, "fused against stages")
    assert got["lengths"][-1] == n_sd - free + calls * k  # (no seed has multiplicity 0)


def test_stage_marks_the_filled_slots_and_reports_the_counts(engine):
    state = sc.state_with_free([10, 0, 3, 4, 9], k=3, n_seeds=5, n_attr=2, index="reversed")
    out = sc.call_stage(engine, state)
    np.testing.assert_array_equal(out["status"][:3], [4, 3, 0])
    np.testing.assert_array_equal(np.flatnonzero(out["idx"] == -1), [0, 3, 4])
    np.testing.assert_array_equal(out["multiplicity"][[0, 3, 4]],
                                  state["seed_multiplicity"][[4, 3, 2]])
    sc.assert_same_bits(out["attributes"][:, [0, 3, 4]], state["seed_attributes"][:, [4, 3, 2]],
                        "rows")
    assert out["multiplicity"][9] == 0  # the fourth free slot stays free


def test_shortfall_stores_nothing_and_is_reported(engine):
    state = sc.state_with_free([10, 2, 7], k=3, n_seeds=4, n_attr=2)
    state["idx"] = np.arange(10, dtype=np.int64)[::-1].copy()
    out = sc.call_stage(engine, state)
    np.testing.assert_array_equal(out["status"][:3], [2, 0, 0])
    fused = sc.call_step(engine, state, shuffle=False)
    assert fused["error"] is not None and "2 free slots" in fused["error"]
    for result in (out, fused):
        for key in ("idx", "multiplicity", "attributes"):
            sc.assert_same_bits(result[key], state[key], f"shortfall: {key}")
    state["seed_index"][1] = 4  # a seed index outside the reservoir, with room enough
    state["multiplicity"][5] = 0
    out = sc.call_stage(engine, state)
    np.testing.assert_array_equal(out["status"][:3], [3, 0, 1])
    sc.assert_same_bits(out["multiplicity"], state["multiplicity"], "bad seed index")


def test_nothing_to_inject_is_no_call_at_all(engine):
    state = sc.state_with_free([4, 1], k=0, n_seeds=2)
    out = sc.call_stage(engine, state)
    np.testing.assert_array_equal(out["status"], [-7] * 4)  # not even the status is written
    fused = sc.call_step(engine, state, shuffle=True)
    assert fused["lengths"] == [-1] and fused["error"] is None
    sc.assert_same_bits(fused["seed_index"], state["seed_index"], "no shuffle either")


# ---- host logic --------------------------------------------------------------------------------------
def _population(engine, n_sd=8, live=5):
    multiplicity = np.where(np.arange(n_sd) < live, 3.0, np.nan)
    return Population(engine, multiplicity=multiplicity, mass=np.full(n_sd, 1e-12))


def test_rate_zero_draws_nothing_and_launches_nothing(engine):
    population = _population(engine)
    runner = sd.SeedingRunner(population, multiplicity=[1, 2, 3],
                              extensive={MASS_ROW: [1e-15, 2e-15, 3e-15]},
                              injection_rate=lambda time: 0, dt=1.0, seed=44)
    calls = []
    engine.seeding_call = lambda *args: calls.append(args)  # (shadows the method)
    try:
        version = population.state_version
        runner.run(3)
    finally:
        del engine.seeding_call
    assert runner.rng_offset == 0 and not calls and runner.n_steps == 3
    assert population.state_version == version and population.live == 5
    np.testing.assert_array_equal(runner.seed_index(), [0, 1, 2])
    runner.injection_rate = lambda time: 2
    runner.step()
    assert runner.rng_offset == 3 and population.live == 7 and runner.n_injections == 1


def test_a_reservoir_of_one_seed_creates_no_stream(engine):
    population = _population(engine)
    runner = sd.SeedingRunner(population, multiplicity=[9], extensive={MASS_ROW: [5e-15]},
                              injection_rate=lambda time: 1, dt=1.0, seed=44)
    assert runner.state_inc is None and runner.u01 is None
    runner.run(2)
    assert runner.rng_offset == 0 and population.live == 7
    np.testing.assert_array_equal(engine.download(population.multiplicity)[5:], [9, 9, 0])
    np.testing.assert_array_equal(engine.download(population.perm)[:7], np.arange(7))


def test_row_names_must_match_and_the_three_refusals(engine):
    population = _population(engine)
    with pytest.raises(ValueError, match="do not match"):
        sd.SeedingRunner(population, multiplicity=[1], extensive={"water mass": [1e-15]},
                         injection_rate=lambda time: 1, dt=1.0, seed=1)
    with pytest.raises(ValueError, match="route"):
        sd.SeedingRunner(population, multiplicity=[1], extensive={MASS_ROW: [1e-15]},
                         injection_rate=lambda time: 1, dt=1.0, seed=1, route="eager")

    def runner_for(pop, n_seeds, number):
        return sd.SeedingRunner(pop, multiplicity=[1] * n_seeds,
                                extensive={MASS_ROW: [1e-15] * n_seeds},
                                injection_rate=lambda time: number, dt=1.0, seed=1)

    with pytest.raises(ValueError, match="No available seeds to inject"):
        runner_for(_population(engine, live=8), 2, 1).step()
    with pytest.raises(ValueError, match="inject more super particles than space available"):
        runner_for(_population(engine, live=7), 4, 2).step()
    with pytest.raises(ValueError,
                       match="inject multiple super particles with the same attributes"):
        runner_for(population, 2, 3).step()
    assert population.live == 5


@pytest.mark.parametrize("route", sd.ROUTES)
def test_a_refusal_on_the_device_spends_the_numbers_of_its_shuffle(engine, route):
    """bookkeeping that claims more room than there is passes the host's check and is refused by
    the library after the seed index was shuffled: the stream position moves with the index on both
    routes, and nothing was stored"""
    population = _population(engine, live=7)
    population.live = population.working = 5  # (wrong on purpose)
    runner = sd.SeedingRunner(population, multiplicity=[1, 2, 3],
                              extensive={MASS_ROW: [1e-15, 2e-15, 3e-15]},
                              injection_rate=lambda time: 2, dt=1.0, seed=44, route=route)
    before = engine.download(population.multiplicity)
    with pytest.raises((RuntimeError, ValueError), match="1 free slots"):
        runner.step()
    assert runner.rng_offset == 3
    np.testing.assert_array_equal(engine.download(population.multiplicity), before)
    other = sd.SeedingRunner(_population(engine, live=5), multiplicity=[1, 2, 3],
                             extensive={MASS_ROW: [1e-15, 2e-15, 3e-15]},
                             injection_rate=lambda time: 2, dt=1.0, seed=44, route=route)
    other.step()  # the same first shuffle, this time with room
    np.testing.assert_array_equal(runner.seed_index(), other.seed_index())
    assert other.rng_offset == 3


# ---- the unmodified PySDM front-end ------------------------------------------------------------------
def import_reference():
    """PySDM in its pure-Python mode with the import-only stand-ins of tests/golden; skips the
    calling test where the reference tree is absent - where it is present, a failing import (a
    broken stand-in, say) is a failure"""
    if not os.path.isdir(os.path.join(REFERENCE, "PySDM")):
        pytest.skip("reference tree not present")
    os.environ.setdefault("CI", "1")
    sys.dont_write_bytecode = True
    added = [os.path.join(HERE, "golden", "standins"), REFERENCE]
    sys.path[:0] = added
    try:
        import PySDM  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.dynamics import Seeding  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.environments import Box  # pylint: disable=import-outside-toplevel,import-error
    finally:
        for path in added:
            sys.path.remove(path)
    return {"PySDM": PySDM, "Seeding": Seeding, "Box": Box}


@pytest.fixture(scope="module", name="ref")
def reference_modules():
    return import_reference()


def run_pysdm_box(ref, backend_class, data, fused):
    """the recorded run through PySDM's own front-end (shared with tests/test_hip_seeding.py);
    yields per step what the golden holds"""
    from pysdm_amd.pysdm_plugin import as_pysdm_backend, fuse  # pylint: disable=import-outside-toplevel

    dt, rates = float(data["dt"]), data["rates"]
    formulae = ref["PySDM"].Formulae(seed=int(data["seed"]))
    n_sd = data["init/multiplicity"].shape[0]
    builder = ref["PySDM"].Builder(n_sd=n_sd, backend=as_pysdm_backend(backend_class)(formulae),
                                   environment=ref["Box"](dt=dt, dv=float(data["dv"])))
    dynamic = ref["Seeding"](
        super_droplet_injection_rate=lambda time: int(rates[int(round(time / dt))]),
        seeded_particle_extensive_attributes={str(data["row"]): data["seed/mass"].copy()},
        seeded_particle_multiplicity=data["seed/multiplicity"].copy())
    builder.add_dynamic(fuse(dynamic) if fused else dynamic)
    particulator = builder.build(attributes={"multiplicity": data["init/multiplicity"].copy(),
                                             "water mass": data["init/mass"].copy()},
                                 products=())
    attrs = particulator.attributes
    for _ in range(len(rates)):
        particulator.run(steps=1)
        idx = attrs._ParticleAttributes__idx  # pylint: disable=protected-access
        yield {"idx": idx.to_ndarray()[:len(idx)], "length": len(idx),
               "multiplicity": attrs["multiplicity"].to_ndarray(raw=True),
               "attributes": attrs.get_extensive_attribute_storage().to_ndarray(raw=True),
               "seed_index": particulator.dynamics["Seeding"].index.to_ndarray()}
        assert attrs.super_droplet_count == len(idx)  # healthy, as after PySDM's own sanitize


@pytest.mark.parametrize("fused", [False, True], ids=["methods", "fuse"])
def test_pysdm_box_runs_on_the_checker_class(ref, backend_class, fused):
    data = sc.gold("seed_box")
    for step, got in enumerate(run_pysdm_box(ref, backend_class, data, fused)):
        sc.assert_box_step(got, data, step, "PySDM front-end")


@pytest.mark.parametrize("fused", [False, True], ids=["methods", "fuse"])
def test_pysdm_particulator_raises_its_three_refusals(ref, backend_class, fused):
    from pysdm_amd.pysdm_plugin import as_pysdm_backend, fuse  # pylint: disable=import-outside-toplevel

    def particulator_for(live, n_seeds, number, n_sd=4):
        builder = ref["PySDM"].Builder(
            n_sd=n_sd, backend=as_pysdm_backend(backend_class)(ref["PySDM"].Formulae()),
            environment=ref["Box"](dt=1.0, dv=1.0))
        dynamic = ref["Seeding"](super_droplet_injection_rate=lambda time: number,
                                 seeded_particle_extensive_attributes={
                                     str(sc.gold("seed_box")["row"]): [1e-15] * n_seeds},
                                 seeded_particle_multiplicity=[1] * n_seeds)
        builder.add_dynamic(fuse(dynamic) if fused else dynamic)
        return builder.build(attributes={
            "multiplicity": np.where(np.arange(n_sd) < live, 2.0, np.nan),
            "water mass": np.full(n_sd, 1e-12)}, products=())

    with pytest.raises(ValueError, match="No available seeds to inject"):
        particulator_for(4, 2, 1).run(steps=1)
    with pytest.raises(ValueError, match="inject more super particles than space available"):
        particulator_for(3, 3, 2).run(steps=1)
    # (Seeding.__call__ asserts the third condition itself before Particulator.seeding is reached,
    # seeding.py:78-80: the refusal is raised through a direct call)
    particulator = particulator_for(1, 2, 1, n_sd=6)
    particulator.run(steps=1)
    dynamic = particulator.dynamics["Seeding"]
    with pytest.raises(ValueError,
                       match="inject multiple super particles with the same attributes"):
        particulator.seeding(
            seeded_particle_index=dynamic.index,
            seeded_particle_multiplicity=dynamic.seeded_particle_multiplicity,
            seeded_particle_extensive_attributes=dynamic.seeded_particle_extensive_attributes,
            number_of_super_particles_to_inject=3)
    assert particulator.attributes.super_droplet_count == 2

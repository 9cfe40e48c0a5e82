"""Shared by the seeding tests (tests/test_seeding_checker.py on the CPU checker,
tests/test_hip_seeding.py on the device): the recorded goldens (tests/golden/seed_*.npz, written
by tests/golden/gen_seeding_golden.py from the reference), seeded and planted states, and the
calls of both symbols of include/sdm_seeding.h on any engine.  Every comparison is for equality:
integers with ==, doubles as uint64 views (they are copies)."""
import ctypes
import functools
import os
import warnings

import numpy as np

from pysdm_amd import recipe as R
from pysdm_amd.abi import pcg64_state_inc
from pysdm_amd.collisions import CollisionRunner
from pysdm_amd.population import MASS_ROW, Population
from pysdm_amd.seeding import SeedingRunner

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the tile of k_seed_scatter / k_seed_count and the tile counts one round of k_seed_scan takes
# (pysdm_amd/csrc/seeding.hip: SEED_TILE, SEED_ROUND)
TILE, ROUND = 1024, 1024


@functools.lru_cache(maxsize=None)
def gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def bits(values):
    values = np.ascontiguousarray(values)
    return values.view(np.uint64) if values.dtype == np.float64 else values


def assert_same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


# ---- recorded backend-method calls ---------------------------------------------------------------
def method_call(data, number):
    n_attr, n_seeds = int(data["n_attr"][number]), int(data["n_seeds"][number])
    return {"idx": data["in_idx"][number].copy(),
            "multiplicity": data["in_multiplicity"][number].copy(),
            "attributes": np.ascontiguousarray(data["in_attributes"][number][:n_attr]),
            "seed_index": data["seed_index"][number][:n_seeds].copy(),
            "seed_multiplicity": data["seed_multiplicity"][number][:n_seeds].copy(),
            "seed_attributes": np.ascontiguousarray(
                data["seed_attributes"][number][:n_attr, :n_seeds]),
            "k": int(data["k"][number])}, {
                "idx": data["out_idx"][number], "multiplicity": data["out_multiplicity"][number],
                "attributes": np.ascontiguousarray(data["out_attributes"][number][:n_attr])}


def replay_method_call(backend_class, data, number):
    """the recorded call through the PySDM-shaped backend method"""
    state, expected = method_call(data, number)
    backend = backend_class()
    S = backend.Storage
    args = {"idx": S.from_ndarray(state["idx"]),
            "multiplicity": S.from_ndarray(state["multiplicity"]),
            "extensive_attributes": S.from_ndarray(state["attributes"]),
            "seeded_particle_index": S.from_ndarray(state["seed_index"]),
            "seeded_particle_multiplicity": S.from_ndarray(state["seed_multiplicity"]),
            "seeded_particle_extensive_attributes": S.from_ndarray(state["seed_attributes"])}
    backend.seeding(**args, number_of_super_particles_to_inject=state["k"])
    got = {"idx": args["idx"].to_ndarray(), "multiplicity": args["multiplicity"].to_ndarray(),
           "attributes": args["extensive_attributes"].to_ndarray()}
    return got, expected


# ---- both symbols on host arrays -------------------------------------------------------------------
def call_stage(engine, state):
    """sdm_seeding on copies of `state`; returns (idx, multiplicity, attributes, status)"""
    up, down = engine.upload, engine.download
    idx, mult, attrs = (up(state[k].copy()) for k in ("idx", "multiplicity", "attributes"))
    status = engine.full(4, np.int64, -7)
    engine.seeding_call(
        "sdm_seeding", idx, mult, attrs, int(state["attributes"].shape[0]),
        int(state["multiplicity"].shape[0]), up(state["seed_index"].copy()),
        up(state["seed_multiplicity"].copy()), up(state["seed_attributes"].copy()),
        int(state["seed_multiplicity"].shape[0]), int(state["k"]), status)
    return {"idx": down(idx), "multiplicity": down(mult), "attributes": down(attrs),
            "status": down(status)}


def call_step(engine, state, *, shuffle, seed=44, offset=0, n_calls=1):
    """sdm_seeding_step, `n_calls` times in a row with the seed index kept; returns the state
    after the last call, the lengths, and what was raised instead (a refusal leaves the rest
    out)"""
    up, down = engine.upload, engine.download
    idx, mult, attrs = (up(state[k].copy()) for k in ("idx", "multiplicity", "attributes"))
    index = up(state["seed_index"].copy())
    seed_mult, seed_attrs = up(state["seed_multiplicity"].copy()), up(
        state["seed_attributes"].copy())
    n_seeds = int(state["seed_multiplicity"].shape[0])
    lengths, error = [], None
    for call in range(n_calls):
        new_length = ctypes.c_int64(-1)
        try:
            engine.seeding_call(
                "sdm_seeding_step", idx, mult, attrs, int(state["attributes"].shape[0]),
                int(state["multiplicity"].shape[0]), index, seed_mult, seed_attrs, n_seeds,
                int(state["k"]), int(shuffle), pcg64_state_inc(seed), offset + call * n_seeds,
                new_length)
        except RuntimeError as refused:
            error = str(refused)
            break
        lengths.append(int(new_length.value))
    return {"idx": down(idx), "multiplicity": down(mult), "attributes": down(attrs),
            "seed_index": down(index), "lengths": lengths, "error": error}


def stage_sequence(engine, state, *, shuffle, seed=44, offset=0, n_calls=1):
    """what sdm_seeding_step stands for, symbol by symbol"""
    up, down = engine.upload, engine.download
    idx, mult, attrs = (up(state[k].copy()) for k in ("idx", "multiplicity", "attributes"))
    index = up(state["seed_index"].copy())
    seed_mult, seed_attrs = up(state["seed_multiplicity"].copy()), up(
        state["seed_attributes"].copy())
    n_seeds, n_sd = int(state["seed_multiplicity"].shape[0]), int(state["multiplicity"].shape[0])
    u01 = engine.empty(max(n_seeds, 1), np.float64)
    status = engine.zeros(4, np.int64)
    lengths, error = [], None
    for call in range(n_calls):
        if shuffle and n_seeds > 1:
            engine.call("sdm_pcg64_uniform", u01, n_seeds, pcg64_state_inc(seed),
                        offset + call * n_seeds)
            engine.call("sdm_shuffle_global", index, n_seeds, u01)
        engine.seeding_call("sdm_seeding", idx, mult, attrs, int(state["attributes"].shape[0]),
                            n_sd, index, seed_mult, seed_attrs, n_seeds, int(state["k"]), status)
        if int(down(status)[1]) != int(state["k"]):
            error = "refused"
            break
        engine.call("sdm_identity_index", idx, n_sd)
        lengths.append(engine.scalar_out("sdm_remove_zero_n_or_flagged", ctypes.c_int64, mult,
                                         idx, n_sd, n_sd))
    return {"idx": down(idx), "multiplicity": down(mult), "attributes": down(attrs),
            "seed_index": down(index), "lengths": lengths, "error": error}


def assert_same_step(got, want, what):
    """two results of call_step / stage_sequence: everything, idx up to the live length"""
    assert got["lengths"] == want["lengths"], what
    assert (got["error"] is None) == (want["error"] is None), what
    for key in ("multiplicity", "attributes", "seed_index"):
        assert_same_bits(got[key], want[key], f"{what}: {key}")
    if got["lengths"]:
        length = got["lengths"][-1]
        assert_same_bits(got["idx"][:length], want["idx"][:length], f"{what}: idx")


# ---- states ------------------------------------------------------------------------------------------
def seeds(rng, n_seeds, n_attr, index="identity"):
    order = {"identity": np.arange(n_seeds), "reversed": np.arange(n_seeds)[::-1],
             "equal": np.full(n_seeds, n_seeds - 1)}[index]
    return {"seed_index": np.ascontiguousarray(order, dtype=np.int64),
            "seed_multiplicity": rng.integers(1, 10 ** 6, n_seeds).astype(np.int64),
            "seed_attributes": rng.uniform(10.0, 20.0, (n_attr, n_seeds))}


def state_with_free(free, *, k, n_seeds=None, n_attr=1, index="identity", seed=1, idx=None):
    """a state whose free slots are exactly `free` (a boolean mask or a list of slots)"""
    rng = np.random.default_rng(seed)
    free = np.asarray(free)
    if free.dtype != bool:
        mask = np.zeros(int(free[0]), dtype=bool)  # (n_sd first, then the slots)
        mask[free[1:]] = True
        free = mask
    n_sd = free.shape[0]
    multiplicity = np.where(free, 0, rng.integers(1, 1000, n_sd)).astype(np.int64)
    state = {"idx": np.arange(n_sd, dtype=np.int64) if idx is None else idx,
             "multiplicity": multiplicity, "attributes": rng.uniform(1.0, 2.0, (n_attr, n_sd)),
             "k": int(k)}
    state.update(seeds(rng, int(n_seeds if n_seeds is not None else max(k, 1)), n_attr, index))
    return state


def seeded_state(n_sd, *, n_seeds, k, n_attr=1, index="identity", seed=1, free_fraction=0.3):
    rng = np.random.default_rng(seed + 1000)
    free = rng.uniform(size=n_sd) < free_fraction
    want = min(n_sd, k)
    if free.sum() < want:  # room for what is asked for
        free[rng.permutation(n_sd)[:want]] = True
    return state_with_free(free, k=k, n_seeds=n_seeds, n_attr=n_attr, index=index, seed=seed,
                           idx=rng.permutation(n_sd).astype(np.int64))


# ---- recorded box runs ---------------------------------------------------------------------------
def run_box(engine, data, route, collision_route="fused"):
    """the recorded Box run on `SeedingRunner` (and `CollisionRunner` first in every step, for the
    box with coalescence); yields per step what the golden holds"""
    dt, seed = float(data["dt"]), int(data["seed"])
    rates = data["rates"]
    population = Population(engine, multiplicity=data["init/multiplicity"],
                            mass=data["init/mass"])
    collisions = None
    if int(data["coalescence"]):
        setup = R.CollisionSetup.coalescence(R.Golovin(b=float(data["golovin_b"])), seed=seed,
                                             adaptive=False)
        collisions = CollisionRunner(population, setup, dt=dt, dv=float(data["dv"]),
                                     route=collision_route)
    seeding = SeedingRunner(
        population, multiplicity=data["seed/multiplicity"],
        extensive={MASS_ROW: data["seed/mass"]}, dt=dt, seed=seed, route=route,
        injection_rate=lambda time: int(rates[int(round(time / dt))]))
    for _ in range(len(rates)):
        if collisions is not None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                collisions.run(1)
        seeding.step()
        population.refresh_bookkeeping()
        population.compact()
        yield {"idx": engine.download(population.perm)[:population.live],
               "length": population.live,
               "multiplicity": engine.download(population.multiplicity),
               "attributes": engine.download(population.extensive),
               "seed_index": seeding.seed_index()}


def assert_box_step(got, data, step, what):
    length = int(data["length"][step])
    assert got["length"] == length, f"{what} step {step}: length"
    assert_same_bits(got["idx"], data["idx"][step][:length], f"{what} step {step}: idx")
    for key in ("multiplicity", "attributes", "seed_index"):
        assert_same_bits(got[key], data[key][step], f"{what} step {step}: {key}")

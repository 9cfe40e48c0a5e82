#!/usr/bin/env python3
"""Generates the seeding goldens (tests/golden/seed_*.npz) by RUNNING THE REFERENCE (PySDM at
/root/reference) in its pure-Python mode, with the same no-JIT import as gen_golden.py (the
stand-ins of tests/golden/standins put in front of it).  Run as:

    PYTHONDONTWRITEBYTECODE=1 CI=1 python3 -B tests/golden/gen_seeding_golden.py

Written:
  seed_methods.npz   direct `backend.seeding` calls on seeded states (free slots scattered over
      the slots, a few of them right at the start and at the end): inputs and outputs, the -1
      entries of `idx` included.  Seed indices identity, permuted, repeated and all equal; 1 and 3
      attribute rows; K = 1, part of the reservoir, all of it, and K = the number of free slots.
  seed_box.npz       an unmodified Builder + Box + Seeding alone: 64 slots of which 24 are in use,
      a reservoir of 10 seeds, rate 0 / 1 / 2 by time over 16 steps.
  seed_box_coal.npz  Box + Coalescence(Golovin) + Seeding: 128 slots of which 96 are in use with
      multiplicities 1..3 (the "deaths" set-up of gen_golden.py, dv scaled to the size), so that
      coalescence empties slots during the run and seeding refills them; asserted: slots die,
      and at least one slot that died is refilled.
  The two box goldens hold, per step: idx[:length] (the tail is stored as -1), the length,
  multiplicity, attributes and the seed index as the reference holds them after the step.
"""
# pylint: disable=wrong-import-position,import-error,too-many-locals,protected-access
import os
import sys
import warnings

os.environ.setdefault("CI", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "standins"), "/root/reference"]

import numpy as np

from PySDM import Builder, Formulae
from PySDM.backends import CPU
from PySDM.dynamics import Coalescence, Seeding
from PySDM.dynamics.collisions.collision_kernels import Golovin
from PySDM.environments import Box

OUT = HERE
PRIVATE = "_ParticleAttributes__"


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


# ---- seed_methods ----------------------------------------------------------------------------------
N_SD, MAX_ROWS, MAX_SEEDS = 64, 3, 24


def methods(seed=20261018):
    """all calls in one set of stacked arrays (rows / seeds beyond a call's n_attr / n_seeds are
    padding: zeros, seed index -1); attribute values are multiples of 2^-10, which are copied like
    any others and compress"""
    rng = np.random.default_rng(seed)
    backend = CPU(Formulae())
    S = backend.Storage
    calls = []
    for n_attr in (1, 3):
        for n_seeds, index_kind in ((1, "identity"), (10, "identity"), (10, "permuted"),
                                    (10, "repeated"), (10, "equal"), (MAX_SEEDS, "permuted")):
            for how_many in ("one", "half", "all", "every_free_slot"):
                free = rng.uniform(size=N_SD) < 0.2
                free[[0, 1, N_SD - 1]] = True
                free[2] = False
                while free.sum() < n_seeds + 3:  # room for the largest K of this reservoir
                    free[rng.integers(3, N_SD - 1)] = True
                multiplicity = np.where(free, 0, rng.integers(1, 1000, N_SD)).astype(np.int64)
                attributes = 1 + rng.integers(0, 1024, (n_attr, N_SD)) / 1024
                idx = rng.permutation(N_SD).astype(np.int64)
                seed_multiplicity = rng.integers(1, 10 ** 6, n_seeds).astype(np.int64)
                seed_attributes = 10 + rng.integers(0, 1024, (n_attr, n_seeds)) / 1024
                index = {"identity": np.arange(n_seeds), "permuted": rng.permutation(n_seeds),
                         "repeated": rng.integers(0, n_seeds, n_seeds),
                         "equal": np.full(n_seeds, n_seeds // 2)}[index_kind].astype(np.int64)
                k = {"one": 1, "half": max(1, n_seeds // 2), "all": n_seeds,
                     "every_free_slot": n_seeds}[how_many]
                if how_many == "every_free_slot":  # exactly as many free slots as are asked for
                    multiplicity[np.flatnonzero(free)[k:]] = 7
                args = {"idx": S.from_ndarray(idx), "multiplicity": S.from_ndarray(multiplicity),
                        "extensive_attributes": S.from_ndarray(attributes),
                        "seeded_particle_index": S.from_ndarray(index),
                        "seeded_particle_multiplicity": S.from_ndarray(seed_multiplicity),
                        "seeded_particle_extensive_attributes": S.from_ndarray(seed_attributes)}
                backend.seeding(**args, number_of_super_particles_to_inject=k)
                out_idx = args["idx"].to_ndarray()
                assert (out_idx == -1).sum() == k

                def rows(values, width):
                    padded = np.zeros((MAX_ROWS, width))
                    padded[:values.shape[0], :values.shape[1]] = values
                    return padded

                def seeds(values, fill):
                    padded = np.full(MAX_SEEDS, fill, dtype=np.int64)
                    padded[:values.shape[0]] = values
                    return padded

                calls.append({
                    "in_idx": idx, "in_multiplicity": multiplicity,
                    "in_attributes": rows(attributes, N_SD), "seed_index": seeds(index, -1),
                    "seed_multiplicity": seeds(seed_multiplicity, 0),
                    "seed_attributes": rows(seed_attributes, MAX_SEEDS), "k": k,
                    "n_attr": n_attr, "n_seeds": n_seeds,
                    "kind": f"{n_attr} rows, {n_seeds} seeds {index_kind}, {how_many}",
                    "out_idx": out_idx, "out_multiplicity": args["multiplicity"].to_ndarray(),
                    "out_attributes": rows(args["extensive_attributes"].to_ndarray(), N_SD)})
    arrays = {key: np.asarray([call[key] for call in calls]) for key in calls[0]}
    arrays["n_calls"] = np.asarray(len(calls))
    save("seed_methods", **arrays)


# ---- the boxes -------------------------------------------------------------------------------------
def box(name, *, n_sd, in_use, reservoir, rates, dt, dv, seed, coalescence, multiplicities):
    rng = np.random.default_rng(seed)
    formulae = Formulae(seed=seed)
    builder = Builder(n_sd=n_sd, backend=CPU(formulae), environment=Box(dt=dt, dv=dv))
    if coalescence:
        builder.add_dynamic(Coalescence(collision_kernel=Golovin(b=1.5e3), adaptive=False))
    used = np.zeros(n_sd, dtype=bool)
    used[rng.permutation(n_sd)[:in_use]] = True
    radius = np.exp(rng.uniform(np.log(5e-6), np.log(40e-6), n_sd))
    mass = formulae.constants.rho_w * formulae.constants.PI_4_3 * radius ** 3
    multiplicity = np.where(used, multiplicities(rng, n_sd).astype(float), np.nan)
    seed_mass = formulae.constants.rho_w * formulae.constants.PI_4_3 * np.exp(
        rng.uniform(np.log(1e-6), np.log(3e-6), reservoir)) ** 3
    seed_multiplicity = multiplicities(rng, reservoir).astype(float)
    rates = np.asarray(rates, dtype=np.int64)
    attributes = {"multiplicity": multiplicity, "water mass": np.where(used, mass, 0.0)}
    particulator_box = []

    def rate(time):
        return int(rates[int(round(time / dt))])

    key_probe = Builder(n_sd=n_sd, backend=CPU(formulae), environment=Box(dt=dt, dv=dv))
    if coalescence:
        key_probe.add_dynamic(Coalescence(collision_kernel=Golovin(b=1.5e3), adaptive=False))
    keys = tuple(key_probe.build(attributes={k: v.copy() for k, v in attributes.items()},
                                 products=()).attributes.get_extensive_attribute_keys())
    assert len(keys) == 1, keys
    builder.add_dynamic(Seeding(
        super_droplet_injection_rate=rate,
        seeded_particle_extensive_attributes={keys[0]: seed_mass.copy()},
        seeded_particle_multiplicity=seed_multiplicity.copy()))
    particulator = builder.build(attributes={k: v.copy() for k, v in attributes.items()},
                                 products=())
    particulator_box.append(particulator)
    attrs = particulator.attributes
    seeding = particulator.dynamics["Seeding"]
    per_step = {k: [] for k in ("idx", "length", "multiplicity", "attributes", "seed_index")}
    ever_dead = np.zeros(n_sd, dtype=bool)
    refilled = 0
    previous = attrs["multiplicity"].to_ndarray(raw=True).copy()
    for _ in range(len(rates)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            particulator.run(steps=1)
        idx = getattr(attrs, PRIVATE + "idx")
        length = len(idx)
        raw = idx.to_ndarray()
        stored = np.full(n_sd, -1, dtype=np.int64)
        stored[:length] = raw[:length]
        now = attrs["multiplicity"].to_ndarray(raw=True).copy()
        refilled += int(((now != 0) & ever_dead & (previous == 0)).sum())
        ever_dead |= used & (now == 0)
        ever_dead |= (previous != 0) & (now == 0)
        previous = now
        per_step["idx"].append(stored)
        per_step["length"].append(length)
        per_step["multiplicity"].append(now)
        per_step["attributes"].append(
            attrs.get_extensive_attribute_storage().to_ndarray(raw=True).copy())
        per_step["seed_index"].append(seeding.index.to_ndarray().copy())
    died = int(ever_dead.sum())
    print(f"{name}: {died} slots died, {refilled} refills of slots that had died, "
          f"{int(rates.sum())} injections, final length {per_step['length'][-1]}")
    if coalescence:
        assert died > 0 and refilled > 0, "no slot died and was refilled"
    arrays = {k: np.asarray(v) for k, v in per_step.items()}
    arrays.update({
        "init/multiplicity": multiplicity, "init/mass": attributes["water mass"],
        "seed/multiplicity": seed_multiplicity, "seed/mass": seed_mass, "rates": rates,
        "row": np.asarray(keys[0]), "dt": np.asarray(float(dt)), "dv": np.asarray(float(dv)),
        "seed": np.asarray(seed), "coalescence": np.asarray(int(coalescence)),
        "golovin_b": np.asarray(1.5e3)})
    save(name, **arrays)


def boxes():
    box("seed_box", n_sd=64, in_use=24, reservoir=10,
        rates=[0, 1, 2, 0, 2, 1, 0, 0, 2, 2, 1, 0, 1, 2, 0, 1], dt=1.0, dv=1.0, seed=44,
        coalescence=False, multiplicities=lambda rng, n: rng.integers(1, 10 ** 6, n))
    box("seed_box_coal", n_sd=128, in_use=96, reservoir=10,
        rates=[0, 2, 1, 0, 2, 2, 0, 1, 2, 0, 1, 2, 2, 0, 1, 2], dt=200.0, dv=6e-4 * 96 / 1024,
        seed=45, coalescence=True, multiplicities=lambda rng, n: 1 + rng.integers(0, 3, n))


if __name__ == "__main__":
    what = sys.argv[1:] or ["methods", "boxes"]
    if "methods" in what:
        methods()
    if "boxes" in what:
        boxes()

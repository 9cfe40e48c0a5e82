#!/usr/bin/env python3
"""Generates the goldens of the fall-velocity laws (tests/golden/traj_velocity_*.npz) by RUNNING
THE REFERENCE (PySDM at /root/reference) in its pure-Python mode, with the same no-JIT import as
gen_golden.py (the stand-ins of tests/golden/standins put in front of it).  Run as:

    PYTHONDONTWRITEBYTECODE=1 CI=1 python3 -B tests/golden/gen_velocity_law_golden.py

Written (every run: an unmodified Builder, one collision dynamic, Geometric kernel):
  traj_velocity_rogers_yau.npz, traj_velocity_power_series.npz
      a box of 1024 slots, Coalescence, adaptive, 4 steps, the planted input of
      tests/velocity_law_cases.py: radii on, and up to eight ulps beside, both limits of Rogers-Yau.
  traj_velocity_4x4_rogers_yau.npz
      the same input spread over 4 x 4 cells, exactly 64 slots in each (a random permutation of
      the slots, modulo 16), Rogers-Yau.
  traj_velocity_breakup_rogers_yau.npz
      a box of 256 rain drops, Collision(Straub2010Ec, ConstEb(1), AlwaysN(4)), Rogers-Yau
      (asserted: breakups happen).
Contents as gen_golden.py's trajectories: per recorded step idx, length, multiplicity, attributes,
cell_start and the counters, keyed step<k>/<name>; init/volume, init/multiplicity
[, init/cell_id, grid]; cfg = [n_sd, seed, adaptive, dt, dv].
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
from PySDM.dynamics import Coalescence, Collision
from PySDM.dynamics.collisions.breakup_efficiencies import ConstEb
from PySDM.dynamics.collisions.breakup_fragmentations import AlwaysN
from PySDM.dynamics.collisions.coalescence_efficiencies import Straub2010Ec
from PySDM.dynamics.collisions.collision_kernels import Geometric
from PySDM.environments import Box
from PySDM.impl.mesh import Mesh

OUT = HERE
SEED = 44
STEPS = (1, 2, 3, 4)
PLANT_SEED = 20261019
LIMITS = (35e-6, 600e-6)  # ROGERS_YAU_TERM_VEL_{SMALL,MEDIUM}_R_LIMIT


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


def planted(n_sd=1024):
    """tests/velocity_law_cases.py:planted, restated (this script imports the reference only);
    tests/test_velocity_laws.py holds the two to each other through init/volume of the goldens"""
    rng = np.random.default_rng(PLANT_SEED)
    radius = np.exp(rng.uniform(np.log(5e-6), np.log(2e-3), n_sd))
    ulps = np.arange(-8, 9)
    for at, limit in enumerate(LIMITS):
        radius[at * len(ulps):(at + 1) * len(ulps)] = limit * (1 + ulps * 2.0 ** -52)
    multiplicity = 1 + rng.integers(0, 3, n_sd)
    return Formulae().constants.PI_4_3 * np.power(radius, 3), multiplicity.astype(np.int64)


def snapshot(particulator, dyn, breakup):
    attrs = particulator.attributes
    idx = attrs._ParticleAttributes__idx
    snap = {
        "idx": idx.to_ndarray(), "length": np.asarray(len(idx)),
        "multiplicity": attrs["multiplicity"].to_ndarray(raw=True),
        "attributes": attrs.get_extensive_attribute_storage().to_ndarray(raw=True),
        "cell_start": attrs.cell_start.to_ndarray(),
        "collision_rate": dyn.collision_rate.to_ndarray(),
        "collision_rate_deficit": dyn.collision_rate_deficit.to_ndarray(),
        "coalescence_rate": dyn.coalescence_rate.to_ndarray(),
        "stats_n_substep": dyn.stats_n_substep.to_ndarray(),
        "stats_dt_min": dyn.stats_dt_min.to_ndarray(),
    }
    if breakup:
        snap["breakup_rate"] = dyn.breakup_rate.to_ndarray()
        snap["breakup_rate_deficit"] = dyn.breakup_rate_deficit.to_ndarray()
    return snap


def trajectory(name, *, law, volume, multiplicity, dt, dv, breakup=False, grid=None, cell_id=None):
    n_sd = len(volume)
    formulae = Formulae(seed=SEED, terminal_velocity=law,
                        **({"fragmentation_function": "AlwaysN"} if breakup else {}))
    env = Box(dt=dt, dv=dv)
    if grid is not None:
        env.mesh = Mesh(grid, size=tuple(float(g) for g in grid))
        env.mesh.dv = dv
    builder = Builder(n_sd=n_sd, backend=CPU(formulae), environment=env)
    if breakup:
        builder.add_dynamic(Collision(
            collision_kernel=Geometric(), coalescence_efficiency=Straub2010Ec(),
            breakup_efficiency=ConstEb(1.0), fragmentation_function=AlwaysN(n=4),
            adaptive=True, warn_overflows=False))
    else:
        builder.add_dynamic(Coalescence(collision_kernel=Geometric(collection_efficiency=1),
                                        adaptive=True))
    attributes = {"volume": volume.copy(), "multiplicity": multiplicity.copy()}
    if cell_id is not None:
        attributes["cell id"] = cell_id.copy()
    particulator = builder.build(attributes)
    dyn = particulator.dynamics["Collision"]
    out = {}
    for step in STEPS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            particulator.run(step - particulator.n_steps)
        for key, value in snapshot(particulator, dyn, breakup).items():
            out[f"step{step}/{key}"] = value
    last = STEPS[-1]
    print(f"{name}: lengths {[int(out[f'step{s}/length']) for s in STEPS]}, coalescences "
          f"{int(out[f'step{last}/coalescence_rate'].sum())}, sub-steps "
          f"{out[f'step{last}/stats_n_substep'].max()}"
          + (f", breakups {int(out[f'step{last}/breakup_rate'].sum())}" if breakup else ""))
    if breakup:
        assert out[f"step{last}/breakup_rate"].sum() > 0, "no breakup"
    out.update({"init/volume": volume, "init/multiplicity": multiplicity,
                "cfg": np.asarray([n_sd, SEED, 1, dt, dv])})
    if grid is not None:
        out["grid"], out["init/cell_id"] = np.asarray(grid), cell_id
    save(name, **out)


if __name__ == "__main__":
    what = sys.argv[1:] or ["box", "4x4", "breakup"]
    plant_volume, plant_multiplicity = planted()
    if "box" in what:
        for tag, law_name in (("rogers_yau", "RogersYau"), ("power_series", "PowerSeries")):
            trajectory(f"traj_velocity_{tag}", law=law_name, volume=plant_volume,
                       multiplicity=plant_multiplicity, dt=1.0, dv=0.1)
    if "4x4" in what:
        cells = np.random.default_rng(PLANT_SEED + 1).permutation(len(plant_volume)) % 16
        trajectory("traj_velocity_4x4_rogers_yau", law="RogersYau", volume=plant_volume,
                   multiplicity=plant_multiplicity, dt=1.0, dv=0.1 / 16, grid=(4, 4),
                   cell_id=cells.astype(np.int64))
    if "breakup" in what:
        rng = np.random.default_rng(PLANT_SEED + 2)
        drops = np.exp(rng.uniform(np.log(0.2e-3), np.log(2e-3), 256))
        trajectory("traj_velocity_breakup_rogers_yau", law="RogersYau",
                   volume=Formulae().constants.PI_4_3 * drops ** 3,
                   multiplicity=rng.integers(2, 50, 256).astype(np.int64), dt=1.0, dv=1e-2,
                   breakup=True)

#!/usr/bin/env python3
"""Generates the relaxed-velocity goldens (tests/golden/relax_*.npz) by RUNNING THE REFERENCE
(PySDM at /root/reference) in its pure-Python mode, with the same no-JIT import as gen_golden.py
(the stand-ins of tests/golden/standins put in front of it).  Run as:

    PYTHONDONTWRITEBYTECODE=1 CI=1 python3 -B tests/golden/gen_relaxed_velocity_golden.py

Written (every run: an unmodified Builder, the dynamics in the order named):
  relax_box.npz           Box + RelaxedVelocity alone: 64 slots, radii 1 um .. 3 mm, both
      `constant` settings x c in {1e-12, 8, 100, 1e15} x the momentum starting from zero and from
      half of init_fall_momenta; the momentum row after each of 8 steps.
  relax_box_coal.npz      Box + RelaxedVelocity(c=1000) + Coalescence(Geometric, adaptive=False): 64
      slots with multiplicities 1..3 (asserted: slots die), the momentum starting from half.
  relax_box_breakup.npz   Box + RelaxedVelocity(c=1000) + Collision(Geometric, Straub2010Ec,
      ConstEb(1), AlwaysN(4)) (asserted: breakups happen).
  relax_4x4.npz           the same coalescence in 16 cells, 256 slots.
  relax_disp.npz          the set-up of traj_disp2d_implicit_sed (gen_golden.py) with
      RelaxedVelocity(c=200) registered ahead of the Displacement.
  The collision goldens hold per step what gen_golden.py's trajectories hold (idx, length,
  multiplicity, attributes, cell_start, the counters), keyed step<k>/<name>.
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
from PySDM.dynamics import Coalescence, Collision, Displacement, RelaxedVelocity
from PySDM.dynamics.collisions.breakup_efficiencies import ConstEb
from PySDM.dynamics.collisions.breakup_fragmentations import AlwaysN
from PySDM.dynamics.collisions.coalescence_efficiencies import Straub2010Ec
from PySDM.dynamics.collisions.collision_kernels import Geometric
from PySDM.environments import Box
from PySDM.impl.mesh import Mesh
from PySDM.initialisation.init_fall_momenta import init_fall_momenta

OUT = HERE
C_VALUES = (1e-12, 8.0, 100.0, 1e15)
STEPS = 8


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


def masses(formulae, rng, n_sd, low, high):
    radius = np.exp(rng.uniform(np.log(low), np.log(high), n_sd))
    return formulae.constants.rho_w * formulae.constants.PI_4_3 * radius ** 3


def relax_box(seed=20261018, n_sd=64, dt=1.0):
    rng = np.random.default_rng(seed)
    formulae = Formulae(seed=44, terminal_velocity="GunnKinzer1949")
    mass = masses(formulae, rng, n_sd, 1e-6, 3e-3)
    multiplicity = rng.integers(1, 10 ** 6, n_sd).astype(float)
    starts = np.stack([init_fall_momenta(mass, zero=True), 0.5 * init_fall_momenta(mass)])
    momentum = np.empty((2, len(C_VALUES), len(starts), STEPS, n_sd))
    rows = None
    for constant in (False, True):
        for at_c, c in enumerate(C_VALUES):
            for at_start, start in enumerate(starts):
                builder = Builder(n_sd=n_sd, backend=CPU(formulae),
                                  environment=Box(dt=dt, dv=1.0))
                builder.add_dynamic(RelaxedVelocity(c=c, constant=constant))
                particulator = builder.build(attributes={
                    "multiplicity": multiplicity.copy(), "water mass": mass.copy(),
                    "relative fall momentum": start.copy()}, products=())
                attrs = particulator.attributes
                rows = tuple(attrs.get_extensive_attribute_keys())
                for step in range(STEPS):
                    particulator.run(steps=1)
                    momentum[int(constant), at_c, at_start, step] = attrs[
                        "relative fall momentum"].to_ndarray(raw=True)
    assert np.isfinite(momentum).all()
    save("relax_box", mass=mass, multiplicity=multiplicity, starts=starts, momentum=momentum,
         c=np.asarray(C_VALUES), dt=np.asarray(dt), rows=np.asarray(rows))


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
    }
    if breakup:
        snap["breakup_rate"] = dyn.breakup_rate.to_ndarray()
        snap["breakup_rate_deficit"] = dyn.breakup_rate_deficit.to_ndarray()
    return snap


def collisions(name, *, n_sd, seed, dt, dv, breakup, radii, multiplicities, grid=None, c=1000.0,
               relaxed=True):
    """`relaxed=False`: the same run without RelaxedVelocity (fall velocity = terminal velocity);
    returns the final multiplicities and writes nothing"""
    rng = np.random.default_rng(seed)
    formulae = Formulae(seed=seed, terminal_velocity="GunnKinzer1949",
                        fragmentation_function="AlwaysN")
    env = Box(dt=dt, dv=dv)
    cell_id = None
    if grid is not None:
        env.mesh = Mesh(grid, size=tuple(float(g) for g in grid))
        env.mesh.dv = dv
        cell_id = rng.integers(0, int(np.prod(grid)), n_sd).astype(np.int64)
    builder = Builder(n_sd=n_sd, backend=CPU(formulae), environment=env)
    if relaxed:
        builder.add_dynamic(RelaxedVelocity(c=c, constant=False))
    if breakup:
        builder.add_dynamic(Collision(
            collision_kernel=Geometric(), coalescence_efficiency=Straub2010Ec(),
            breakup_efficiency=ConstEb(1.0), fragmentation_function=AlwaysN(n=4),
            adaptive=False, warn_overflows=False))
    else:
        builder.add_dynamic(Coalescence(collision_kernel=Geometric(), adaptive=False))
    mass = masses(formulae, rng, n_sd, *radii)
    multiplicity = multiplicities(rng, n_sd).astype(float)
    momentum = 0.5 * init_fall_momenta(mass)
    attributes = {"multiplicity": multiplicity, "water mass": mass}
    if relaxed:
        attributes["relative fall momentum"] = momentum
    if cell_id is not None:
        attributes["cell id"] = cell_id
    particulator = builder.build(attributes={k: v.copy() for k, v in attributes.items()},
                                 products=())
    dyn = particulator.dynamics["Collision"]
    rows = tuple(particulator.attributes.get_extensive_attribute_keys())
    out = {}
    lengths = []
    for step in range(1, STEPS + 1):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            particulator.run(steps=1)
        for key, value in snapshot(particulator, dyn, breakup).items():
            out[f"step{step}/{key}"] = value
        lengths.append(int(out[f"step{step}/length"]))
    if not relaxed:
        return out[f"step{STEPS}/multiplicity"]
    # the time scale must matter: with the terminal velocity the run ends elsewhere
    plain = collisions(name, n_sd=n_sd, seed=seed, dt=dt, dv=dv, breakup=breakup, radii=radii,
                       multiplicities=multiplicities, grid=grid, relaxed=False)
    assert (plain != out[f"step{STEPS}/multiplicity"]).any(), "indistinguishable from terminal"
    print(f"{name}: lengths {lengths}, collisions "
          f"{int(out[f'step{STEPS}/collision_rate'].sum())}"
          + (f", breakups {int(out[f'step{STEPS}/breakup_rate'].sum())}" if breakup else ""))
    if breakup:
        assert out[f"step{STEPS}/breakup_rate"].sum() > 0, "no breakup"
    else:
        assert lengths[-1] < n_sd, "no slot died"
    out.update({"init/multiplicity": multiplicity, "init/mass": mass, "init/momentum": momentum,
                "rows": np.asarray(rows), "dt": np.asarray(float(dt)), "dv": np.asarray(float(dv)),
                "seed": np.asarray(seed), "c": np.asarray(c), "breakup": np.asarray(int(breakup)),
                "steps": np.asarray(STEPS)})
    if grid is not None:
        out["grid"], out["init/cell_id"] = np.asarray(grid), cell_id
    save(name, **out)


def displacement(name="relax_disp", c=200.0):
    """gen_golden.py:gen_displacement, case disp2d_implicit_sed, with RelaxedVelocity"""
    grid, size, dt, n_sd, steps = (6, 5), (600.0, 500.0), 5.0, 400, 6
    rng = np.random.default_rng(len("disp2d_implicit_sed") * 7919)
    formulae = Formulae(seed=44, particle_advection="ImplicitInSpace",
                        terminal_velocity="GunnKinzer1949")
    env = Box(dt=dt, dv=None)
    env.mesh = Mesh(grid, size)
    builder = Builder(n_sd=n_sd, backend=CPU(formulae), environment=env)
    builder.add_dynamic(RelaxedVelocity(c=c, constant=False))
    builder.add_dynamic(Displacement(enable_sedimentation=True, adaptive=True,
                                     precipitation_counting_level_index=0))
    positions = rng.uniform(0, 1, (len(grid), n_sd)) * np.asarray(grid).reshape(-1, 1)
    cell_id, cell_origin, position_in_cell = env.mesh.cellular_attributes(positions)
    radius = np.exp(rng.uniform(np.log(10e-6), np.log(1.5e-3), n_sd))
    mass = formulae.constants.rho_w * formulae.trivia.volume(radius=radius)
    mult = rng.integers(1, 10**5, n_sd).astype(float)
    momentum = 0.5 * init_fall_momenta(mass)
    particulator = builder.build({
        "water mass": mass.copy(), "multiplicity": mult.copy(), "cell id": cell_id.copy(),
        "cell origin": cell_origin.copy(), "position in cell": position_in_cell.copy(),
        "relative fall momentum": momentum.copy()}, products=())
    courant = tuple(
        rng.uniform(-0.45, 0.45, tuple(g + (1 if a == d else 0) for a, g in enumerate(grid)))
        for d in range(len(grid)))
    disp = particulator.dynamics["Displacement"]
    disp.upload_courant_field(courant)
    attrs = particulator.attributes
    out = {"grid": np.asarray(grid), "size": np.asarray(size), "dt": np.asarray(dt),
           "steps": np.asarray(steps), "c": np.asarray(c), "init/mass": mass,
           "init/multiplicity": mult, "init/positions": positions, "init/momentum": momentum,
           "rows": np.asarray(tuple(attrs.get_extensive_attribute_keys())),
           "n_substeps": np.asarray(disp._n_substeps)}
    for d, component in enumerate(courant):
        out[f"courant/{d}"] = component
    for step in range(1, steps + 1):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            particulator.run(1)
        attrs.sanitize()
        out[f"step{step}/length"] = np.asarray(attrs.super_droplet_count)
        out[f"step{step}/idx"] = attrs._ParticleAttributes__idx.to_ndarray()
        out[f"step{step}/precipitation"] = np.asarray(disp.precipitation_mass_in_last_step)
        for key, tag in (("cell origin", "cell_origin"), ("position in cell", "position"),
                         ("cell id", "cell_id"), ("multiplicity", "multiplicity"),
                         ("water mass", "mass"), ("relative fall momentum", "momentum")):
            out[f"step{step}/{tag}"] = attrs[key].to_ndarray(raw=True)
    print(f"{name}: lengths {[int(out[f'step{s}/length']) for s in range(1, steps + 1)]}")
    save(name, **out)


if __name__ == "__main__":
    what = sys.argv[1:] or ["box", "coal", "breakup", "4x4", "disp"]
    small = lambda rng, n: 1 + rng.integers(0, 3, n)  # noqa: E731
    if "box" in what:
        relax_box()
    if "coal" in what:
        collisions("relax_box_coal", n_sd=64, seed=44, dt=1.0, dv=1e-2, breakup=False,
                   radii=(10e-6, 1e-3), multiplicities=small)
    if "breakup" in what:
        collisions("relax_box_breakup", n_sd=64, seed=45, dt=1.0, dv=1e-2, breakup=True,
                   radii=(0.2e-3, 2e-3), multiplicities=lambda rng, n: rng.integers(2, 50, n))
    if "4x4" in what:
        collisions("relax_4x4", n_sd=256, seed=46, dt=1.0, dv=1e-3, breakup=False,
                   radii=(10e-6, 1e-3), multiplicities=small, grid=(4, 4))
    if "disp" in what:
        displacement()

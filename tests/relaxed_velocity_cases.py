"""Shared by the relaxed-velocity tests (tests/test_relaxed_velocity_checker.py on the CPU,
tests/test_hip_relaxed_velocity.py on the device): the recorded goldens (tests/golden/relax_*.npz,
written by tests/golden/gen_relaxed_velocity_golden.py from the reference), planted states, the
call of the one symbol of include/sdm_relaxed_velocity.h on any engine, and the recorded runs on
this package's runners.

Bounds.  The reference evaluates exp and power through libm / NumPy, this package through
sdm_math.h, and the momentum accumulates over a run.  Measured on the CPU checker against
relax_box.npz (16 runs of 8 steps):
  * largest relative difference over the runs with c in {1e-12, 8, 100}: 1.144e-14
    -> RELATIVE_BOUND = 4 x that;
  * c = 1e15: 3.52e-3.  Not an error of either side: scale = 1 - exp(-dt / tau) with
    dt / tau ~ 1e-15 .. 1e-12 cancels to a few multiples of 2^-53, so one unit in the last place
    of exp(-dt / tau) - which libm and sdm_math.h are both entitled to - is up to a tenth of the
    scale factor, and of the momentum that started from zero.  The quantity that is well
    conditioned there is the difference over the terminal momentum (terminal velocity x mass, what
    the momentum relaxes to): 8.88e-16 over ALL 16 runs -> NORMALISED_BOUND = 4 x that, applied
    to every run; the relative bound to the twelve runs where the scale factor carries its digits.
Integers (multiplicities, permutation, counters) are compared for equality.
"""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

from pysdm_amd import abi
from pysdm_amd import recipe as R
from pysdm_amd.collisions import CollisionRunner
from pysdm_amd.displacement import DisplacementRunner
from pysdm_amd.population import MASS_ROW, MOMENTUM_ROW, Population, locate
from pysdm_amd.relaxed_velocity import (LAW_CODES, RelaxedVelocityRunner, init_fall_momenta)
from pysdm_amd.terminal_velocity import (TABLE_POINTS_PER_METRE, TABLE_TOP, RogersYau,
                                         gunn_kinzer_table)

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"
GOLDEN = os.path.join(HERE, "golden")
MEASURED_RELATIVE = 1.144e-14    # checker against relax_box.npz, c in {1e-12, 8, 100}
MEASURED_NORMALISED = 8.882e-16  # the same over all runs, differences over the terminal momentum
RELATIVE_BOUND = 4 * MEASURED_RELATIVE
NORMALISED_BOUND = 4 * MEASURED_NORMALISED
ILL_CONDITIONED_C = 1e15         # 1 - exp(-dt / tau) cancels (see the module docstring)
C_VALUES = (1e-12, 8.0, 100.0, 1e15)
RHO_W = 1000.0
# relaxed_velocity.hip: slots per workgroup and per pass of the capped grid
# (SDM_BLOCK * RV_PER_THREAD, RV_GRID_CAP workgroups)
WORKGROUP, GRID_PASS = 256 * 2, 2048 * 256 * 2


@functools.lru_cache(maxsize=None)
def gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def bits(values):
    return np.ascontiguousarray(values).view(np.uint64)


def assert_same_doubles(got, want, what):
    """bit for bit wherever neither side is NaN; the NaN positions equal (the sign of a NaN from
    0 / 0 is the processor's choice)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{what}: NaN positions")
    keep = ~np.isnan(got)
    np.testing.assert_array_equal(bits(got[keep]), bits(want[keep]), err_msg=what)


def mass_of_radius(radius):
    return RHO_W * (4 / 3 * np.pi) * np.asarray(radius, dtype=float) ** 3


# ---- the one symbol on host arrays -------------------------------------------------------------------
def make_cfg(n_sd, *, dt, c, constant, law):
    cfg = abi.RelaxedVelocityCfg()
    cfg.n_sd, cfg.dt, cfg.c, cfg.constant = int(n_sd), float(dt), float(c), int(constant)
    cfg.rho_w, cfg.law = RHO_W, LAW_CODES[law]
    cfg.gk_table_len, cfg.gk_factor = len(gunn_kinzer_table()[0]), float(TABLE_POINTS_PER_METRE)
    cfg.gk_top = float(TABLE_TOP)
    cfg.rogers_yau = (abi.c_f64 * 5)(*RogersYau().consts)
    return cfg


def call_step(engine, mass, momentum, *, dt=1.0, c=8.0, constant=False, law="GunnKinzer1949",
              with_velocity=True, row=None, mass_row=0, velocity_offset=0, n_calls=1):
    """sdm_relaxed_velocity_step on copies.  `row`: None - the columns are arrays of their own;
    k - the momentum is row k and the mass row `mass_row` of one block (for odd n_sd rows of odd
    k are only 8-byte aligned).  `velocity_offset`: the velocity column starts that many doubles
    into its allocation (1: only 8-byte aligned).  Returns momentum, velocity (or None) and the
    status."""
    n_sd = int(mass.shape[0])
    if row is None:
        mass_dev, momentum_dev = engine.upload(mass.copy()), engine.upload(momentum.copy())
    else:
        assert row != mass_row
        block = np.zeros((max(row, mass_row) + 1, n_sd))
        block[mass_row], block[row] = mass, momentum
        block_dev = engine.upload(block)
        mass_dev, momentum_dev = block_dev[mass_row], block_dev[row]
    velocity = None
    if with_velocity:
        velocity = engine.full(n_sd + velocity_offset, np.float64, -7.0)[velocity_offset:]
    status = engine.full(2, np.int64, -7)
    table = tuple(engine.upload(np.array(t)) for t in gunn_kinzer_table())
    cfg = make_cfg(n_sd, dt=dt, c=c, constant=constant, law=law)
    for _ in range(n_calls):
        engine.relaxed_velocity_call("sdm_relaxed_velocity_step", cfg, mass_dev, momentum_dev,
                                     velocity, *table, status)
    return {"momentum": engine.download(momentum_dev),
            "velocity": engine.download(velocity) if with_velocity else None,
            "status": engine.download(status), "mass": engine.download(mass_dev)}


def planted_state(n_sd, seed=1):
    """radii log-uniform over 1 um .. 5.9 mm with, as far as n_sd allows, the planted slots: mass
    0, a negative mass (the sign of ice), radii on table knots (10 um apart), at the 40 um change
    of regime and at the table top; momenta equal to the terminal momentum, zero and negative"""
    rng = np.random.default_rng(seed)
    radius = np.exp(rng.uniform(np.log(1e-6), np.log(5.9e-3), n_sd))
    special = [0.0, 50e-6, 40e-6, 10e-6, 5.99e-3, 35e-6, 600e-6, 3.0e-3, 20e-6]
    for at, value in enumerate(special[:n_sd]):
        radius[(at * 7) % n_sd] = value
    mass = mass_of_radius(radius)
    # (the top itself and the first radius above it: `mass_at_table_top`)
    if n_sd > 12:
        mass[11] = -mass[11]
    momentum = mass * rng.uniform(0.0, 9.0, n_sd)
    if n_sd > 20:
        momentum[13], momentum[17] = 0.0, -momentum[17]
    return mass, momentum


def terminal_momentum(engine, mass, law="GunnKinzer1949"):
    return init_fall_momenta(engine, mass, law)


def mass_at_table_top(engine):
    """(the largest mass whose radius, derived as the library derives it, does not exceed the table
    top; the next double, whose radius does)"""
    def radius(mass):
        population = Population(engine, multiplicity=np.ones(2, dtype=np.int64),
                                mass=np.asarray([mass, mass]))
        return float(engine.download(population.radius())[0])

    mass = float(mass_of_radius(TABLE_TOP))
    while radius(mass) > TABLE_TOP:
        mass = float(np.nextafter(mass, 0.0))
    while radius(float(np.nextafter(mass, np.inf))) <= TABLE_TOP:
        mass = float(np.nextafter(mass, np.inf))
    return mass, float(np.nextafter(mass, np.inf))


# ---- recorded runs on the runners --------------------------------------------------------------------
def population_from(engine, data, *, cell_id=None, grid=None, **more):
    rows = [str(name) for name in data["rows"]]
    assert rows == [MASS_ROW, MOMENTUM_ROW]
    return Population(engine, multiplicity=data["init/multiplicity"], mass=data["init/mass"],
                      more_extensive={MOMENTUM_ROW: data["init/momentum"]},
                      velocity_source="momentum", cell_id=cell_id, grid=grid, **more)


def collision_setup(data):
    seed = int(data["seed"])
    if int(data["breakup"]):
        return R.CollisionSetup.collision(R.Geometric(), R.Straub2010Ec(), R.ConstEb(1.0),
                                          R.AlwaysN(n=4), seed=seed, adaptive=False,
                                          warn_overflows=False)
    return R.CollisionSetup.coalescence(R.Geometric(), seed=seed, adaptive=False)


def run_collisions(engine, name, *, collision_route, relax_route):
    """the recorded run: RelaxedVelocity, then the collisions, per step; yields (step, snapshot)"""
    data = gold(name)
    grid = tuple(int(g) for g in data["grid"]) if "grid" in data.files else None
    population = population_from(engine, data, grid=grid,
                                 cell_id=data["init/cell_id"] if grid else None)
    relax = RelaxedVelocityRunner(population, c=float(data["c"]), dt=float(data["dt"]),
                                  route=relax_route)
    collisions = CollisionRunner(population, collision_setup(data), dt=float(data["dt"]),
                                 dv=float(data["dv"]), route=collision_route, velocity="momentum")
    for step in range(1, int(data["steps"]) + 1):
        relax.step()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            collisions.run(1)
        snap = collisions.snapshot()
        snap.pop("stats_n_substep", None)
        snap.pop("stats_dt_min", None)
        yield step, snap


INT_KEYS = ("idx", "length", "multiplicity", "cell_start", "collision_rate",
            "collision_rate_deficit", "coalescence_rate", "breakup_rate", "breakup_rate_deficit")


def assert_collision_step(snap, data, step, what):
    length = int(snap["length"])
    for key, value in snap.items():
        want = data[f"step{step}/{key}"]
        tag = f"{what} step {step}: {key}"
        if key == "idx":
            value, want = value[:length], want[:length]
        if key in INT_KEYS:
            np.testing.assert_array_equal(value, want, err_msg=tag)
        else:
            np.testing.assert_allclose(value, want, rtol=RELATIVE_BOUND, atol=0, err_msg=tag)


def run_displacement(engine, *, route, relax_route):
    """relax_disp.npz: RelaxedVelocity, then the displacement with sedimentation, per step"""
    data = gold("relax_disp")
    grid = tuple(int(g) for g in data["grid"])
    size = tuple(float(v) for v in data["size"])
    cell_id, cell_origin, position_in_cell = locate(data["init/positions"], grid)
    population = population_from(engine, data, cell_id=cell_id, grid=grid,
                                 cell_origin=cell_origin, position_in_cell=position_in_cell)
    relax = RelaxedVelocityRunner(population, c=float(data["c"]), dt=float(data["dt"]),
                                  route=relax_route)
    displacement = DisplacementRunner(
        population, dt=float(data["dt"]), size=size, enable_sedimentation=True, adaptive=True,
        precipitation_counting_level_index=0, scheme="ImplicitInSpace", route=route)
    displacement.set_courant(tuple(data[f"courant/{d}"] for d in range(len(grid))))
    assert displacement.n_substeps == int(data["n_substeps"])
    down = engine.download
    for step in range(1, int(data["steps"]) + 1):
        relax.step()
        displacement.run()
        population.compact()
        tag = f"relax_disp step {step}"
        length = population.live
        assert length == int(data[f"step{step}/length"]), tag
        live = down(population.perm)[:length]
        np.testing.assert_array_equal(live, data[f"step{step}/idx"][:length], err_msg=tag)
        np.testing.assert_allclose(displacement.precipitation_mass_in_last_step,
                                   float(data[f"step{step}/precipitation"]),
                                   rtol=RELATIVE_BOUND, err_msg=tag)
        # (positions lie in [0, 1): the absolute term is the one tests/displacement_cases.py uses)
        for column, short, atol in ((population.cell_origin, "cell_origin", None),
                                    (population.cell_id, "cell_id", None),
                                    (population.multiplicity, "multiplicity", None),
                                    (population.position_in_cell, "position", 1e-13),
                                    (population.mass, "mass", 0.0),
                                    (population.momentum, "momentum", 0.0)):
            actual, expected = down(column)[..., live], data[f"step{step}/{short}"][..., live]
            if atol is None:
                np.testing.assert_array_equal(actual, expected, err_msg=f"{tag} {short}")
            else:
                np.testing.assert_allclose(actual, expected, rtol=RELATIVE_BOUND, atol=atol,
                                           err_msg=f"{tag} {short}")


def momentum_population(engine, mass, momentum, multiplicity=None):
    n_sd = len(mass)
    return Population(
        engine, multiplicity=np.ones(n_sd, dtype=np.int64) if multiplicity is None
        else multiplicity, mass=np.array(mass), more_extensive={MOMENTUM_ROW: np.array(momentum)},
        velocity_source="momentum")


# ---- the unmodified PySDM front-end -----------------------------------------------------------------
def import_reference():
    """PySDM in its pure-Python mode with the import-only stand-ins of tests/golden; skips the
    calling test where the reference tree is absent"""
    if not os.path.isdir(os.path.join(REFERENCE, "PySDM")):
        pytest.skip("reference tree not present")
    os.environ.setdefault("CI", "1")
    sys.dont_write_bytecode = True
    added = [os.path.join(HERE, "golden", "standins"), REFERENCE]
    sys.path[:0] = added
    try:
        import PySDM  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.dynamics import Coalescence, RelaxedVelocity  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.dynamics.collisions.collision_kernels import Geometric  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.environments import Box  # pylint: disable=import-outside-toplevel,import-error
    finally:
        for path in added:
            sys.path.remove(path)
    return {"PySDM": PySDM, "Coalescence": Coalescence, "RelaxedVelocity": RelaxedVelocity,
            "Geometric": Geometric, "Box": Box}


def run_pysdm_box(ref, backend_class, data, *, fuse_relaxation, fuse_collisions):
    """relax_box_coal.npz through PySDM's own front-end (shared with
    tests/test_hip_relaxed_velocity.py); yields (step, snapshot)"""
    from pysdm_amd.pysdm_plugin import as_pysdm_backend, fuse  # pylint: disable=import-outside-toplevel

    formulae = ref["PySDM"].Formulae(seed=int(data["seed"]), terminal_velocity="GunnKinzer1949")
    n_sd = data["init/multiplicity"].shape[0]
    builder = ref["PySDM"].Builder(
        n_sd=n_sd, backend=as_pysdm_backend(backend_class)(formulae),
        environment=ref["Box"](dt=float(data["dt"]), dv=float(data["dv"])))
    relaxation = ref["RelaxedVelocity"](c=float(data["c"]), constant=False)
    builder.add_dynamic(fuse(relaxation) if fuse_relaxation else relaxation)
    collisions = ref["Coalescence"](collision_kernel=ref["Geometric"](), adaptive=False)
    builder.add_dynamic(fuse(collisions) if fuse_collisions else collisions)
    particulator = builder.build(attributes={
        "multiplicity": data["init/multiplicity"].copy(), "water mass": data["init/mass"].copy(),
        "relative fall momentum": data["init/momentum"].copy()}, products=())
    assert "RelaxedVelocity" in particulator.dynamics
    attrs = particulator.attributes
    dyn = particulator.dynamics["Collision"]
    for step in range(1, int(data["steps"]) + 1):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            particulator.run(steps=1)
        idx = attrs._ParticleAttributes__idx  # pylint: disable=protected-access
        yield step, {
            "idx": idx.to_ndarray(), "length": np.asarray(len(idx)),
            "multiplicity": attrs["multiplicity"].to_ndarray(raw=True),
            "attributes": attrs.get_extensive_attribute_storage().to_ndarray(raw=True),
            "collision_rate": dyn.collision_rate.to_ndarray(),
            "coalescence_rate": dyn.coalescence_rate.to_ndarray()}

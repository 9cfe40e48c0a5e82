"""The relaxed-fall-velocity path on the device (pysdm_amd/csrc/relaxed_velocity.hip) against the
CPU checker of include/sdm_relaxed_velocity.h and against the goldens recorded from the reference.

Kernel against checker: bit for bit wherever neither side is NaN, the NaN positions equal (0 / 0
of a slot of mass 0 has the processor's sign).  Sizes: 1, around a wave (63, 64, 65), around what
one workgroup takes (W - 1, W, W + 1 with W = 512 slots), around one pass of the capped grid
(G - 1, G, G + 1 with G = 2^20 slots), and odd sizes with the momentum in row 1 and in row 2 of an
[n_attr, n_sd] block (row 1 is then only 8-byte aligned).  Planted: mass 0, a negative mass, radii
on table knots, at 40 um, at the table top; momenta equal to the terminal momentum, zero and
negative; the four c, both `constant` settings, both laws, with and without the velocity column.
The recorded runs: the collisions on both of their routes and the displacement on both of its
routes, fed from the momentum, within the bounds of tests/relaxed_velocity_cases.py, integers equal.
The fused collision step against the chain route, to the bit, on every route of its dispatcher."""
import warnings

import numpy as np
import pytest

from pysdm_amd.collisions import CollisionRunner
from pysdm_amd.relaxed_velocity import ROUTES, RelaxedVelocityRunner
from tests import relaxed_velocity_cases as rc

pytestmark = pytest.mark.gpu

W, G = rc.WORKGROUP, rc.GRID_PASS
SMALL = [1, 63, 64, 65, W - 1, W, W + 1]
LARGE = [G - 1, G, G + 1]
COMBOS = [(law, constant, c, with_velocity) for law in ("GunnKinzer1949", "RogersYau")
          for constant in (False, True) for c in rc.C_VALUES for with_velocity in (True, False)]


@pytest.fixture(scope="module", name="checker")
def checker_engine():
    from tests.relaxed_velocity_checker import RelaxedVelocityCheckerEngine  # pylint: disable=import-outside-toplevel

    return RelaxedVelocityCheckerEngine.get()


def state_with_terminal_momenta(checker, n_sd, seed):
    mass, momentum = rc.planted_state(n_sd, seed=seed)
    if n_sd > 30:  # a few slots already at the terminal momentum of the table
        terminal = rc.terminal_momentum(checker, mass)
        momentum[23:27] = terminal[23:27]
    return mass, momentum


def agree(hip_engine, checker, mass, momentum, combo, row, what):
    law, constant, c, with_velocity = combo
    options = {"dt": 1.5, "c": c, "constant": constant, "law": law,
               "with_velocity": with_velocity, "row": row, "n_calls": 2}
    got = rc.call_step(hip_engine, mass, momentum, **options)
    want = rc.call_step(checker, mass, momentum, **options)
    what = f"{what}: {law}, constant {constant}, c {c:g}, velocity {with_velocity}, row {row}"
    np.testing.assert_array_equal(got["status"], [0, 0], err_msg=what)
    rc.assert_same_doubles(got["momentum"], want["momentum"], f"{what}: momentum")
    np.testing.assert_array_equal(rc.bits(got["mass"]), rc.bits(mass), err_msg=what)
    if with_velocity:
        rc.assert_same_doubles(got["velocity"], want["velocity"], f"{what}: velocity")
        assert np.isfinite(got["velocity"][mass != 0]).all(), what


@pytest.mark.parametrize("n_sd", SMALL)
def test_hip_equals_checker_at_small_sizes(hip_engine, checker, n_sd):
    mass, momentum = state_with_terminal_momenta(checker, n_sd, seed=n_sd)
    for combo in COMBOS:
        agree(hip_engine, checker, mass, momentum, combo, None, f"n_sd {n_sd}")


@pytest.mark.parametrize("n_sd", LARGE)
def test_hip_equals_checker_around_one_grid_pass(hip_engine, checker, n_sd):
    """two of the 32 combinations per size: between them both laws, both `constant` settings, with
    and without the velocity column (all 32 run at the small sizes)"""
    mass, momentum = state_with_terminal_momenta(checker, n_sd, seed=n_sd % 1000)
    at = LARGE.index(n_sd)
    picks = (COMBOS[2 * at + 2], COMBOS[16 + 8 + 2 * at + 1])
    assert {p[1] for p in picks} == {True, False}
    assert {p[0] for p in picks} == {"GunnKinzer1949", "RogersYau"}
    assert {p[3] for p in picks} == {True, False}
    for combo in picks:
        agree(hip_engine, checker, mass, momentum, combo, None, f"n_sd {n_sd}")


@pytest.mark.parametrize("row", [1, 2])
@pytest.mark.parametrize("n_sd", [65, 1001, W + 1])
def test_hip_equals_checker_with_the_momentum_in_a_row_of_an_odd_block(hip_engine, checker, n_sd,
                                                                       row):
    mass, momentum = state_with_terminal_momenta(checker, n_sd, seed=n_sd + row)
    for combo in COMBOS[::5]:
        agree(hip_engine, checker, mass, momentum, combo, row, f"n_sd {n_sd}")


@pytest.mark.parametrize("mass_row, row, velocity_offset", [(1, 0, 0), (1, 2, 0), (0, 1, 1),
                                                            (1, 2, 1), (0, 2, 1)])
@pytest.mark.parametrize("n_sd", [65, W + 1])
def test_hip_equals_checker_with_every_column_only_8_byte_aligned(hip_engine, checker, n_sd,
                                                                  mass_row, row,
                                                                  velocity_offset):
    """the three alignment flags of k_rv_step one by one and together: the mass in row 1 of an odd
    block, the momentum in row 1, the velocity column one double into its allocation"""
    mass, momentum = state_with_terminal_momenta(checker, n_sd, seed=n_sd + 7 * row)
    for law, constant, c, _ in COMBOS[::7]:
        options = {"dt": 1.5, "c": c, "constant": constant, "law": law, "row": row,
                   "mass_row": mass_row, "velocity_offset": velocity_offset, "n_calls": 2}
        got = rc.call_step(hip_engine, mass, momentum, **options)
        want = rc.call_step(checker, mass, momentum, **options)
        what = f"n_sd {n_sd}, mass row {mass_row}, momentum row {row}, +{velocity_offset}"
        rc.assert_same_doubles(got["momentum"], want["momentum"], f"{what}: momentum")
        rc.assert_same_doubles(got["velocity"], want["velocity"], f"{what}: velocity")
        np.testing.assert_array_equal(rc.bits(got["mass"]), rc.bits(mass), err_msg=what)


def test_hip_refuses_a_radius_above_the_table_top_with_nothing_stored(hip_engine, checker):
    at_top, above = rc.mass_at_table_top(checker)
    for n_sd, slots in ((1, [0]), (W + 1, [W]), (3 * W + 5, [0, W - 1, 3 * W + 4])):
        mass, momentum = rc.planted_state(n_sd, seed=n_sd)
        mass[slots] = at_top
        agree(hip_engine, checker, mass, momentum, COMBOS[0], None, f"top, n_sd {n_sd}")
        mass[slots] = above
        mass[slots[0]] = -above  # (the sign does not matter)
        got = rc.call_step(hip_engine, mass, momentum)
        want = rc.call_step(checker, mass, momentum)
        np.testing.assert_array_equal(got["status"], [len(slots), 0])
        np.testing.assert_array_equal(want["status"], [len(slots), 0])
        np.testing.assert_array_equal(rc.bits(got["momentum"]), rc.bits(momentum))
        np.testing.assert_array_equal(got["velocity"], np.full(n_sd, -7.0))
        got = rc.call_step(hip_engine, mass, momentum, law="RogersYau")  # no top there
        want = rc.call_step(checker, mass, momentum, law="RogersYau")
        np.testing.assert_array_equal(got["status"], [0, 0])
        rc.assert_same_doubles(got["momentum"], want["momentum"], "Rogers-Yau above the top")


@pytest.mark.parametrize("law", ["GunnKinzer1949", "RogersYau"])
def test_hip_runner_routes_agree_and_the_fused_one_fills_the_cache(hip_engine, checker, law):
    momentum_population = rc.momentum_population

    mass, momentum = rc.planted_state(2 * W + 3, seed=8)
    results = {}
    for route in ROUTES:
        population = momentum_population(hip_engine, mass, momentum)
        RelaxedVelocityRunner(population, c=8, dt=1.0, terminal_velocity=law, route=route).run(2)
        results[route] = (hip_engine.download(population.momentum),
                          hip_engine.download(population.fall_velocity(None)))
    want = rc.call_step(checker, mass, momentum, law=law, n_calls=2)
    for route, (got_momentum, got_velocity) in results.items():
        rc.assert_same_doubles(got_momentum, want["momentum"], f"{route}: momentum")
        rc.assert_same_doubles(got_velocity, want["velocity"], f"{route}: velocity")
    _, above = rc.mass_at_table_top(checker)
    mass[5] = above
    population = momentum_population(hip_engine, mass, momentum)
    runner = RelaxedVelocityRunner(population, dt=1.0, terminal_velocity=law)
    if law == "GunnKinzer1949":
        with pytest.raises(ValueError, match="Radii can be interpolated up to"):
            runner.step()
        np.testing.assert_array_equal(rc.bits(hip_engine.download(population.momentum)),
                                      rc.bits(momentum))
    else:
        runner.step()


# ---- the recorded runs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("relax_route", ROUTES)
@pytest.mark.parametrize("name", ["relax_box_coal", "relax_box_breakup", "relax_4x4"])
def test_hip_chain_route_fed_from_the_momentum_reproduces_the_recorded_run(hip_engine, name,
                                                                           relax_route):
    data = rc.gold(name)
    for step, snap in rc.run_collisions(hip_engine, name, collision_route="chain",
                                        relax_route=relax_route):
        rc.assert_collision_step(snap, data, step, f"{name} ({relax_route})")
    assert step == int(data["steps"])


@pytest.mark.parametrize("route", ["fused", "chain"])
def test_hip_displacement_sediments_with_the_relaxed_velocity(hip_engine, route):
    rc.run_displacement(hip_engine, route=route, relax_route="fused")


# ---- the fused collision step reads the velocity from the momentum -----------------------------------
@pytest.mark.parametrize("relax_route", ROUTES)
@pytest.mark.parametrize("name", ["relax_box_coal", "relax_box_breakup", "relax_4x4"])
def test_hip_fused_route_fed_from_the_momentum_reproduces_the_recorded_run(hip_engine, name,
                                                                           relax_route):
    assert hip_engine.fused_momentum_velocity is True
    data = rc.gold(name)
    for step, snap in rc.run_collisions(hip_engine, name, collision_route="fused",
                                        relax_route=relax_route):
        rc.assert_collision_step(snap, data, step, f"{name} fused ({relax_route})")
    assert step == int(data["steps"])


# The routes of the dispatcher in pysdm_amd/csrc/fused.hip (collision_step) a population with a
# momentum row - two extensive attributes, so never the one-attribute kernels k_cell_step2* - can
# take, and the sizes that select them:
#   one cell (n_cell == 1): the pair kernels; the mirror is wide (32-byte records with radius and
#       velocity) for the Geometric kernel and for Straub's breakup parts, narrow (16 bytes) for
#       Golovin with coalescence only, which reads no velocity at all (mirror_is_wide)
#   several cells, the largest of at most CELL_CAP = 6144 super-droplets: k_cell_step (per cell)
#   several cells, one of more than CELL_CAP: the generic pair kernels over all cells
# each adaptive and not, with coalescence only and with breakup.
CELL_CAP = 6144
ROUTE_CASES = {
    "one cell, wide mirror": (1, 1024),
    "one cell, narrow mirror": (1, 1024),
    "per cell": (16, 4096),
    "generic multi-cell": (2, 2 * CELL_CAP + 2048),
}


def route_state(n_cell, n_sd, seed):
    rng = np.random.default_rng(seed)
    mass = rc.mass_of_radius(np.exp(rng.uniform(np.log(10e-6), np.log(1e-3), n_sd)))
    multiplicity = 1 + rng.integers(0, 3, n_sd)
    cell_id = rng.integers(0, n_cell, n_sd).astype(np.int64)
    return mass, multiplicity.astype(np.int64), cell_id


@pytest.mark.parametrize("breakup", [False, True], ids=["coalescence", "breakup"])
@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("case", list(ROUTE_CASES))
def test_hip_fused_equals_chain_on_every_route(hip_engine, case, adaptive, breakup):
    """three steps with a relaxation ahead of each: everything equal, doubles as bits"""
    from pysdm_amd import recipe as R  # pylint: disable=import-outside-toplevel
    from pysdm_amd.population import MOMENTUM_ROW, Population  # pylint: disable=import-outside-toplevel
    from pysdm_amd.relaxed_velocity import init_fall_momenta  # pylint: disable=import-outside-toplevel

    n_cell, n_sd = ROUTE_CASES[case]
    mass, multiplicity, cell_id = route_state(n_cell, n_sd, seed=len(case))
    if case == "generic multi-cell":  # one cell above the per-cell kernel's capacity
        cell_id[:CELL_CAP + 1024] = 0
        assert np.bincount(cell_id).max() > CELL_CAP
    elif n_cell > 1:
        assert np.bincount(cell_id).max() <= CELL_CAP
    kernel = R.Golovin(b=1.5e3) if "narrow" in case else R.Geometric()
    if breakup:
        ec = R.ConstEc(Ec=0.5) if "narrow" in case else R.Straub2010Ec()
        setup = R.CollisionSetup.collision(kernel, ec, R.ConstEb(1.0), R.AlwaysN(n=4), seed=44,
                                           adaptive=adaptive, warn_overflows=False)
    else:
        setup = R.CollisionSetup.coalescence(kernel, seed=44, adaptive=adaptive)
    momentum = 0.5 * init_fall_momenta(hip_engine, mass)
    dv = 1e-3 * n_sd / n_cell / 64
    snaps = {}
    for route in ("fused", "chain"):
        population = Population(
            hip_engine, multiplicity=multiplicity, mass=mass, cell_id=cell_id, n_cell=n_cell,
            more_extensive={MOMENTUM_ROW: momentum}, velocity_source="momentum")
        relax = RelaxedVelocityRunner(population, c=1000, dt=1.0)
        collisions = CollisionRunner(population, setup, dt=1.0, dv=dv, route=route,
                                     velocity="momentum")
        for _ in range(3):
            relax.step()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                collisions.run(1)
        population.refresh_bookkeeping()
        population.compact()
        snaps[route] = collisions.snapshot()
    fused, chain = snaps["fused"], snaps["chain"]
    length = int(fused["length"])
    assert length == int(chain["length"])
    assert fused["collision_rate"].sum() > 0, "nothing collided: the case shows nothing"
    for key, value in fused.items():
        want = chain[key]
        if key == "idx":
            value, want = value[:length], want[:length]
        if value.dtype == np.float64:
            rc.assert_same_doubles(value, want, f"{case}: {key}")
        else:
            np.testing.assert_array_equal(value, want, err_msg=f"{case}: {key}")


def test_hip_sharded_runs_refuse_the_momentum_source(hip_engine):
    from pysdm_amd import sharding  # pylint: disable=import-outside-toplevel

    data = rc.gold("relax_4x4")
    population = rc.population_from(hip_engine, data, grid=(4, 4), cell_id=data["init/cell_id"])
    runner = CollisionRunner(population, rc.collision_setup(data), dt=1.0, dv=1.0, route="fused",
                             velocity="momentum")
    with pytest.raises(NotImplementedError, match="[Ss]harded"):
        sharding._sharded(runner)  # pylint: disable=protected-access


def test_hip_under_the_pysdm_front_end_reproduces_the_recorded_run(hip_backend_class):
    """(where PySDM can be imported: skipped otherwise) `fuse(RelaxedVelocity)` beside
    `fuse(Coalescence)` and beside PySDM's own Coalescence on the plugged backend"""
    ref = rc.import_reference()
    data = rc.gold("relax_box_coal")
    for fuse_collisions in (True, False):
        for step, snap in rc.run_pysdm_box(ref, hip_backend_class, data, fuse_relaxation=True,
                                           fuse_collisions=fuse_collisions):
            rc.assert_collision_step(snap, data, step,
                                     f"PySDM front-end on HIP (fuse: {fuse_collisions})")

"""Inputs shared by the fall-velocity-law tests (test_velocity_laws.py, test_hip_velocity_laws.py).
The script that records their goldens (tests/golden/gen_velocity_law_golden.py) imports nothing of
this package and restates `planted`; the goldens' init/volume is compared with this one.

The planted input puts radii one to eight ulps on either side of, and exactly on, both limits of the
Rogers-Yau law (35 um and 600 um), so that a law evaluated with the wrong comparison, or from a
radius derived otherwise than the stage route derives it, changes a collision probability.
"""
import os

import numpy as np

from pysdm_amd import recipe as R
from pysdm_amd.collisions import CollisionRunner
from pysdm_amd.physics import constants as const
from pysdm_amd.population import Population
from pysdm_amd.terminal_velocity import PowerSeries

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLANT_SEED = 20261019
LIMITS = (const.ROGERS_YAU_TERM_VEL_SMALL_R_LIMIT, const.ROGERS_YAU_TERM_VEL_MEDIUM_R_LIMIT)
PLANT_DT, PLANT_DV = 1.0, 0.1
TWO_TERMS = {"prefactors": [0.3, 1.1], "powers": [1 / 6, 1 / 3]}
GOLDENS = {
    # name: (law, breakup)
    "traj_velocity_rogers_yau": ("RogersYau", False),
    "traj_velocity_power_series": ("PowerSeries", False),
    "traj_velocity_4x4_rogers_yau": ("RogersYau", False),
    "traj_velocity_breakup_rogers_yau": ("RogersYau", True),
}


def planted(n_sd=1024):
    """(volume, multiplicity) of the planted input"""
    rng = np.random.default_rng(PLANT_SEED)
    radius = np.exp(rng.uniform(np.log(5e-6), np.log(2e-3), n_sd))
    ulps = np.arange(-8, 9)
    for at, limit in enumerate(LIMITS):
        radius[at * len(ulps):(at + 1) * len(ulps)] = limit * (1 + ulps * 2.0 ** -52)
    multiplicity = 1 + rng.integers(0, 3, n_sd)
    return const.PI_4_3 * np.power(radius, 3), multiplicity.astype(np.int64)


def device_radius(volume, rho_w=const.rho_w):
    """the radius as the library derives it from the mass column, operation by operation
    (physics.h: volume_of_mass, radius_of_volume; `**` here is within an ulp of sdm_pow, which is
    all the census of the regimes needs)"""
    mass = volume * rho_w
    return np.power(mass / rho_w * (1 / const.PI_4_3), 1 / 3)


def laws():
    """the laws under test on the GPU, by a label: fresh objects (a law may hold device arrays)"""
    return {"rogers_yau": "RogersYau", "power_series": "PowerSeries",
            "two_terms": PowerSeries(**TWO_TERMS)}


def law_of(label):
    return laws()[label]


def box_runner(engine, law, *, route, adaptive, volume=None, multiplicity=None, cell_id=None,
               grid=None, dt=PLANT_DT, dv=PLANT_DV, setup=None, more_extensive=None, **options):
    """a CollisionRunner over the planted input (or the given one) with Geometric coalescence"""
    if volume is None:
        volume, multiplicity = planted()
    setup = setup or R.CollisionSetup.coalescence(R.Geometric(collection_efficiency=1),
                                                  adaptive=adaptive, seed=44, **options)
    population = Population(engine, multiplicity=multiplicity, volume=volume, cell_id=cell_id,
                            grid=grid, more_extensive=more_extensive)
    return CollisionRunner(population, setup, dt=dt, dv=dv, route=route, terminal_velocity=law)


def golden_runner(name, engine, route):
    """(runner, golden, recorded steps) of one of GOLDENS"""
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    law, breakup = GOLDENS[name]
    n_sd, seed, adaptive, dt, dv = gold["cfg"][:5]
    cell_id = gold["init/cell_id"] if "init/cell_id" in gold.files else None
    grid = tuple(int(g) for g in gold["grid"]) if "grid" in gold.files else None
    if breakup:
        setup = R.CollisionSetup.collision(R.Geometric(), R.Straub2010Ec(), R.ConstEb(1.0),
                                           R.AlwaysN(n=4), seed=int(seed), adaptive=bool(adaptive),
                                           warn_overflows=False)
    else:
        setup = R.CollisionSetup.coalescence(R.Geometric(collection_efficiency=1),
                                             seed=int(seed), adaptive=bool(adaptive))
    assert int(n_sd) == len(gold["init/volume"])
    runner = box_runner(engine, law, route=route, adaptive=bool(adaptive),
                        volume=gold["init/volume"], multiplicity=gold["init/multiplicity"],
                        cell_id=cell_id, grid=grid, dt=float(dt), dv=float(dv), setup=setup)
    steps = sorted({int(k.split("/")[0][4:]) for k in gold.files if k.startswith("step")})
    return runner, gold, steps


def rogers_yau_regimes(radius):
    """rows per regime of the law: (below 35 um, 35 .. 600 um, from 600 um)"""
    small, medium = LIMITS
    return (int((radius < small).sum()), int(((radius >= small) & (radius < medium)).sum()),
            int((radius >= medium).sum()))


"""Shared by the tests of the parcel with coalescence (tests/test_parcel_coal_checker.py,
tests/test_hip_parcel_coal.py): seeded ensembles of tests/parcel_cases.py with cloud-sized
droplets and planted multiplicities of 1 and 2 (so that equal-multiplicity pairs collide and
super-droplets die), collision set-ups whose constants make that happen within a few steps,
runners on both routes, and the comparison of two runs bit for bit."""
import numpy as np

from pysdm_amd import recipe
from pysdm_amd.condensation import CondensationSetup
from pysdm_amd.parcel import ParcelRunner
from tests import condensation_formulae_cases as fc
from tests import parcel_cases as pc

MAX_ROWS = 2048  # SDM_PARCEL_COAL_MAX_ROWS
GRID_CAP = 1024  # SDM_PARCEL_COAL_MAX_GRID
# parcels of no pair, one pair, an odd tail, the wave edges, more rows than one pass of a lane
SIZES = (1, 2, 3, 63, 64, 65, 257, 600)
COUNTERS = ("collision_rate", "collision_rate_deficit", "coalescence_rate")
PROFILE_KEYS = ("n_live", "n_substeps", "coalescence_rate", "collision_rate_deficit", "dv")
# formulae of the general condensation kernel (Constant surface tension, no ventilation)
GENERAL_OPTIONS = {"diffusion_kinetics": "LoweEtAl2019", "diffusion_thermics": "LoweEtAl2019",
                   "latent_heat_vapourisation": "Lowe2019",
                   "saturation_vapour_pressure": "AugustRocheMagnus"}

# the kernels' constants: a pair of multiplicities (1, 1) in a parcel of ~100 rows of 5 - 20
# micrometres in ~1 m3 collides with a probability of the order of 0.1 - 1 per second, so that
# within 4 - 6 steps of 1 s rows die in every parcel of more than a few rows, while the rows of
# large multiplicity collide every step (and fill collision_rate_deficit)
KERNELS = {
    "constant": lambda: recipe.ConstantK(a=4e-3),
    "golovin": lambda: recipe.Golovin(b=2e11),
    "geometric": lambda: recipe.Geometric(collection_efficiency=2e8),
    "electric": recipe.Electric,
}


def formulae_of(kind):
    """"default": PySDM's defaults (k_parcel_p); "general": GENERAL_OPTIONS (k_parcel_f_p)"""
    return fc.formulae_for(GENERAL_OPTIONS) if kind == "general" else pc.formulae_of(kind)


def setup_of(kernel="constant", adaptive=True, substeps=1, **options):
    """a CollisionSetup of coalescence; adaptive sub-steps between 0.05 s and the time step"""
    if not adaptive:
        options.update(adaptive=False, substeps=substeps)
    options.setdefault("dt_range", (0.05, 100.0))
    return recipe.CollisionSetup.coalescence(KERNELS[kernel](), **options)


def ensemble(sizes=SIZES, seed=7, multiplicity=1000):
    """pc.ensemble with droplets of 5 - 20 micrometres; every third row has multiplicity 1, every
    third 2, the others a seeded `multiplicity` .. 2 `multiplicity`"""
    kwargs = pc.ensemble(sizes, seed=seed)
    rng = np.random.default_rng(seed + 2000)
    n_sd = kwargs["water_mass"].size
    radius = rng.uniform(5e-6, 20e-6, n_sd)
    kwargs["water_mass"] = 1000.0 * 4 / 3 * np.pi * radius ** 3
    planted = np.arange(n_sd) % 3
    large = (multiplicity * rng.uniform(1.0, 2.0, n_sd)).astype(np.int64)
    kwargs["multiplicity"] = np.where(planted == 0, 1, np.where(planted == 1, 2, large))
    kwargs["w"] = np.abs(kwargs["w"])  # ascents: the droplets stay droplets
    return kwargs


def runner(engine, kind, kwargs, route, collisions=None, seed=None, **more):
    """a ParcelRunner of a seeded ensemble with coalescence as the third dynamic"""
    formulae = formulae_of(kind)
    setup = more.pop("setup", None) or CondensationSetup()
    return ParcelRunner(engine, formulae, setup, route=route,
                        collisions=collisions or setup_of(), seed=seed,
                        **pc.saturated(kwargs, formulae), **more)


def run(engine, kind, kwargs, route, steps, **more):
    """(snapshot, parcel profile, coalescence profile) of `steps` steps"""
    instance = runner(engine, kind, kwargs, route, **more)
    out = instance.run(steps)
    return (instance.snapshot(), *out)


def assert_same_run(a, b, what):
    """two results of `run`, bit for bit: state and every column, idx up to n_live, n_live, the
    counters, the stream positions, both profiles"""
    assert len(a) == len(b) == 3, what
    for part, x, y in zip(("state", "profile", "coalescence profile"), a, b):
        pc.assert_same_bits(x, y, f"{what}: {part}")


def concatenated(parts):
    """the profiles of consecutive runs as one"""
    return {key: np.concatenate([part[key] for part in parts], axis=0) for key in parts[0]}


def solo(kwargs, formulae, starts, c):
    """the keyword arguments of parcel `c` of an ensemble alone"""
    rows = slice(int(starts[c]), int(starts[c + 1]))
    return {key: (value if key == "dt" else value[rows] if key in (
        "multiplicity", "water_mass", "dry_volume", "kappa", "f_org") and value is not None
                  else None if value is None else np.asarray(value)[c:c + 1])
            for key, value in pc.saturated(kwargs, formulae).items()}


def conserved(runner_, rows=None):
    """(sum of n vdry, sum of n ktdv, sum of n) over the live rows of every parcel, per parcel,
    each sum formed with math.fsum"""
    import math  # pylint: disable=import-outside-toplevel

    state = runner_.snapshot()
    starts = runner_.parcel_start_host
    out = []
    for c in range(runner_.n_parcel):
        live = state["idx"][starts[c]:starts[c] + state["n_live"][c]]
        n = state["multiplicity"][live].astype(float)
        out.append((math.fsum(n * state["dry_volume"][live]),
                    math.fsum(n * state["kappa_times_dry_volume"][live]),
                    int(state["multiplicity"][live].sum())))
    return out

"""Shared by the tests of the parcel with collisional breakup (tests/test_parcel_breakup_checker.py,
tests/test_hip_parcel_breakup.py): the ensembles of tests/parcel_coal_cases.py with parcels of 2,
3, 256, 257 and 2048 rows added, collision set-ups with breakup whose constants make coalescences,
breakups and bounces happen within a few steps, runners on both routes with `breakup=True`, and the
comparison of two runs bit for bit."""
import math

from pysdm_amd import recipe
from tests import parcel_coal_cases as cc

# cc.SIZES (1, 2, 3, 63, 64, 65, 257, 600) holds a single pair (2), an odd tail (3) and one lane
# with two positions (257); 256: one position per lane
SIZES = cc.SIZES + (256,)
# the cap: four pairs per lane, and a colliding-pair list that can hold every pair
CAP_SIZES = (cc.MAX_ROWS, 5)
COUNTERS = cc.COUNTERS + ("breakup_rate", "breakup_rate_deficit")
PROFILE_KEYS = cc.PROFILE_KEYS + ("breakup_rate", "breakup_rate_deficit", "n_overflow")
UM3 = 1e-18  # m3

# every fragmentation function once; fragment volumes of the order of the droplets' (5 - 20 um:
# 500 - 33 000 um3), so that a breakup multiplies a multiplicity by a few
FRAGMENTATIONS = {
    "always_n": lambda: recipe.AlwaysN(3),
    "constant_mass": lambda: recipe.ConstantMass(1e-12),
    "exponential": lambda: recipe.Exponential(scale=2000 * UM3),
    "gaussian": lambda: recipe.Gaussian(mu=2000 * UM3, sigma=500 * UM3),
    "feingold1988": lambda: recipe.Feingold1988(scale=2000 * UM3),
    "slams": recipe.SLAMS,
    "straub2010": recipe.Straub2010Nf,
    # (made for millimetre drops: the limiters keep its fragments of cloud droplets droplets)
    "lowlist1982": lambda: recipe.LowList1982Nf(vmin=500 * UM3, nfmax=10),
}
EFFICIENCIES = {
    "const": lambda: recipe.ConstEc(0.4),
    "berry1967": recipe.Berry1967,
    "straub2010": recipe.Straub2010Ec,
    "lowlist1982": recipe.LowList1982Ec,
}
# Straub and Low-List form the pair's kinetic energy: the Geometric kernel, so that derive_ru runs
NEEDS_VELOCITY = ("straub2010", "lowlist1982")


# the kernels' constants: weaker than cc.KERNELS', since every breakup multiplies a multiplicity
# and with it the pair's probability - within 3 - 5 steps of 1 s the planted rows of multiplicity
# 1 and 2 still collide, and the counters stay far from the range of int64
KERNELS = {
    "constant": lambda: recipe.ConstantK(a=KERNEL_CONSTANTS["constant"]),
    "geometric": lambda: recipe.Geometric(collection_efficiency=KERNEL_CONSTANTS["geometric"]),
}
KERNEL_CONSTANTS = {"constant": 4e-4, "geometric": 2e7}
# ... and at most four adaptive sub-steps per step of 1 s bound the growth of a run of a few steps
DT_RANGE = (0.25, 100.0)


def kernel_of(name):
    return KERNELS["geometric" if name in NEEDS_VELOCITY else "constant"]()


def collision_setup(frag="always_n", ec="const", eb=0.5, adaptive=True, substeps=1, kernel=None,
                    **options):
    """CollisionSetup.collision: coalescence, breakup or bounce per colliding pair"""
    if not adaptive:
        options.update(adaptive=False, substeps=substeps)
    options.setdefault("dt_range", DT_RANGE)
    needs = frag if frag in NEEDS_VELOCITY else ec
    return recipe.CollisionSetup.collision(
        kernel or kernel_of(needs), EFFICIENCIES[ec](), recipe.ConstEb(eb), FRAGMENTATIONS[frag](),
        **options)


def breakup_setup(frag="always_n", adaptive=True, substeps=1, kernel=None, **options):
    """CollisionSetup.breakup_only: every collision breaks up"""
    if not adaptive:
        options.update(adaptive=False, substeps=substeps)
    options.setdefault("dt_range", DT_RANGE)
    return recipe.CollisionSetup.breakup_only(kernel or kernel_of(frag), FRAGMENTATIONS[frag](),
                                              **options)


def ensemble(sizes=SIZES, seed=7, multiplicity=1000):
    return cc.ensemble(sizes, seed=seed, multiplicity=multiplicity)


def runner(engine, kwargs, route, collisions, seed=None, kind="default", breakup=True, **more):
    return cc.runner(engine, kind, kwargs, route, collisions=collisions, seed=seed,
                     breakup=breakup, **more)


def run(engine, kwargs, route, steps, collisions, **more):
    """(snapshot, parcel profile, collision profile) of `steps` steps"""
    instance = runner(engine, kwargs, route, collisions, **more)
    out = instance.run(steps)
    return (instance.snapshot(), *out)


def assert_same_run(a, b, what):
    cc.assert_same_run(a, b, what)
    assert set(PROFILE_KEYS) <= set(a[2]), what


def bounces(state):
    """collisions counted in neither rate (nor in a deficit of breakups): the pairs that bounced"""
    return (state["collision_rate"] - state["coalescence_rate"] - state["breakup_rate"]
            - state["breakup_rate_deficit"])


def extensive_sums(runner_):
    """per parcel, the sums of multiplicity x {water mass, dry volume, kappa times dry volume}
    over the live rows (math.fsum) and the number of live rows"""
    state = runner_.snapshot()
    starts = runner_.parcel_start_host
    out = []
    for c in range(runner_.n_parcel):
        live = state["idx"][starts[c]:starts[c] + state["n_live"][c]]
        n = state["multiplicity"][live].astype(float)
        out.append(tuple(math.fsum(n * state[key][live]) for key in
                         ("water_mass", "dry_volume", "kappa_times_dry_volume"))
                   + (int(state["n_live"][c]),))
    return out


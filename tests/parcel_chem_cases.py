"""Shared by the tests of the parcel with aqueous chemistry (tests/test_parcel_chem_checker.py,
tests/test_hip_parcel_chem.py): the chemistry arguments of a seeded ensemble of
tests/parcel_cases.py, runners on both routes, and the comparison of two runs bit for bit."""
import numpy as np

from pysdm_amd.chemistry import GASES, ChemistrySetup
from pysdm_amd.condensation import CondensationSetup
from pysdm_amd.parcel import ParcelRunner
from tests import condensation_formulae_cases as fc
from tests import parcel_cases as pc

# ammonium bisulphate, as the reference's Kreidenweis et al. 2003 example takes it
DRY_RHO = 1800.0
DRY_MOLAR_MASS = 0.11511
# the trace gases of that example
MOLE_FRACTIONS = {"SO2": 0.2e-9, "O3": 50e-9, "H2O2": 0.5e-9, "CO2": 360e-6, "HNO3": 0.1e-9,
                  "NH3": 0.1e-9}
ZERO_FRACTIONS = {gas: 0.0 for gas in GASES}
PROFILE_KEYS = ("mixing_ratio", "aq_total", "n_flagged", "dv")


# formulae of the general condensation kernel with the Constant surface tension chemistry needs
GENERAL_OPTIONS = {"diffusion_kinetics": "LoweEtAl2019", "diffusion_thermics": "LoweEtAl2019",
                   "latent_heat_vapourisation": "Lowe2019",
                   "saturation_vapour_pressure": "AugustRocheMagnus"}


def formulae_of(kind):
    """"default": PySDM's defaults (k_parcel); "general": GENERAL_OPTIONS (k_parcel_f)"""
    return fc.formulae_for(GENERAL_OPTIONS) if kind == "general" else pc.formulae_of(kind)


def setup_of(system="closed", sum_mode="ordered", n_substep=1):
    return ChemistrySetup(system, n_substep, sum=sum_mode)


def runner(engine, kind, kwargs, route, *, system="closed", sum_mode="ordered", n_substep=1,
           mole_fractions=None, **more):
    """a ParcelRunner of a seeded ensemble with the third dynamic"""
    formulae = formulae_of(kind)
    setup = more.pop("setup", None) or CondensationSetup()
    return ParcelRunner(engine, formulae, setup, route=route,
                        chemistry=setup_of(system, sum_mode, n_substep),
                        mole_fractions=MOLE_FRACTIONS if mole_fractions is None else mole_fractions,
                        dry_rho=DRY_RHO, dry_molar_mass=DRY_MOLAR_MASS,
                        **pc.saturated(kwargs, formulae), **more)


def run(engine, kind, kwargs, route, steps, products=(), **more):
    """(snapshot, parcel profile, chemistry profile[, products]) of `steps` steps"""
    instance = runner(engine, kind, kwargs, route, **more)
    out = instance.run(steps, products=products)
    return (instance.snapshot(), *out)


def assert_same_run(a, b, what):
    """two results of `run`, bit for bit"""
    assert len(a) == len(b), what
    for part, x, y in zip(("state", "profile", "chemistry profile", "products"), a, b):
        pc.assert_same_bits(x, y, f"{what}: {part}")


def concatenated(parts):
    """the profiles of consecutive runs as one: rows along the step axis (the last but one of the
    chemistry profile's stacked members)"""
    out = {}
    for key in parts[0]:
        axis = 1 if key in ("mixing_ratio", "aq_total") else 0
        out[key] = np.concatenate([part[key] for part in parts], axis=axis)
    return out


def ensemble(sizes, seed=7):
    """pc.ensemble with a seeded half of the rows grown to 12 .. 30 dry radii: dilute enough for
    the ionic-strength threshold, so that their do_chemistry_flag is set and the gases dissolve
    and react in them, while the haze rows stay unflagged"""
    kwargs = pc.ensemble(sizes, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    n_sd = kwargs["water_mass"].size
    grown = rng.uniform(0.0, 1.0, n_sd) < 0.5
    ratio = rng.uniform(12.0, 30.0, n_sd)
    dry_mass = 1000.0 * kwargs["dry_volume"]
    kwargs["water_mass"] = np.where(grown, dry_mass * ratio ** 3, kwargs["water_mass"])
    return kwargs


# (index into pc.FAILURE_CASES, seed of `ensemble`): with the grown rows of `ensemble` the solver
# gives up in some parcels and not in others at these seeds - at the first step (the case's own
# seed), and at steps 0 and 4 beside a parcel that goes on (after the chemistry has acted)
FAILURE_CASES = ((0, 5), (2, 9))
FAILURE_IDS = ("fixed-first-step", "adaptive-later-step")

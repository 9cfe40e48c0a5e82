"""Shared by the tests of the ventilated parcel (tests/test_parcel_vent_checker.py,
tests/test_hip_parcel_vent.py): the two ventilations, the three fall-velocity laws, seeded
ensembles of ascending haze and of descending drizzle, and the run of one runner as a pair
(snapshot, profile) for `parcel_cases.assert_same_bits`."""
import numpy as np

from pysdm_amd.condensation import CondensationSetup
from pysdm_amd.parcel import ParcelRunner
from tests import condensation_formulae_cases as fc
from tests import parcel_cases as pc

# rows per parcel: one row, a lane edge (COND_CB = 256) and past the register-cached rows
# (COND_CH = 1024)
SIZES = (1, 255, 256, 257, 1025)
VENTILATIONS = ("PruppacherAndRasmussen1979", "Froessling1938")  # (the second: by descriptor)
LAWS = ("GunnKinzer1949", "RogersYau", "PowerSeries")
VENT_KEYS = ("air_density", "air_dynamic_viscosity", "reynolds_number", "out_of_table")
RHO_W = 1000.0


def formulae_of(ventilation, kind="default"):
    """(formulae, explicit descriptor or None): `Formulae` refuses Froessling1938, which travels
    in a descriptor beside the formulae of the other choices - PySDM's defaults, or with `kind`
    "lowe2019" those of tests/parcel_cases.py's second kind"""
    options = dict(fc.GOLDENS["parcel_lowe2019"]) if kind == "lowe2019" else {}
    if ventilation != "Neglect":
        options["ventilation"] = ventilation
    return fc.formulae_for(options), fc.descriptor_for(options)


def ascending(sizes=SIZES, seed=7):
    """the haze ensemble of tests/parcel_cases.py with every updraft positive"""
    kwargs = pc.ensemble(sizes, seed=seed)
    kwargs["w"] = np.abs(kwargs["w"])
    return kwargs


def descending(sizes=SIZES, seed=9, radii=(50e-6, 500e-6)):
    """drizzle below cloud base: every parcel sinks through subsaturated air (RH 0.85 .. 0.95), its
    rows hold radii drawn log-uniformly from `radii` (Reynolds numbers of 1 .. 1000: the
    ventilation factor differs from 1), some 0.1 g of liquid water per kg of dry air"""
    kwargs = pc.ensemble(sizes, seed=seed)
    rng = np.random.default_rng(seed + 100)
    n_parcel, n_sd = len(sizes), int(np.sum(sizes))
    r_wet = np.exp(rng.uniform(np.log(radii[0]), np.log(radii[1]), n_sd))
    mass = RHO_W * 4 / 3 * np.pi * r_wet ** 3
    per_row_n = np.repeat(np.asarray(sizes), sizes)
    per_row_air = np.repeat(kwargs["mass_of_dry_air"], sizes)
    kwargs.update(
        w=-np.abs(kwargs["w"]), RH0=rng.uniform(0.85, 0.95, n_parcel), water_mass=mass,
        multiplicity=np.maximum(1, (1e-4 * per_row_air / per_row_n / mass
                                    * rng.uniform(0.5, 1.5, n_sd)).astype(np.int64)))
    return kwargs


def runner(engine, ventilation, law, kwargs, route, **more):
    formulae, descriptor = formulae_of(ventilation, more.pop("kind", "default"))
    setup = more.pop("setup", None) or CondensationSetup()
    if ventilation != "Neglect":
        more.update(terminal_velocity=law, descriptor=descriptor)
    return ParcelRunner(engine, formulae, setup, route=route, **pc.saturated(kwargs, formulae),
                        **more)


def run(engine, ventilation, law, kwargs, route, steps, **more):
    """(snapshot, profile) after `steps` steps"""
    one = runner(engine, ventilation, law, kwargs, route, **more)
    profile = one.run(steps)
    return one.snapshot(), profile


def liquid_water(snapshot, kwargs):
    """per parcel: sum of multiplicity * water mass"""
    starts = np.concatenate(([0], np.cumsum(kwargs["counts"])))
    terms = np.asarray(kwargs["multiplicity"], dtype=float) * snapshot["water_mass"]
    return np.array([terms[a:b].sum() for a, b in zip(starts[:-1], starts[1:])])

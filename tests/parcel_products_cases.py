"""Shared by the tests of the parcel's diagnostics (tests/test_parcel_products_checker.py,
tests/test_hip_parcel_products.py): a full request table (16 moment requests, 256 bins) for the
seeded ensembles of tests/parcel_cases.py, the eleven products, and the evaluated rows of a
runner as a dict for `parcel_cases.assert_same_bits`."""
import numpy as np

from pysdm_amd import products as pr
from pysdm_amd.products import MomentRequest, RequestTable, SpectrumRequest

# rows per parcel: lane, wave and register-chunk edges of the pass (256 lanes; the solver caches
# the first 1024 rows in registers) and rows past the cache
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 1024, 1025, 2049)

RHO_W = 1000.0
PI_4_3 = np.pi * 4 / 3


def mass_of_radius(radius):
    return RHO_W * PI_4_3 * radius ** 3


# the ensembles' wet radii lie in 3e-8 .. 1.6e-6 m, the dry radii in 2e-8 .. 4e-7 m: every cut
# below has rows on both sides.  All five attributes, all four filters, ranks 0, 1, 1/3, 2/3 and
# 2, the division by moment_0 on and off; request 15 selects nothing (an empty range).
SIXTEEN = (
    MomentRequest("water mass", 0, "water mass", 0.0, np.inf, False),
    MomentRequest("water mass", 1, "water mass", mass_of_radius(2e-7), np.inf, False),
    MomentRequest("water mass", 1, "water mass", 0.0, mass_of_radius(5e-7), True),
    MomentRequest("volume", 1 / 3, "water mass", 0.0, np.inf, False),
    MomentRequest("volume", 2 / 3, "volume", PI_4_3 * 1e-7 ** 3, PI_4_3 * 1e-6 ** 3, False),
    MomentRequest("volume", 1, "volume", PI_4_3 * 1e-7 ** 3, PI_4_3 * 1e-6 ** 3, True),
    MomentRequest("radius", 1, "volume", 0.0, np.inf, False),
    MomentRequest("radius", 2, "dry volume", PI_4_3 * 5e-8 ** 3, PI_4_3 * 2e-7 ** 3, False),
    MomentRequest("dry volume", 1, "dry volume", 0.0, PI_4_3 * 1e-7 ** 3, True),
    MomentRequest("dry radius", 1, "water mass", 0.0, np.inf, False),
    MomentRequest("dry radius", 2 / 3, "wet to critical volume ratio", 0.0, 1.0, False),
    MomentRequest("volume", 0, "wet to critical volume ratio", 1.0, np.inf, False),
    MomentRequest("volume", 1 / 3, "wet to critical volume ratio", 1.0, np.inf, False),
    MomentRequest("volume", 2 / 3, "wet to critical volume ratio", 0.0, np.inf, True),
    MomentRequest("radius", 1 / 3, "wet to critical volume ratio", 1e-3, 0.5, False),
    MomentRequest("water mass", 1, "water mass", mass_of_radius(3e-7), mass_of_radius(3e-7),
                  False),
)
SPECTRUM_256 = SpectrumRequest("volume", tuple(PI_4_3 * np.geomspace(5e-8, 1.2e-6, 257) ** 3))


def full_table(formulae):
    return RequestTable.from_requests(SIXTEEN, SPECTRUM_256, formulae)


def eleven(edges=None, activated=(False, True), dry=False):
    """the eleven products of pysdm_amd.products, the activation-filtered ones counting
    (unactivated, activated) = `activated`, the two spectra on `edges` (64 bins by default)"""
    if edges is None:
        edges = np.geomspace(2e-8, 2e-5, 65)
    un, act = activated
    return (
        pr.ParticleConcentration(), pr.ParticleSpecificConcentration(), pr.WaterMixingRatio(),
        pr.MeanRadius(), pr.EffectiveRadius(),
        pr.ActivatedParticleConcentration(count_unactivated=un, count_activated=act),
        pr.ActivatedParticleSpecificConcentration(count_unactivated=un, count_activated=act),
        pr.ActivatedMeanRadius(count_unactivated=un, count_activated=act),
        pr.ActivatedEffectiveRadius(count_unactivated=un, count_activated=act),
        pr.ParticleSizeSpectrumPerMassOfDryAir(radius_bins_edges=edges, dry=dry),
        pr.ParticleSizeSpectrumPerVolume(radius_bins_edges=edges, dry=dry),
    )


def raw(rows, dv=True):
    """the evaluated table of a runner (`last_rows`) as a dict of arrays"""
    out = {"moment_0": rows.moment_0_all, "moments": rows.moments_all,
           "spectrum": rows.spectrum}
    if dv:
        out["dv"] = rows.dv
    return out


def run_with_table(runner, table, splits):
    """`runner.run(n, products=table)` for every n of `splits`; (profile, raw rows) concatenated
    over the steps"""
    profiles, rows = [], []
    for n in splits:
        profile, _ = runner.run(n, products=table)
        profiles.append(profile)
        rows.append(raw(runner.last_rows))
    join = lambda parts: {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}  # noqa: E731
    return join(profiles), join(rows)


def diagnose_after_each_step(runner, table, n_steps):
    """`run(1)` without products, then `diagnose`, n_steps times: the rows the fused route must
    reproduce (moment_0, moments, spectrum), stacked over the steps"""
    rows = []
    for _ in range(n_steps):
        runner.run(1)
        runner.diagnose(table)
        rows.append(raw(runner.last_rows, dv=False))
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


# ---- the products recorded from the reference (tests/golden/gen_parcel_products_golden.py) ------
# (class name, keyword arguments): instantiated from PySDM.products by the generator and from
# pysdm_amd.products by the tests.  Radius ranges and bin edges are chosen so that no droplet of
# the recorded steps lies within a relative 1e-9 of a bound (the generator asserts it).
GOLDEN_WET_EDGES = tuple(np.geomspace(1.1e-8, 3.3e-5, 33))
GOLDEN_DRY_EDGES = tuple(np.geomspace(1.1e-9, 1.3e-6, 33))
_ACT = dict(count_unactivated=False, count_activated=True)
GOLDEN_PRODUCTS = (
    ("ParticleConcentration", dict(name="n")),
    ("ParticleSpecificConcentration", dict(name="n_specific")),
    ("WaterMixingRatio", dict(name="ql")),
    ("MeanRadius", dict(name="r_mean")),
    ("EffectiveRadius", dict(name="r_eff")),
    ("ActivatedParticleConcentration", dict(name="n_act", **_ACT)),
    ("ActivatedParticleSpecificConcentration", dict(name="n_act_specific", **_ACT)),
    ("ActivatedMeanRadius", dict(name="r_mean_act", **_ACT)),
    ("ActivatedEffectiveRadius", dict(name="r_eff_act", **_ACT)),
    ("ParticleSizeSpectrumPerMassOfDryAir", dict(name="spectrum_per_mass",
                                                 radius_bins_edges=GOLDEN_WET_EDGES)),
    ("ParticleSizeSpectrumPerVolume", dict(name="spectrum_per_volume",
                                           radius_bins_edges=GOLDEN_WET_EDGES)),
    # constructor arguments beyond the defaults: ranges, stp, units, the unactivated side, dry
    ("ParticleConcentration", dict(name="n_cloud_stp", radius_range=(0.53e-6, 25.7e-6),
                                   stp=True, unit="cm^-3")),
    ("WaterMixingRatio", dict(name="ql_cloud", radius_range=(0.53e-6, 25.7e-6), unit="g/kg")),
    ("MeanRadius", dict(name="r_mean_cloud", radius_range=(0.53e-6, 25.7e-6), unit="um")),
    ("EffectiveRadius", dict(name="r_eff_cloud", radius_range=(0.53e-6, 25.7e-6))),
    ("ActivatedParticleConcentration", dict(name="n_unact", count_unactivated=True,
                                            count_activated=False, unit="cm^-3")),
    ("ParticleSizeSpectrumPerVolume", dict(name="dry_spectrum_stp", dry=True, stp=True,
                                           radius_bins_edges=GOLDEN_DRY_EDGES)),
)
GOLDEN_EVERY = {"a": 4, "b": 6, "c": 2}  # every k-th step of the run is recorded


def golden_products(module):
    """the products of GOLDEN_PRODUCTS from `module` (PySDM.products or pysdm_amd.products)"""
    return tuple(getattr(module, cls)(**kwargs) for cls, kwargs in GOLDEN_PRODUCTS)

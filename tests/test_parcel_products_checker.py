"""The parcel's diagnostics (include/sdm_parcel_diag.h) without a GPU: the CPU checker
(tests/parcel_diag_checker/) against an independent restatement, the semantics at the edges of
ranges and bins, the product classes (pysdm_amd/products.py) against products recorded from the
reference, the fused rows against `diagnose` bit for bit, resumption, a failing parcel, the
refusals and the PySDM hook."""
import ctypes
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
from mpmath import mp

from pysdm_amd import abi
from pysdm_amd import products as pr
from pysdm_amd.condensation import critical_volume_call
from pysdm_amd.engine import FLOAT
from pysdm_amd.formulae import Formulae
from pysdm_amd.parcel import diagnose_call
from pysdm_amd.products import MomentRequest, RequestTable, Rows, SpectrumRequest
from tests import parcel_cases as pc
from tests import parcel_products_cases as ppc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = os.environ.get("PYSDM_REFERENCE", "/root/reference")
# the project's bar for moments against the reference (diagnostics.py, moments.npz)
MOMENT_RTOL = 1e-12
U = 2.0 ** -53  # the unit round-off of a double


@pytest.fixture(scope="module")
def engine():
    from tests.parcel_diag_checker import ParcelDiagCheckerEngine  # pylint: disable=import-outside-toplevel

    return ParcelDiagCheckerEngine.get()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "parcel_products.npz"))


def evaluate(engine, formulae, table, *, counts, water_mass, multiplicity, dry_volume, kappa,
             T, f_org=None, general=False):
    """`sdm_parcel_diagnose` on host columns: the raw rows (moment_0, moments, spectrum)"""
    counts = np.asarray(counts, dtype=np.int64)
    n_parcel, n_sd = counts.size, int(counts.sum())
    up = engine.upload
    diag = {name: engine.full(n_parcel * size, FLOAT, np.nan) for name, size in
            (("moment_0", table.n_moments), ("moments", table.n_moments),
             ("spectrum", table.n_bins)) if size > 0}
    diagnose_call(
        engine, formulae, table.c_struct(),
        parcel_start=up(np.concatenate(([0], np.cumsum(counts))).astype(np.int64)),
        water_mass=up(np.ascontiguousarray(water_mass, dtype=float)),
        multiplicity=up(np.ascontiguousarray(multiplicity, dtype=np.int64)),
        dry_volume=up(np.ascontiguousarray(dry_volume, dtype=float)),
        kappa=up(np.ascontiguousarray(np.broadcast_to(kappa, (n_sd,)), dtype=float)),
        f_org=up(np.zeros(n_sd) if f_org is None else np.ascontiguousarray(f_org, dtype=float)),
        T=up(np.ascontiguousarray(np.broadcast_to(T, (n_parcel,)), dtype=float)), diag=diag,
        general=general)
    out = {name: engine.download(array).reshape(n_parcel, -1) for name, array in diag.items()}
    for name in ("moment_0", "moments", "spectrum"):
        out.setdefault(name, np.empty((n_parcel, 0)))
    return out


# ---- 1. binding ------------------------------------------------------------------------------------
def test_header_parses_and_the_symbols_bind(engine):
    table = abi.parse_header(abi.PARCEL_DIAG_HEADER_PATH)
    assert sorted(table) == ["sdm_parcel_diagnose", "sdm_parcel_run_diag"]
    params = [p.name for p in table["sdm_parcel_run_diag"][1]]
    assert params[:-2] == [p.name for p in abi.parse_header(abi.PARCEL_HEADER_PATH)[
        "sdm_parcel_run"][1]] and params[-2:] == ["requests", "diag"]
    for library in (engine.parcel_diag_library, abi.parcel_diag_library()):
        assert hasattr(library.cdll, "sdm_parcel_run_diag")
        assert hasattr(library.cdll, "sdm_parcel_diagnose")


def test_struct_layouts_and_enums_match_the_header():
    structs = (("sdm_parcel_moment_request", abi.ParcelMomentRequest),
               ("sdm_parcel_requests", abi.ParcelRequests), ("sdm_parcel_diag", abi.ParcelDiag))
    prints = []
    for c_name, mirror in structs:
        prints.append(f'printf("%zu\\n", sizeof({c_name}));')
        prints += [f'printf("%zu\\n", offsetof({c_name}, {field}));'
                   for field, _ in mirror._fields_]  # pylint: disable=protected-access
    names = ["SDM_PARCEL_MAX_MOMENTS", "SDM_PARCEL_MAX_BINS"]
    names += ["SDM_PARCEL_ATTR_" + key.upper().replace(" ", "_") for key in abi.PARCEL_ATTRS]
    names += ["SDM_PARCEL_FILTER_WATER_MASS", "SDM_PARCEL_FILTER_VOLUME",
              "SDM_PARCEL_FILTER_DRY_VOLUME", "SDM_PARCEL_FILTER_VOLUME_RATIO"]
    prints += [f'printf("%d\\n", (int){name});' for name in names]
    source = ('#include "include/sdm_parcel_diag.h"\n#include <stddef.h>\n#include <stdio.h>\n'
              "int main(){" + "".join(prints) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w", encoding="utf-8") as handle:
            handle.write(source)
        subprocess.check_call(["gcc", "-I", ROOT, src, "-o", exe], cwd=ROOT)
        numbers = [int(x) for x in subprocess.check_output([exe]).split()]
    expected = []
    for _, mirror in structs:
        expected.append(ctypes.sizeof(mirror))
        expected += [getattr(mirror, field).offset for field, _ in mirror._fields_]  # pylint: disable=protected-access
    expected += [abi.PARCEL_MAX_MOMENTS, abi.PARCEL_MAX_BINS, *abi.PARCEL_ATTRS.values()]
    expected += [abi.PARCEL_FILTERS[key] for key in ("water mass", "volume", "dry volume",
                                                     "wet to critical volume ratio")]
    assert numbers == expected
    assert abi.PARCEL_FILTERS["signed water mass"] == abi.PARCEL_FILTERS["water mass"]


# ---- a. the checker against an independent restatement -------------------------------------------------
# The relative error of a computed moment against the exact value for the double inputs, in units
# of U = 2^-53, to first order (the factor SECOND_ORDER covers the products of the errors):
#   attribute   water mass, dry volume: 0 (inputs); volume = m / rho_w: 1;
#               radius = sdm_pow(volume * (1 / PI_4_3), 1 / 3): the argument carries 3 roundings
#               (volume, the reciprocal, the product), the power divides that by 3, and sdm_pow
#               adds its own error; dry radius likewise with 2 roundings in the argument
#   sdm_pow     0.7 ulp (tests/test_sdm_math.py MAX_ULP["pow"]), an ulp being at most 2 U relative
#   term        n * power(attr, rank): |rank| times the attribute's error, sdm_pow's unless the
#               rank is 0 or 1, and the product's rounding
#   sum         all terms are non-negative, so n terms in any order add at most (n - 1) U
#   division    by moment_0 (exact: integers below 2^53): 1
POW_ERROR = 0.7 * 2
ATTR_ERROR = {"water mass": 0.0, "dry volume": 0.0, "volume": 1.0, "radius": 3 / 3 + POW_ERROR,
              "dry radius": 2 / 3 + POW_ERROR}
SECOND_ORDER = 1.01


def moment_bound(request, n_rows):
    term = abs(request.rank) * ATTR_ERROR[request.attr] + 1
    if request.rank not in (0, 1):
        term += POW_ERROR
    return (term + (n_rows - 1) + (0 if request.skip else 1)) * U * SECOND_ORDER


def exact_rows(formulae, table, columns, v_cr):
    """the table for one parcel with 50-digit arithmetic on the same doubles (filters compare the
    attributes as the library derives them: a double each)"""
    const = formulae.constants
    mass, n = columns["water_mass"], columns["multiplicity"]
    volume = mass / const.rho_w
    filters = {"water mass": mass, "signed water mass": mass, "volume": volume,
               "dry volume": columns["dry_volume"], "wet to critical volume ratio": volume / v_cr}
    mp.dps = 50
    pi_4_3 = mp.mpf(float(const.PI_4_3))
    third = mp.mpf(1.0 / 3.0)  # the double the header's radius is defined with
    exact = {
        "water mass": [mp.mpf(float(m)) for m in mass],
        "volume": [mp.mpf(float(m)) / mp.mpf(float(const.rho_w)) for m in mass],
        "dry volume": [mp.mpf(float(v)) for v in columns["dry_volume"]]}
    exact["radius"] = [mp.power(v / pi_4_3, third) for v in exact["volume"]]
    exact["dry radius"] = [mp.power(v / pi_4_3, third) for v in exact["dry volume"]]
    moment_0, moments = [], []
    for request in table.index:
        f = filters[request.filter_attr]
        chosen = np.flatnonzero((request.min_x <= f) & (f < request.max_x))
        m0 = math.fsum(float(n[q]) for q in chosen)
        rank = mp.mpf(float(request.rank))
        total = mp.fsum(int(n[q]) * mp.power(exact[request.attr][q], rank) for q in chosen)
        moment_0.append(m0)
        moments.append(total if request.skip else (total / m0 if m0 else mp.mpf(0)))
    spectrum = None
    if table.spectrum is not None:
        f, edges = filters[table.spectrum.bin_attr], np.asarray(table.spectrum.edges)
        spectrum = [float(n[(edges[b] <= f) & (f < edges[b + 1])].sum())
                    for b in range(edges.size - 1)]
    return moment_0, moments, spectrum


@pytest.mark.parametrize("kind", ("default", "lowe2019"))
def test_checker_against_an_independent_restatement(engine, kind):
    """parcels of 1, 255, 257 and 700 rows, the full table: every moment within the bound derived
    above of the 50-digit value; every moment_0 and every count of the spectrum equal"""
    sizes = (1, 255, 257, 700)
    kwargs = pc.ensemble(sizes, seed=31, f_org=kind != "default")
    formulae = pc.formulae_of(kind)
    table = ppc.full_table(formulae)
    T = np.array([281.0, 285.5, 290.25, 294.0])
    got = evaluate(engine, formulae, table, counts=sizes, T=T,
                   **{k: kwargs[k] for k in ("water_mass", "multiplicity", "dry_volume", "kappa",
                                             "f_org")})
    starts = np.concatenate(([0], np.cumsum(sizes)))
    n_sd = int(starts[-1])
    v_cr, v_wet = engine.empty(n_sd, FLOAT), kwargs["water_mass"] / formulae.constants.rho_w
    critical_volume_call(engine, formulae, v_cr, engine.upload(kwargs["kappa"]),
                         engine.upload(np.zeros(n_sd) if kwargs["f_org"] is None
                                       else kwargs["f_org"]),
                         engine.upload(kwargs["dry_volume"]), engine.upload(v_wet),
                         engine.upload(T), engine.upload(np.repeat(np.arange(4), sizes)), n_sd)
    v_cr = engine.download(v_cr)
    worst = 0.0
    for c, size in enumerate(sizes):
        rows = slice(starts[c], starts[c + 1])
        columns = {k: np.asarray(kwargs[k])[rows] for k in ("water_mass", "multiplicity",
                                                            "dry_volume")}
        moment_0, moments, spectrum = exact_rows(formulae, table, columns, v_cr[rows])
        assert got["moment_0"][c].tolist() == moment_0
        assert got["spectrum"][c].tolist() == spectrum
        for i, request in enumerate(table.index):
            exact, value = moments[i], mp.mpf(float(got["moments"][c, i]))
            if exact == 0:
                assert value == 0, (c, i)
                continue
            error = float(abs(value - exact) / exact)
            worst = max(worst, error / moment_bound(request, size))
            assert error <= moment_bound(request, size), (c, i, request, error)
    print("worst error / bound:", worst)
    assert got["moment_0"][:, 15].tolist() == [0, 0, 0, 0]  # the empty selection


# ---- b. semantics at the edges ------------------------------------------------------------------------
def test_ranges_are_half_open_and_bins_too(engine):
    """rows with the filter attribute exactly on min_x, on max_x and one nextafter either side
    (8 rows each); rows on a bin edge, below the first and above the last edge; an empty
    selection; ranks 0, 1, 1/3 and 2/3; the division by moment_0 on and off"""
    formulae = Formulae()
    lo, hi = 3.0e-15, 7.0e-13
    edges = np.array([1.0e-15, 2.0e-14, 5.0e-13, 9.0e-12])
    labels = {
        "below_min": np.nextafter(lo, 0), "on_min": lo, "above_min": np.nextafter(lo, 1),
        "below_max": np.nextafter(hi, 0), "on_max": hi, "above_max": np.nextafter(hi, 1),
        "below_first_edge": np.nextafter(edges[0], 0), "on_first_edge": edges[0],
        "below_inner_edge": np.nextafter(edges[1], 0), "on_inner_edge": edges[1],
        "below_last_edge": np.nextafter(edges[3], 0), "on_last_edge": edges[3],
        "above_last_edge": np.nextafter(edges[3], 1)}
    rng = np.random.default_rng(5)
    mass = np.repeat(np.array(list(labels.values())), 8)
    order = rng.permutation(mass.size)
    mass = mass[order]
    label = np.repeat(np.array(list(labels)), 8)[order]
    n = rng.integers(1, 1000, mass.size)
    ranks = (0, 1, 1 / 3, 2 / 3)
    requests = tuple(MomentRequest("water mass", rank, "water mass", lo, hi, skip)
                     for rank in ranks for skip in (False, True))
    requests += (MomentRequest("water mass", 1, "water mass", hi, hi, False),
                 MomentRequest("water mass", 1, "water mass", 1.0, 2.0, True))
    table = RequestTable.from_requests(requests, SpectrumRequest("water mass", tuple(edges)),
                                       formulae)
    got = evaluate(engine, formulae, table, counts=[mass.size], water_mass=mass, multiplicity=n,
                   dry_volume=np.full(mass.size, 1e-22), kappa=0.5, T=290.0)
    inside = np.isin(label, ("on_min", "above_min", "below_inner_edge", "on_inner_edge",
                             "below_max"))
    assert np.array_equal(inside, (lo <= mass) & (mass < hi))
    m0 = float(n[inside].sum())
    for i, request in enumerate(requests[:8]):
        assert got["moment_0"][0, i] == m0
        total = math.fsum(float(k) * float(m) ** request.rank for k, m in
                          zip(n[inside], mass[inside]))
        expected = total if request.skip else total / m0
        bound = (abs(request.rank) * 0 + 1 + 2 * POW_ERROR + inside.sum()) * U * SECOND_ORDER
        assert got["moments"][0, i] == pytest.approx(expected, rel=bound, abs=0), request
        if request.rank == 0:
            assert got["moments"][0, i] == (m0 if request.skip else 1.0)
    # the empty selections: moment_0 == 0 gives moment == 0, divided or not
    assert got["moment_0"][0, 8:].tolist() == [0, 0] and got["moments"][0, 8:].tolist() == [0, 0]
    bins = [("on_first_edge", "below_inner_edge", "on_min", "above_min", "below_min"),
            ("on_inner_edge",),
            ("below_max", "on_max", "above_max", "below_last_edge")]
    for b, names in enumerate(bins):
        chosen = (edges[b] <= mass) & (mass < edges[b + 1])
        assert np.array_equal(chosen, np.isin(label, names)), b
        assert got["spectrum"][0, b] == float(n[chosen].sum())
    assert got["spectrum"][0].sum() == float(n[~np.isin(label, (
        "below_first_edge", "on_last_edge", "above_last_edge"))].sum())


@pytest.mark.parametrize("kind", ("default", "lowe2019"))
def test_the_ratio_filter_at_one_exactly(engine, kind):
    """droplets whose volume IS the critical volume at the parcel's temperature (ratio == 1.0),
    8 of them, among the same droplets a relative 1e-9 of mass below and above: [0, 1) excludes
    them, [1, inf) includes them"""
    formulae = pc.formulae_of(kind)
    rho_w = formulae.constants.rho_w
    rng = np.random.default_rng(9)
    n_try, T = 200, 287.5
    up = engine.upload

    def v_cr_of(mass, dry_volume, kappa, f_org):
        out = engine.empty(mass.size, FLOAT)
        critical_volume_call(engine, formulae, out, up(kappa), up(f_org), up(dry_volume),
                             up(mass / rho_w), up(np.array([T])),
                             up(np.zeros(mass.size, dtype=np.int64)), mass.size)
        return engine.download(out)

    # candidates: with a film of organics the critical volume depends on the wet volume, so
    # iterate to the fixed point, then walk the last ulps of the mass; not every critical volume
    # is m / rho_w of some double m, so keep the first 8 candidates that reach ratio == 1
    drops = (4 / 3 * np.pi * rng.uniform(3e-8, 2e-7, n_try) ** 3, rng.uniform(0.3, 1.2, n_try),
             rng.uniform(0.1, 0.5, n_try))
    mass = v_cr_of(np.full(n_try, 1e-15), *drops) * rho_w
    for _ in range(60):
        mass = v_cr_of(mass, *drops) * rho_w
    for _ in range(8):
        ratio = (mass / rho_w) / v_cr_of(mass, *drops)
        mass = np.where(ratio < 1, np.nextafter(mass, np.inf),
                        np.where(ratio > 1, np.nextafter(mass, 0), mass))
    exact = np.flatnonzero((mass / rho_w) / v_cr_of(mass, *drops) == 1)[:8]
    assert exact.size == 8
    dry_volume, kappa, f_org = (np.tile(column[exact], 3) for column in drops)
    kinds = np.repeat(np.arange(3), 8)  # 0: at one, 1: below, 2: above
    mass = np.tile(mass[exact], 3) * np.where(kinds == 1, 1 - 1e-9,
                                              np.where(kinds == 2, 1 + 1e-9, 1.0))
    ratio = (mass / rho_w) / v_cr_of(mass, dry_volume, kappa, f_org)
    assert (ratio[kinds == 0] == 1).all() and (ratio[kinds == 1] < 1).all() \
        and (ratio[kinds == 2] > 1).all()
    n = rng.integers(1, 1000, mass.size)
    name = "wet to critical volume ratio"
    table = RequestTable.from_requests(
        (MomentRequest("volume", 0, name, 0.0, 1.0, False),
         MomentRequest("volume", 0, name, 1.0, np.inf, False)),
        SpectrumRequest(name, (0.5, 1.0, 2.0)), formulae)
    got = evaluate(engine, formulae, table, counts=[mass.size], water_mass=mass, multiplicity=n,
                   dry_volume=dry_volume, kappa=kappa, f_org=f_org, T=T)
    below, rest = float(n[kinds == 1].sum()), float(n[kinds != 1].sum())
    assert got["moment_0"][0].tolist() == [below, rest]
    assert got["spectrum"][0].tolist() == [below, rest]


# ---- c. the product classes against the reference ------------------------------------------------------
def assert_products_match_the_reference(engine, data, run, general=None):
    """the recorded masses of every recorded step of `run` through `sdm_parcel_diagnose` (one
    parcel per recorded step, each at its recorded temperature) and the product classes: the
    reference's recorded values at MOMENT_RTOL, counts (the spectra, and the concentrations
    scaled back to counts) exactly"""
    get = lambda key: np.array(data[f"{run}/{key}"])  # noqa: E731
    formulae = pc.formulae_of("lowe2019" if run == "c" else "default")
    mass, n_steps = get("water_mass"), get("steps").size
    n_sd = mass.shape[1]
    groups = {}
    for product in ppc.golden_products(pr):
        groups.setdefault(product.spectrum(formulae), []).append(product)
    wet = [key for key in groups if key is not None and key.bin_attr == "volume"][0]
    groups[wet] += groups.pop(None)
    checked = 0
    for products in groups.values():
        table = RequestTable(products, formulae)
        raw = evaluate(engine, formulae, table, counts=[n_sd] * n_steps,
                       water_mass=mass.reshape(-1), multiplicity=np.tile(get("multiplicity"),
                                                                         n_steps),
                       dry_volume=np.tile(get("dry_volume"), n_steps),
                       kappa=np.tile(get("kappa"), n_steps), f_org=np.tile(get("f_org"), n_steps),
                       T=get("T"), general=(run == "c") if general is None else general)
        rows = Rows(table, moment_0=raw["moment_0"], moments=raw["moments"],
                    spectrum=raw["spectrum"], dv=get("dv"), rhod=get("rhod"))
        for product in products:
            value, recorded = product.get(formulae, rows), get(f"product/{product.name}")
            assert value.shape == recorded.shape, product.name
            np.testing.assert_allclose(value, recorded, rtol=MOMENT_RTOL, atol=0,
                                       err_msg=f"run {run}: {product.name}")
            assert np.array_equal(np.isnan(value), np.isnan(recorded)), product.name
            checked += 1
        # counts exactly: the reference's spectrum times dv (x rhod) x bin width is an integer
        spectrum = [p for p in products if p.spectrum(formulae) is not None][0]
        edges = np.asarray(spectrum.spectrum(formulae).edges)
        const = formulae.constants
        widths = np.power(edges[1:] / const.PI_4_3, const.ONE_THIRD) \
            - np.power(edges[:-1] / const.PI_4_3, const.ONE_THIRD)
        recorded = get(f"product/{spectrum.name}") * spectrum.unit_magnitude_in_base_units
        counts = recorded * widths * get("dv")[:, None]
        if spectrum.specific or spectrum.stp:
            counts = counts * get("rhod")[:, None]
        if spectrum.stp:
            counts = counts / (const.p_STP / const.Rd / const.T_STP)
        assert np.array_equal(np.rint(counts), raw["spectrum"]), spectrum.name
        np.testing.assert_allclose(counts, raw["spectrum"], rtol=1e-9, atol=1e-3)
        for product in products:
            if isinstance(product, pr.ParticleConcentration) and not product.specific \
                    and not product.stp:
                count = get(f"product/{product.name}") * product.unit_magnitude_in_base_units \
                    * get("dv")
                assert np.array_equal(np.rint(count), rows.moment_0(product.requests(formulae)[0]))
    assert checked == len(ppc.GOLDEN_PRODUCTS)


@pytest.mark.parametrize("run", "abc")
def test_product_classes_against_the_reference(engine, golden, run):
    assert_products_match_the_reference(engine, golden, run)
    if run != "c":  # PySDM's defaults through the general evaluation too
        assert_products_match_the_reference(engine, golden, run, general=True)


def test_recorded_runs_activate_and_deactivate(golden):
    assert golden["a/product/n_act"].max() > 0 and golden["c/product/n_act"].max() > 0
    n_act = np.array(golden["b/product/n_act"])
    assert n_act[-1] == 0 < n_act.max()  # run b: the droplets deactivate
    assert os.path.getsize(os.path.join(HERE, "golden", "parcel_products.npz")) \
        <= os.path.getsize(os.path.join(HERE, "golden", "parcel_runs.npz"))


def test_units_and_names():
    assert pr.ParticleConcentration().name == "particle concentration"
    assert pr.ParticleConcentration(unit="cm^-3").unit_magnitude_in_base_units \
        == pytest.approx(1e6, rel=1e-15)
    assert pr.WaterMixingRatio(unit="g/kg").unit_magnitude_in_base_units == 1e-3
    assert pr.ParticleSizeSpectrumPerMassOfDryAir(
        radius_bins_edges=(1e-6, 2e-6), unit="mg^-1 um^-1").unit_magnitude_in_base_units \
        == pytest.approx(1e12)
    with pytest.raises(AssertionError, match="dimensionality"):
        pr.MeanRadius(unit="kg")
    with pytest.raises(ValueError, match="precludes"):
        pr.ParticleConcentration(specific=True, stp=True)
    formulae = Formulae()
    shared = RequestTable(ppc.eleven(), formulae)
    assert shared.n_moments == 9 and shared.n_bins == 64  # identical requests are shared
    with pytest.raises(NotImplementedError, match="one size spectrum"):
        RequestTable(ppc.eleven() + (pr.ParticleSizeSpectrumPerVolume(
            name="other", radius_bins_edges=(1e-6, 2e-6)),), formulae)


# ---- d. route equivalence, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("kind,general", (("default", False), ("default", True),
                                          ("lowe2019", False)),
                         ids=("default", "default-general", "lowe2019"))
def test_fused_rows_equal_diagnose_after_each_step(engine, kind, general):
    """both evaluations of the checker, and the stage route of ParcelRunner (which serves the
    products with `sdm_parcel_diagnose` after each step): moment_0, moments, spectrum, dv"""
    kwargs = pc.ensemble((1, 65, 257, 1100), seed=11, f_org=kind != "default")
    fused = pc.runner(engine, kind, kwargs, "fused", general=general)
    table = ppc.full_table(fused.formulae)
    profile, rows = ppc.run_with_table(fused, table, (4,))
    assert profile["n_activating"].max() > 0
    staged = ppc.diagnose_after_each_step(
        pc.runner(engine, kind, kwargs, "fused", general=general), table, 4)
    stages = pc.runner(engine, kind, kwargs, "stages", general=general)
    profile_s, rows_s = ppc.run_with_table(stages, table, (4,))
    pc.assert_same_bits(profile, profile_s, "profile, fused vs stages")
    pc.assert_same_bits(rows, rows_s, "rows, fused vs stages")
    pc.assert_same_bits(fused.snapshot(), stages.snapshot(), "state, fused vs stages")
    # dv is the step's mid-point volume
    rhod0 = pc.runner(engine, kind, kwargs, "fused").snapshot()["rhod"]
    before = np.concatenate(([rhod0], profile["rhod"][:-1]))
    mass = np.asarray(kwargs["mass_of_dry_air"])
    assert np.array_equal(rows["dv"], mass / ((profile["rhod"] + before) / 2))
    rows.pop("dv")
    pc.assert_same_bits(rows, staged, "fused rows vs diagnose after each step")


def _dv_rows(engine, profile, kwargs):
    """the steps' mid-point volumes from the profile and a fresh runner's initial rhod"""
    rhod0 = pc.runner(engine, "default", kwargs, "fused").snapshot()["rhod"]
    before = np.concatenate(([rhod0], profile["rhod"][:-1]))
    return np.asarray(kwargs["mass_of_dry_air"]) / ((profile["rhod"] + before) / 2)


def test_products_of_a_run_and_of_the_initial_state(engine):
    """`run(products=...)` with the eleven products equals the products of `diagnose` after each
    step (given the step's dv); `profile=False` changes nothing; products without a run: the
    initial state"""
    kwargs = pc.ensemble((40, 300), seed=23)
    a, b, c = (pc.runner(engine, "default", kwargs, "fused") for _ in range(3))
    products = ppc.eleven()
    initial = a.diagnose(products)
    assert list(initial) == [p.name for p in products] and len(initial) == 11
    assert initial["particle concentration"].shape == (2,)
    assert initial["particle size spectrum per volume"].shape == (2, 64)
    assert (initial["particle concentration"] > 0).all()
    profile, values = a.run(3, products=products)
    nothing, values_b = b.run(3, profile=False, products=products)
    assert nothing is None and b.last_profile is None
    pc.assert_same_bits(values, values_b, "profile=False")
    assert a.run(0, products=products)[1]["mean radius"].shape == (0, 2)
    dv = _dv_rows(engine, profile, kwargs)
    for k in range(3):
        c.run(1)
        step = c.diagnose(products, dv=dv[k])
        pc.assert_same_bits({name: value[k] for name, value in values.items()}, step,
                            f"step {k}")


def test_resumption_across_launch_edges(engine):
    """run(4); run(5) == run(9) with steps_per_launch = 4: the rows cross launch edges"""
    kwargs = pc.ensemble((3, 65, 300), seed=13)
    results = []
    for splits in ((9,), (4, 5)):
        runner = pc.runner(engine, "default", kwargs, "fused", steps_per_launch=4)
        table = ppc.full_table(runner.formulae)
        results.append((*ppc.run_with_table(runner, table, splits), runner.snapshot()))
    for at, what in enumerate(("profile", "rows", "state")):
        pc.assert_same_bits(results[0][at], results[1][at], what)


@pytest.mark.parametrize("route", ("fused", "stages"))
def test_a_failing_parcel_leaves_its_rows_untouched(engine, route):
    """the outputs prefilled with a sentinel: the rows of the steps a failing parcel did not carry
    out keep it, the others hold values; both routes agree"""
    kind, setup, sizes, seed = pc.FAILURE_CASES[2]
    kwargs = pc.ensemble(sizes, seed=seed)
    sentinel = -7.25
    runner = pc.runner(engine, kind, kwargs, route, setup=setup)
    runner.diag_fill = sentinel
    table = ppc.full_table(runner.formulae)
    with pytest.raises(RuntimeError, match="Condensation failed"):
        runner.run(5, products=table)
    state, rows = runner.snapshot(), ppc.raw(runner.last_rows)
    failed, done = state["failed_step"], state["steps_done"]
    assert (failed >= 0).any() and (failed == -1).any() and (done[failed >= 0] > 0).any()
    for c in range(len(sizes)):
        for key, value in rows.items():
            assert (value[done[c]:, c] == sentinel).all(), (key, c)
            assert (value[:done[c], c] != sentinel).all(), (key, c)
    good = np.flatnonzero(failed == -1)
    clean = pc.runner(engine, kind, kwargs, "fused", setup=setup)
    with pytest.raises(RuntimeError, match="Condensation failed"):
        clean.run(5, products=table)
    for key, value in ppc.raw(clean.last_rows).items():  # (NaN-filled: compare the good ones)
        assert np.array_equal(pc.bits(np.ascontiguousarray(value[:, good])),
                              pc.bits(np.ascontiguousarray(rows[key][:, good]))), key


def test_refusals(engine):
    formulae = Formulae()
    columns = dict(counts=[4], water_mass=np.full(4, 1e-15), multiplicity=np.ones(4),
                   dry_volume=np.full(4, 1e-22), kappa=0.5, T=290.0)
    good = MomentRequest("volume", 1, "volume", 0.0, 1.0, False)

    def refused(moments, spectrum=None):
        table = RequestTable.from_requests(moments, spectrum, formulae)
        with pytest.raises(RuntimeError, match="error -"):
            evaluate(engine, formulae, table, **columns)
        runner = pc.runner(engine, "default", pc.ensemble((5, 9), seed=3), "fused")
        with pytest.raises(RuntimeError, match="error -"):
            runner.run(1, products=table)
        assert runner.snapshot()["steps_done"].tolist() == [0, 0]  # refused before any step

    refused(tuple(good._replace(min_x=-float(i)) for i in range(17)))  # 17 moment requests
    refused((good,), SpectrumRequest("volume", tuple(np.arange(1.0, 259.0))))  # 257 bins
    refused((good._replace(attr=5),))
    refused((good._replace(attr=-1),))
    refused((good._replace(filter_attr=4),))
    refused((good._replace(attr="no such attribute"),))
    refused((good,), SpectrumRequest(7, (1.0, 2.0)))
    refused((good,), SpectrumRequest("volume", (1.0, 2.0, 2.0)))  # not strictly increasing
    refused((good,), SpectrumRequest("volume", (1.0, 3.0, 2.0)))
    refused((good,), SpectrumRequest("volume", (1.0, np.nan, 2.0)))
    refused((good._replace(min_x=2.0, max_x=1.0),))  # min_x > max_x
    # and what is allowed: min_x == max_x (nothing selected), a table without moments
    table = RequestTable.from_requests((good._replace(min_x=1.0),), None, formulae)
    assert evaluate(engine, formulae, table, **columns)["moment_0"].tolist() == [[0.0]]
    table = RequestTable.from_requests((), SpectrumRequest("water mass", (1e-16, 1e-14)), formulae)
    assert evaluate(engine, formulae, table, **columns)["spectrum"].tolist() == [[4.0]]


def test_an_engine_without_the_library_says_so():
    from tests.parcel_checker import ParcelCheckerEngine  # pylint: disable=import-outside-toplevel

    runner = pc.runner(ParcelCheckerEngine.get(), "default", pc.ensemble((5, 9), seed=3), "fused")
    with pytest.raises(NotImplementedError, match="no parcel-diagnostics library"):
        runner.run(1, products=ppc.eleven())
    assert runner.run(1)["z"].shape == (1, 2)  # without products it runs as before


# ---- the PySDM hook ----------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "PySDM")),
                    reason="reference tree not present")
def test_run_parcel_products_against_the_front_end(engine):  # pylint: disable=unused-argument,too-many-locals
    """`run_parcel(particulator, steps, products=...)` against the reference's own product objects
    evaluated step by step by the unmodified front-end on the checker-bound backend (whose
    moments are the oracle's, summed in another order: MOMENT_RTOL; the spectra's counts equal)"""
    from tests import condensation_cases as cc  # pylint: disable=import-outside-toplevel

    os.environ.setdefault("CI", "1")
    added = [os.path.join(HERE, "golden", "standins"), REFERENCE]
    sys.path[:0] = added
    try:
        import PySDM.products as reference_products  # pylint: disable=import-outside-toplevel,import-error
        import PySDM.products.impl.product as product_module  # pylint: disable=import-outside-toplevel,import-error
        from PySDM import Builder  # pylint: disable=import-outside-toplevel,import-error
        from PySDM import Formulae as PySDMFormulae  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.dynamics import AmbientThermodynamics, Condensation  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.environments import Parcel  # pylint: disable=import-outside-toplevel,import-error
    except Exception as error:  # pylint: disable=broad-except
        pytest.skip(f"PySDM not importable here: {error}")
    finally:
        for path in added:
            sys.path.remove(path)
    from pysdm_amd.pysdm_plugin import as_pysdm_backend, run_parcel  # pylint: disable=import-outside-toplevel
    from tests.parcel_diag_checker import ParcelDiagCheckerBackend  # pylint: disable=import-outside-toplevel

    import re  # pylint: disable=import-outside-toplevel

    # (pint reads "kg^-1 m^-1" as a product; the stand-in wants the `*`)
    registry = product_module._UNIT_REGISTRY  # pylint: disable=protected-access
    parse = type(registry).parse_expression
    registry.parse_expression = lambda text, *a, **k: parse(
        re.sub(r"(?<=[\w)])\s+(?=[A-Za-z(])", " * ", str(text).strip()), *a, **k)

    gold = cc.gold("cond_parcel_a1")
    cfg = {k[len("parcel/"):]: gold[k] for k in gold.files if k.startswith("parcel/")}

    def twin(products):
        backend = as_pysdm_backend(ParcelDiagCheckerBackend)(PySDMFormulae())
        env = Parcel(dt=float(cfg["dt"]), mass_of_dry_air=float(cfg["mass_of_dry_air"]),
                     p0=float(cfg["p0"]), initial_water_vapour_mixing_ratio=float(cfg["qv0"]),
                     T0=float(cfg["T0"]), w=lambda t: 5.0 if t < 6 else 3.0)
        builder = Builder(n_sd=int(cfg["n_sd"]), backend=backend, environment=env)
        builder.add_dynamic(AmbientThermodynamics())
        builder.add_dynamic(Condensation(adaptive=True))
        attributes = {k[len("init/"):]: np.array(gold[k]) for k in gold.files
                      if k.startswith("init/")}
        return builder.build(attributes=attributes, products=products)

    try:
        stepped = twin(ppc.golden_products(reference_products)[:16])
    finally:
        del registry.parse_expression
    own = ppc.golden_products(pr)[:16]  # (all but the dry spectrum: one spectrum per run)
    steps = 8
    recorded = {p.name: [] for p in own}
    for _ in range(steps):
        stepped.run(1)
        for name in recorded:
            recorded[name].append(np.array(stepped.products[name].get(), dtype=float,
                                           copy=True).reshape(-1))
    fused = twin(())
    values = run_parcel(fused, steps, products=own)
    assert list(values) == [p.name for p in own]
    for name, series in recorded.items():
        expected = np.squeeze(np.stack(series))
        assert values[name].shape == expected.shape, name
        np.testing.assert_allclose(values[name], expected, rtol=MOMENT_RTOL, atol=0,
                                   err_msg=name)
    assert np.array_equal(fused.attributes["signed water mass"].to_ndarray(raw=True),
                          stepped.attributes["signed water mass"].to_ndarray(raw=True))
    assert run_parcel(fused, 1)["z"].shape == (1,)  # without products: the profile, as before

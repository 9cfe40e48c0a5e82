"""Shared by the deposition tests: the goldens of tests/golden/dep_*.npz
(gen_deposition_golden.py) replayed through a PySDM-shaped backend class or a `DepositionRunner`,
the tolerances against the reference, and seeded cases for HIP / checker parity.

Tolerances against the reference (which ran on NumPy's exp / log / power, not correctly rounded):
  masses            |out - gold| <= MASS_RTOL max(|gold|, |in|), MASS_RTOL = 1e-12: the project's
                    bound against the reference where transcendentals feed attributes (README,
                    tests/test_hip_parity.py).
  predicted columns per cell with n_c contributing rows: |out - gold| <= INCREMENT_RTOL |gold - in|
                    + n_c 2^-52 max(|in|, |gold|); the second term is the rounding of n_c
                    additions on each side.
  rows and cells the reference left unchanged: bit-identical to the input.
Measured on the checker (test_checker_replays_recorded_method_calls prints them), the largest
relative difference over the 8 recorded calls: 4.7e-15 for the masses (|out - gold| / max(|gold|,
|in|); 3.4e-16 or less in 7 of the 8 calls), and 1.3e-13 of the increment for the predicted
columns (|out - gold| / |gold - in|: one cell of one call differs, by one unit in the last place
of the predicted value - within the additions' rounding term; every other cell of every call has
the reference's bits).  The 20 recorded consecutive calls: masses 2.2e-16, cells bit-identical.
"""
import itertools
import os

import numpy as np

from pysdm_amd import deposition as dep
from pysdm_amd.formulae import Formulae

HERE = os.path.dirname(os.path.abspath(__file__))
MASS_RTOL = 1e-12
INCREMENT_RTOL = 1e-12
ULP = 2.0 ** -52
COMBINATIONS = list(itertools.product(("WaterMassLogarithm", "WaterMass"),
                                      ("Spherical", "Columnar"), ("Standard", "Neglect")))
AMBIENT = ("T", "p", "RH", "a_w_ice", "qv", "rhod", "thd")


def gold(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def formulae_for(coordinate="WaterMassLogarithm", capacity="Spherical", kinetics="Standard",
                 constants=None):
    return Formulae(particle_shape_and_density="MixedPhaseSpheres",
                    diffusion_coordinate=coordinate, diffusion_ice_capacity=capacity,
                    diffusion_ice_kinetics=kinetics, constants=constants)


def assert_same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64), err_msg=what)


# ---- a case: host arrays of one sdm_deposition call -----------------------------------------------
def contributing_rows(case):
    """the rows that add to their cell: ice (mass not > 0) in a cell with S_ice != 1"""
    s_ice = case["RH"] / case["a_w_ice"]
    return ~(case["signed_water_mass"] > 0) & (s_ice != 1)[case["cell_id"]]


def call_backend(backend_class, case, formulae):
    """the case through `Backend.deposition` (sum mode ORDERED); returns (mass, pqv, pthd)"""
    backend = backend_class(formulae)
    S = backend.Storage
    store = {k: S.from_ndarray(np.array(case[k])) for k in AMBIENT}
    mass = S.from_ndarray(np.array(case["signed_water_mass"]))
    pqv = S.from_ndarray(np.array(case["predicted_qv"]))
    pthd = S.from_ndarray(np.array(case["predicted_thd"]))
    n_sd = mass.shape[0]
    backend.deposition(
        multiplicity=S.from_ndarray(np.array(case["multiplicity"])), signed_water_mass=mass,
        current_temperature=store["T"], current_total_pressure=store["p"],
        current_relative_humidity=store["RH"], current_water_activity=store["a_w_ice"],
        current_vapour_mixing_ratio=store["qv"], current_dry_air_density=store["rhod"],
        current_dry_potential_temperature=store["thd"], cell_volume=float(case["cell_volume"]),
        time_step=float(case["time_step"]), cell_id=S.from_ndarray(np.array(case["cell_id"])),
        reynolds_number=S.from_ndarray(np.zeros(n_sd)),
        schmidt_number=S.from_ndarray(np.zeros(store["T"].shape[0])),
        predicted_vapour_mixing_ratio=pqv, predicted_dry_potential_temperature=pthd)
    return mass.to_ndarray(), pqv.to_ndarray(), pthd.to_ndarray()


def call_engine(engine, case, formulae, sum="ordered", misaligned=False, with_count=True):  # pylint: disable=redefined-builtin
    """the case through `sdm_deposition` on `engine`; returns (mass, pqv, pthd, n_exceeded).
    `misaligned`: the mass column is a view that starts one element into its buffer (8-byte but
    not 16-byte aligned)"""
    up = engine.upload
    n_sd = case["signed_water_mass"].shape[0]
    if misaligned:
        buffer = up(np.concatenate([[np.nan], case["signed_water_mass"]]))
        mass = buffer[1:]
    else:
        mass = up(np.array(case["signed_water_mass"]))
    pqv, pthd = up(np.array(case["predicted_qv"])), up(np.array(case["predicted_thd"]))
    count = up(np.array([-7], dtype=np.int64)) if with_count else None
    cfg = dep.deposition_cfg(formulae, case["time_step"], case["cell_volume"], sum)
    engine.call_deposition(
        "sdm_deposition", cfg, n_sd, case["T"].shape[0],
        up(np.array(case["multiplicity"], dtype=np.int64)), mass,
        up(np.array(case["cell_id"], dtype=np.int64)), *(up(np.array(case[k])) for k in AMBIENT),
        pqv, pthd, count, dep.constants_of(formulae))
    down = engine.download
    return (np.array(down(mass)), down(pqv), down(pthd),
            int(down(count)[0]) if with_count else None)


# ---- against the reference ------------------------------------------------------------------------
def golden_case(data, number):
    """recorded call `number` of dep_methods.npz: (case, formulae, (mass, pqv, pthd))"""
    case = {k: np.array(data[f"cell/{k}"]) for k in AMBIENT}
    for key in ("cell_id", "signed_water_mass", "multiplicity", "predicted_qv", "predicted_thd"):
        case[key] = np.array(data[key])
    case["cell_volume"] = float(data["cell_volume"])
    case["time_step"] = float(data[f"calls/{number}/time_step"])
    formulae = formulae_for(*(str(data[f"calls/{number}/{k}"])
                              for k in ("coordinate", "capacity", "kinetics")))
    want = tuple(np.array(data[f"calls/{number}/out_{k}"])
                 for k in ("signed_water_mass", "predicted_qv", "predicted_thd"))
    return case, formulae, want


def assert_within_reference_tolerance(case, got, want, what=""):
    """the bounds of this module's docstring; returns the largest relative differences seen:
    |out - gold| / max(|gold|, |in|) over the masses, |out - gold| / |gold - in| over the cells"""
    mass_in = case["signed_water_mass"]
    untouched = want[0].view(np.uint64) == mass_in.view(np.uint64)
    assert_same_bits(got[0][untouched], mass_in[untouched], f"{what}: rows left unchanged")
    scale = np.maximum(np.abs(want[0]), np.abs(mass_in))
    mass_diff = np.abs(got[0] - want[0]) / scale
    assert (mass_diff <= MASS_RTOL).all(), f"{what}: masses differ by {mass_diff.max():.3g}"
    n_c = np.bincount(case["cell_id"][contributing_rows(case)], minlength=case["T"].shape[0])
    worst_increment = 0.0
    for got_column, want_column, before in ((got[1], want[1], case["predicted_qv"]),
                                            (got[2], want[2], case["predicted_thd"])):
        same = want_column.view(np.uint64) == before.view(np.uint64)
        assert_same_bits(got_column[same], before[same], f"{what}: cells left unchanged")
        assert ((n_c == 0) <= same).all()
        increment = np.abs(want_column - before)
        rounding = n_c * ULP * np.maximum(np.abs(before), np.abs(want_column))
        diff = np.abs(got_column - want_column)
        assert (diff <= INCREMENT_RTOL * increment + rounding).all(), (
            f"{what}: cells differ by {diff} with increments {increment}")
        touched = ~same
        if touched.any():
            worst_increment = max(worst_increment,
                                  float((diff[touched] / increment[touched]).max()))
    return float(mass_diff.max()), worst_increment


def replay_steps(engine, data):
    """dep_steps.npz through a `DepositionRunner` over `AmbientColumns(mixed_phase=True)`, call by
    call FROM THE RECORDED INPUTS: before every step the population's masses, the ambient's rhod /
    thd / qv (current and predicted) and its T, p, RH, a_w_ice are set to what the reference had
    at that point, so no difference is carried from step to step and the tolerances of a single
    call hold unchanged (widening them for a free-running replay would need a bound on how the
    ambient methods' last bits - RH and a_w_ice enter through S_ice - 1, down to 2.6e-5 here -
    and the alternating cell's overshoot propagate, which is not argued here).  After the step the
    ambient accepts its predictions.  Yields per step (case, got, want, ambient after)."""
    from pysdm_amd.condensation import AmbientColumns  # pylint: disable=import-outside-toplevel
    from pysdm_amd.population import Population  # pylint: disable=import-outside-toplevel

    formulae = formulae_for()
    n_cell = data["rhod"].shape[0]
    population = Population(engine, multiplicity=np.array(data["multiplicity"]),
                            mass=np.array(data["signed_water_mass"]),
                            cell_id=np.array(data["cell_id"]), n_cell=n_cell)
    ambient = AmbientColumns(engine, formulae, rhod=np.array(data["rhod"]),
                             thd=np.array(data["thd"]), qv=np.array(data["qv"]),
                             mixed_phase=True)
    runner = dep.DepositionRunner(population, ambient, dt=float(data["dt"]),
                                  dv=float(data["dv"]))
    before = {k: np.array(data[k]) for k in ("signed_water_mass", "qv", "thd", "T", "p", "RH",
                                             "a_w_ice")}
    up, assign = engine.upload, engine.assign
    for step in range(int(data["n_steps"])):
        assign(runner.signed_water_mass, up(before["signed_water_mass"]))
        for column, key in ((ambient.qv, "qv"), (ambient.pqv, "qv"), (ambient.thd, "thd"),
                            (ambient.pthd, "thd"), (ambient.T, "T"), (ambient.p, "p"),
                            (ambient.RH, "RH"), (ambient.a_w_ice, "a_w_ice")):
            assign(column, up(before[key]))
        runner.step()
        out = runner.snapshot()
        case = dict(before, rhod=np.array(data["rhod"]), cell_id=np.array(data["cell_id"]),
                    predicted_qv=before["qv"], predicted_thd=before["thd"])
        after = {k: np.array(data[f"steps/{k}"][step]) for k in before}
        got = (out["signed_water_mass"], out["pqv"], out["pthd"])
        want = (after["signed_water_mass"], after["qv"], after["thd"])
        ambient.accept_predictions()
        down = engine.download
        yield case, got, want, {k: down(getattr(ambient, k)) for k in ("T", "p", "RH",
                                                                        "a_w_ice")}, after
        before = after
    runner.check()


# ---- seeded cases for parity ----------------------------------------------------------------------
def ambient_columns(rng, n_cell, s_one=()):
    """plausible cold cells; S_ice = RH / a_w_ice in [0.9, 1.15], exactly 1 in `s_one`"""
    T = rng.uniform(235.0, 268.0, n_cell)
    p = rng.uniform(40e3, 90e3, n_cell)
    a_w_ice = rng.uniform(0.7, 0.95, n_cell)
    RH = a_w_ice * rng.uniform(0.9, 1.15, n_cell)
    for c in s_one:
        RH[c] = a_w_ice[c]
    qv = rng.uniform(1e-4, 2e-3, n_cell)
    rhod = p / 287.0 / T
    thd = T * (1e5 / p) ** 0.2856
    return dict(T=T, p=p, RH=RH, a_w_ice=a_w_ice, qv=qv, rhod=rhod, thd=thd)


def case_of(rng, cell_id, ice, n_cell, s_one=(), time_step=0.004):
    """a case from its cell ids and ice mask: masses log-uniform in 1e-15 .. 1e-9 kg, ~5 % of the
    rows of multiplicity 0, predicted columns that differ from the current ones"""
    n_sd = cell_id.shape[0]
    case = ambient_columns(rng, n_cell, s_one)
    mass = np.exp(rng.uniform(np.log(1e-15), np.log(1e-9), n_sd))
    mass[ice] *= -1
    multiplicity = np.exp(rng.uniform(np.log(1e3), np.log(1e6), n_sd)).astype(np.int64)
    multiplicity[rng.uniform(size=n_sd) < 0.05] = 0
    case.update(cell_id=cell_id.astype(np.int64), signed_water_mass=mass,
                multiplicity=multiplicity, time_step=time_step, cell_volume=1.0,
                predicted_qv=case["qv"] * (1 + 1e-3 * rng.uniform(-1, 1, n_cell)),
                predicted_thd=case["thd"] + 0.1 * rng.uniform(-1, 1, n_cell))
    return case


def seeded_case(seed, n_sd, n_cell, *, ice=0.6, sort=False, s_one=(), empty=()):
    """`n_sd` rows spread over the cells not in `empty`; cell ids shuffled unless `sort`"""
    rng = np.random.default_rng(seed)
    allowed = np.array([c for c in range(n_cell) if c not in empty], dtype=np.int64)
    cell_id = allowed[rng.integers(0, allowed.shape[0], n_sd)]
    if sort:
        cell_id = np.sort(cell_id)
    return case_of(rng, cell_id, rng.uniform(size=n_sd) < ice, n_cell, s_one)


def counted_case(seed, counts, *, liquid=0, sort=False, s_one=()):
    """cell c gets exactly counts[c] ice rows (contributing unless c is in `s_one`) and `liquid`
    further liquid rows are spread over all cells"""
    rng = np.random.default_rng(seed)
    n_cell = len(counts)
    cell_id = np.concatenate([np.repeat(np.arange(n_cell), counts),
                              rng.integers(0, n_cell, liquid)]).astype(np.int64)
    ice = np.arange(cell_id.shape[0]) < int(np.sum(counts))
    order = np.argsort(cell_id, kind="stable") if sort else rng.permutation(cell_id.shape[0])
    return case_of(rng, cell_id[order], ice[order], n_cell, s_one)


def exceeding_case(seed, n_sd=300, n_cell=3, cell=1):
    """every ice row of `cell` (growing: S_ice = 1.1) takes more vapour than the cell's tiny qv
    holds; no row of another cell does.  Returns (case, number of such rows)"""
    case = seeded_case(seed, n_sd, n_cell)
    case["RH"][cell] = 1.1 * case["a_w_ice"][cell]
    case["qv"][cell] = 1e-300
    case["multiplicity"][case["cell_id"] == cell] = 1000
    rows = contributing_rows(case) & (case["cell_id"] == cell)
    return case, int(rows.sum())

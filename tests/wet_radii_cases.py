"""Shared by the tests of the initialisation path (include/sdm_initialisation.h) and by the
generator of their goldens (tests/golden/gen_wet_radii_golden.py): the formulae sets, the labels of
the rows, the measured differences and a NumPy restatement of minfun for the independent check."""
import json
import os

import numpy as np

from tests import condensation_cases as cc
from tests.condensation_formulae_cases import (CONSTANTS, HYGRO_CHOICES, SGM_CHOICES, formulae_for)

# one set per surface tension times hygroscopicity (the organic-film constants of
# tests/condensation_formulae_cases.py)
SETS = {f"{sgm}_{hygro}": {"surface_tension": sgm, "hygroscopicity": hygro}
        for sgm in SGM_CHOICES for hygro in HYGRO_CHOICES}
FAIL_OPTIONS = {}  # wet_radii_fail.npz: PySDM's defaults
RTOL, MAX_ITERS = 1e-5, 64  # equilibrate_wet_radii.py:12-13
GRID_PASS = 262144  # SDM_INIT_ROWS_PER_PASS of include/sdm_initialisation.h (a test checks it)

# the labels of a row (bit flags, `label` of wet_radii.npz): why the reference returned what it did
SOLVED, NOT_A_LT_B, FA_NEGATIVE = 1, 2, 4
# ... and what the row was put there for
RH_ABOVE_ONE, RH_ZERO, RH_ONE, F_ORG_ZERO, F_ORG_ONE, KAPPA_ZERO, KAPPA_TINY = (
    8, 16, 32, 64, 128, 256, 512)
LABEL_NAMES = {SOLVED: "solved", NOT_A_LT_B: "not a < b", FA_NEGATIVE: "fa < 0",
               RH_ABOVE_ONE: "RH > 1", RH_ZERO: "RH == 0", RH_ONE: "RH == 1",
               F_ORG_ZERO: "f_org == 0", F_ORG_ONE: "f_org == 1", KAPPA_ZERO: "kappa == 0",
               KAPPA_TINY: "kappa tiny"}

MEASURED_PATH = os.path.join(cc.HERE, "golden", "wet_radii_measured.json")
REGENERATE = "SDM_REGENERATE_WET_RADII_MEASURED"  # set to 1: the CPU test rewrites MEASURED_PATH


def measured():
    with open(MEASURED_PATH, encoding="utf-8") as file:
        return json.load(file)


def formulae_of(name):
    return formulae_for(SETS[name] if name in SETS else FAIL_OPTIONS)


def set_arrays(data, name):
    """{key: array} of one set of wet_radii.npz"""
    prefix = name + "/"
    return {key[len(prefix):]: np.array(data[key]) for key in data.files
            if key.startswith(prefix)}


# the sets with rows on which the reference's search finds no sign change (wet_radii_fail.npz,
# `no_sign_change/<set>/`: three solved rows, the failing rows, two solved rows)
NO_SIGN_CHANGE_SETS = ("Constant_KappaKoehler", "CompressedFilmOvadnevaite_KappaKoehler",
                       "CompressedFilmRuehl_KappaKoehler")


def no_sign_change_rows(data, name):
    """{key: array} of one `no_sign_change/<set>/` group of wet_radii_fail.npz"""
    return set_arrays(data, f"no_sign_change/{name}")


def call_set(engine, formulae, rows, T, RH, *, index=None, cell_id="rows", f_org="rows",
             rtol=RTOL, max_iters=MAX_ITERS):
    """`sdm_equilibrate_wet_radii` on the rows of a set (`index`: which of them, in that order;
    `cell_id` / `f_org`: "rows" = the set's own, None, or an array): host copies of r_wet, iters
    and the status words"""
    from pysdm_amd.initialisation import wet_radii_call  # pylint: disable=import-outside-toplevel

    pick = (lambda a: a) if index is None else (lambda a: np.ascontiguousarray(a[index]))
    r_wet, iters, status = wet_radii_call(
        engine, formulae, r_dry=pick(rows["r_dry"]),
        kappa_times_dry_volume=pick(rows["kappa_times_dry_volume"]), T=np.array(T),
        RH=np.array(RH), rtol=rtol, max_iters=max_iters,
        f_org=pick(rows["f_org"]) if isinstance(f_org, str) else f_org,
        cell_id=pick(rows["cell_id"]) if isinstance(cell_id, str) else cell_id)
    return engine.download(r_wet), engine.download(iters), engine.download(status)


def expected_status(iters, max_iters):
    """the status words the iteration counts imply"""
    bad = (iters == -1) | (iters == max_iters)
    return [int((iters == -1).sum()), int((iters == max_iters).sum()),
            int(np.flatnonzero(bad)[0]) if bad.any() else len(iters)]


def aerosol_step(engine, gold):
    """wet_aerosol at the golden's ambient state, then ONE non-adaptive condensation step: the
    aerosol dict, the water masses after the step and the largest relative change"""
    from pysdm_amd import spectra  # pylint: disable=import-outside-toplevel
    from pysdm_amd.condensation import (AmbientColumns, CondensationRunner,  # pylint: disable=import-outside-toplevel
                                        CondensationSetup)
    from pysdm_amd.formulae import Formulae  # pylint: disable=import-outside-toplevel
    from pysdm_amd.initialisation import wet_aerosol  # pylint: disable=import-outside-toplevel
    from pysdm_amd.population import Population  # pylint: disable=import-outside-toplevel

    cfg = {k[len("aerosol/"):]: gold[k] for k in gold.files if k.startswith("aerosol/")}
    formulae = Formulae()
    ambient = AmbientColumns(engine, formulae, rhod=cfg["rhod"], thd=cfg["thd"], qv=cfg["qv"])
    aerosol = wet_aerosol(
        engine, formulae, ambient, spectrum=spectra.Lognormal(*cfg["spectrum"]),
        kappa=float(cfg["kappa"]), n_sd=int(cfg["n_sd"]), cell_id=cfg["cell_id"],
        domain_volume=float(cfg["domain_volume"]))
    population = Population(engine, multiplicity=aerosol["multiplicity"],
                            mass=aerosol["water_mass"], cell_id=aerosol["cell_id"],
                            n_cell=len(cfg["rhod"]))
    setup = CondensationSetup(adaptive=False, substeps=int(cfg["n_substeps"][0]), rtol_x=1e-6,
                              rtol_thd=1e-9, dt_cond_range=(1e-4, float(cfg["dt"])))
    runner = CondensationRunner(population, ambient, setup, timestep=float(cfg["dt"]),
                                dv=float(cfg["dv"]), dry_volume=aerosol["dry_volume"],
                                kappa=aerosol["kappa"])
    runner.step()
    after = runner.snapshot()["water_mass"]
    change = float(np.max(np.abs(after - aerosol["water_mass"]) / aerosol["water_mass"]))
    return aerosol, after, change, cfg


class StubEnvironment:  # pylint: disable=too-few-public-methods
    """what equilibrate_wet_radii reads of a Kinematic2D: particulator.formulae, ["T"], ["RH"]"""

    def __init__(self, backend_class, formulae, T, RH):
        self.particulator = type("Particulator", (), {"formulae": formulae})()
        self.thermo = {"T": backend_class.Storage.from_ndarray(np.asarray(T)),
                       "RH": backend_class.Storage.from_ndarray(np.asarray(RH))}

    def __getitem__(self, item):
        return self.thermo[item]


def minfun_constant_sgm(formulae, hygroscopicity, r, T, RH, kappa, rd3):
    """RH - RH_eq with the constant surface tension sgm_w, in NumPy (hygroscopicity/
    kappa_koehler_leading_terms.py, kappa_koehler.py): the independent statement of what the solver
    solves, for the sign-change check"""
    k = formulae.constants
    A = 2 * k.sgm_w / k.Rv / T / k.rho_w
    RH = np.clip(RH, 0, 1)
    if hygroscopicity == "KappaKoehler":
        return RH - np.exp(A / r) * (r ** 3 - rd3) / (r ** 3 - rd3 * (1 - kappa))
    return RH - (1 + A / r - kappa * rd3 / r ** 3)

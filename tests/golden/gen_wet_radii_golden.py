#!/usr/bin/env python3
"""Generates the goldens of the initialisation path (tests/golden/wet_radii.npz,
wet_radii_fail.npz, lognormal_sampling.npz) by RUNNING THE REFERENCE (PySDM, its tree named by the
environment variable PYSDM_REFERENCE) in its pure-Python mode, with the same no-JIT import as
gen_condensation_formulae_golden.py (the stand-ins of tests/golden/standins put in front of it).
Run as:

    PYSDM_REFERENCE=<tree> PYTHONDONTWRITEBYTECODE=1 CI=1 \\
        python3 -B tests/golden/gen_wet_radii_golden.py [wet_radii] [fail] [sampling]

Written (the sets and the labels are tests/wet_radii_cases.py):
  wet_radii.npz  per set <surface tension>_<hygroscopicity>: 7 cells (T in 250..300 K, RH in
      {0, 0.2, 0.5, 0.9, 0.98, 1, 1.02}) and about 360 rows with r_dry from 1 nm to 5 um (rows on
      which the reference itself fails are left out); what
      PySDM.initialisation.equilibrate_wet_radii returned (`r_wet`), the iteration count of each
      row's TOMS748 search (`iters`, taken where the reference's function calls toms748_solve) and
      the labels of the rows.  Under `aerosol/`: a three-cell ambient state below saturation, a
      ConstantMultiplicity(Lognormal) sample brought to equilibrium by the reference, and the
      largest relative change of a water mass over ONE non-adaptive `backend.condensation` call of
      the reference from that state (`aerosol/max_relative_change`).
  wet_radii_fail.npz  one set (PySDM's defaults) with rtol = 1e-12 and max_iters 1 and 2: the
      reference itself returns max_iters; r_wet, iters and that its assertion fired.  Under
      `no_sign_change/<set>/`: the rows left out of wet_radii.npz, on which the reference returns
      (NaN, -1), between rows it solves.
  lognormal_sampling.npz  a single Lognormal and a two-mode Sum of Lognormals, n_sd 2^6 and 2^10,
      sampled by ConstantMultiplicity and Logarithmic: x and the counts; discretise_multiplicities
      of scaled counts.
"""
# pylint: disable=wrong-import-position,import-error,too-many-locals,protected-access
import os
import sys

os.environ.setdefault("CI", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.join(HERE, "standins"),
                os.environ["PYSDM_REFERENCE"]]

import numpy as np

from PySDM import Formulae
from PySDM.backends import CPU
from PySDM.initialisation import discretise_multiplicities, equilibrate_wet_radii, spectra
from PySDM.initialisation.sampling.spectral_sampling import ConstantMultiplicity, Logarithmic

from tests import wet_radii_cases as wc
from tests.golden.gen_condensation_formulae_golden import record_calls
from tests.golden.gen_condensation_golden import save

EWR = sys.modules["PySDM.initialisation.equilibrate_wet_radii"]
MIN_ROWS = 8  # of every label, in every set where it can occur
RH_CELLS = np.asarray([0.0, 0.2, 0.5, 0.9, 0.98, 1.0, 1.02])
T_CELLS = np.asarray([250.0, 300.0, 265.0, 280.0, 291.5, 273.15, 258.0])


class Env:  # pylint: disable=too-few-public-methods
    """the environment the reference's function reads: `particulator.formulae`, ["T"], ["RH"]"""

    def __init__(self, formulae, T, RH):
        self.particulator = type("Particulator", (), {"formulae": formulae})()
        self.thermo = {"T": CPU.Storage.from_ndarray(np.array(T)),
                       "RH": CPU.Storage.from_ndarray(np.array(RH))}

    def __getitem__(self, item):
        return self.thermo[item]


def reference_rows(formulae, *, r_dry, ktdv, f_org, cell_id, T, RH, rtol, max_iters):
    """(r_wet, iters, asserted) of the reference row by row: its function on one row at a time,
    the row's iteration count taken from the toms748_solve call the function makes (none: the row
    left early with iters = 0 and r_wet = r_dry); `asserted`: the closing assertion fired"""
    n = len(r_dry)
    r_wet, iters = np.full(n, np.nan), np.zeros(n, dtype=np.int64)
    asserted = np.zeros(n, dtype=bool)
    seen = []
    original = EWR.toms748_solve

    def recording(*args, **kwargs):
        out = original(*args, **kwargs)
        seen.append(out)
        return out

    EWR.toms748_solve = recording
    try:
        env = Env(formulae, T, RH)
        for i in range(n):
            seen.clear()
            row = slice(i, i + 1)
            try:
                out = equilibrate_wet_radii(
                    r_dry=r_dry[row], environment=env, kappa_times_dry_volume=ktdv[row],
                    f_org=f_org[row], cell_id=cell_id[row], rtol=rtol, max_iters=max_iters)
                r_wet[i] = out[0]
            except AssertionError:
                asserted[i] = True
            assert len(seen) <= 1
            if seen:
                iters[i] = seen[0][1]
                if asserted[i]:
                    r_wet[i] = seen[0][0]
                else:
                    assert r_wet[i] == seen[0][0] or (np.isnan(r_wet[i]) and np.isnan(seen[0][0]))
            else:
                assert not asserted[i] and r_wet[i] == r_dry[i]
    finally:
        EWR.toms748_solve = original
    return r_wet, iters, asserted


def rows_of(rng):
    """the rows of one set: (r_dry, kappa, f_org, cell_id, purpose flags)"""
    blocks = []

    def block(r_dry, kappa, f_org, cell, flags=0):
        n = len(r_dry)
        blocks.append((np.asarray(r_dry, dtype=float), np.broadcast_to(kappa, (n,)).astype(float),
                       np.broadcast_to(f_org, (n,)).astype(float),
                       np.broadcast_to(cell, (n,)).astype(np.int64),
                       np.full(n, flags, dtype=np.int64)))

    def radii(n):
        return np.exp(rng.uniform(np.log(1e-9), np.log(5e-6), n))

    # (the pole of the full kappa-Koehler RH_eq, kappa < 1, lies below r_dry: outside the bracket)
    n = 240
    block(radii(n), rng.uniform(0.05, 1.4, n), rng.uniform(0, 1, n), rng.integers(0, 7, n))
    block([1e-9, 5e-6, 1e-9, 5e-6], 0.6, 0.3, [3, 3, 4, 4])
    n = 12
    block(radii(n), 0.0, rng.uniform(0, 1, n), rng.integers(0, 7, n), wc.KAPPA_ZERO)
    block(np.exp(rng.uniform(np.log(1e-8), np.log(1e-7), n)), 1e-5, rng.uniform(0, 1, n),
          rng.integers(0, 7, n), wc.KAPPA_TINY)
    # the reference's own unit test: kappa 0.356, RH 0.9, T 280 (cell 3), f_org 0.607
    block(np.full(n, 2.4e-9), 0.356, 0.607, 3)
    block(np.full(n, 2.5e-9), 0.356, 0.607, 3)
    block(np.exp(rng.uniform(np.log(1.5e-9), np.log(4e-9), n)), 0.356, rng.uniform(0, 1, n), 3)
    big = np.exp(rng.uniform(np.log(2e-8), np.log(2e-6), 4 * n))
    block(big[:n], rng.uniform(0.1, 1.3, n), rng.uniform(0, 1, n), 6, wc.RH_ABOVE_ONE)
    block(big[n:2 * n], rng.uniform(0.1, 1.3, n), rng.uniform(0, 1, n), 0, wc.RH_ZERO)
    block(big[2 * n:3 * n], rng.uniform(0.1, 1.3, n), rng.uniform(0, 1, n), 5, wc.RH_ONE)
    block(big[3 * n:], rng.uniform(0.1, 1.3, n), 0.0, rng.integers(1, 5, n), wc.F_ORG_ZERO)
    block(np.exp(rng.uniform(np.log(2e-8), np.log(2e-6), n)), rng.uniform(0.1, 1.3, n), 1.0,
          rng.integers(1, 5, n), wc.F_ORG_ONE)
    columns = [np.concatenate(c) for c in zip(*blocks)]
    order = rng.permutation(len(columns[0]))
    return [c[order] for c in columns]


def generated_rows(at, options):
    """the rows generated for set number `at`, before any is left out: the formulae, the columns
    (r_dry, kappa, f_org, cell_id, purpose, ktdv) and on which rows the reference asserts"""
    rng = np.random.default_rng(20261019 + at)
    formulae = Formulae(constants=dict(wc.CONSTANTS), **options)
    r_dry, kappa, f_org, cell_id, purpose = rows_of(rng)
    ktdv = kappa * formulae.trivia.volume(radius=r_dry)
    with np.errstate(all="ignore"):
        _, _, asserted = reference_rows(
            formulae, r_dry=r_dry, ktdv=ktdv, f_org=f_org, cell_id=cell_id, T=T_CELLS,
            RH=RH_CELLS, rtol=wc.RTOL, max_iters=wc.MAX_ITERS)
    return formulae, (r_dry, kappa, f_org, cell_id, purpose, ktdv), asserted


def wet_radii():
    arrays = {"T": T_CELLS, "RH": RH_CELLS, "rtol": np.asarray(wc.RTOL),
              "max_iters": np.asarray(wc.MAX_ITERS)}
    for at, (name, options) in enumerate(wc.SETS.items()):
        formulae, (r_dry, kappa, f_org, cell_id, purpose, ktdv), asserted = generated_rows(
            at, options)
        with np.errstate(all="ignore"):
            # rows on which the reference itself fails (no sign change between r_dry and r_cr: the
            # smallest particles under the full kappa-Koehler curve, whose maximum lies beyond the
            # leading-terms r_cr) are left out here; wet_radii_fail.npz pins them
            keep = ~asserted
            print(name, "left out (the reference fails):", int(asserted.sum()))
            r_dry, kappa, f_org, cell_id, purpose, ktdv = (
                a[keep] for a in (r_dry, kappa, f_org, cell_id, purpose, ktdv))
            whole = equilibrate_wet_radii(
                r_dry=r_dry, environment=Env(formulae, T_CELLS, RH_CELLS),
                kappa_times_dry_volume=ktdv, f_org=f_org, cell_id=cell_id, rtol=wc.RTOL,
                max_iters=wc.MAX_ITERS)
            r_wet, iters, asserted = reference_rows(
                formulae, r_dry=r_dry, ktdv=ktdv, f_org=f_org, cell_id=cell_id, T=T_CELLS,
                RH=RH_CELLS, rtol=wc.RTOL, max_iters=wc.MAX_ITERS)
        assert not asserted.any()
        np.testing.assert_array_equal(whole, r_wet)
        # why a row left early: the two conditions of equilibrate_wet_radii.py:71,86, evaluated
        # with the reference's formulae
        const = formulae.constants
        label = purpose.copy()
        with np.errstate(all="ignore"):
            kp = ktdv / formulae.trivia.volume(radius=r_dry)
            b = formulae.hygroscopicity.r_cr(kp, r_dry ** 3, T_CELLS[cell_id], const.sgm_w)
        for i, rd in enumerate(r_dry):
            if iters[i] > 0:
                label[i] |= wc.SOLVED
            elif not rd < b[i]:
                label[i] |= wc.NOT_A_LT_B
            else:
                with np.errstate(all="ignore"):
                    sgm = formulae.surface_tension.sigma(
                        T_CELLS[cell_id[i]], formulae.trivia.volume(radius=rd),
                        const.PI_4_3 * rd ** 3, f_org[i])
                    fa = min(1, max(0, RH_CELLS[cell_id[i]])) - formulae.hygroscopicity.RH_eq(
                        rd, T_CELLS[cell_id[i]], kp[i], rd ** 3, sgm)
                if fa < 0:
                    label[i] |= wc.FA_NEGATIVE
                # (else: the search itself returned without an iteration, e.g. fa == 0)
        counts = {flag: int(np.count_nonzero(label & flag)) for flag in wc.LABEL_NAMES}
        print(name, len(r_dry), "rows;", {wc.LABEL_NAMES[f]: c for f, c in counts.items()},
              "iters max", iters.max())
        for flag, count in counts.items():
            can_occur = flag != wc.FA_NEGATIVE or options["hygroscopicity"] != "KappaKoehler"
            assert count >= MIN_ROWS or not can_occur, (name, wc.LABEL_NAMES[flag], count)
        assert r_dry.min() == 1e-9 and r_dry.max() == 5e-6
        arrays.update({f"{name}/r_dry": r_dry, f"{name}/kappa_times_dry_volume": ktdv,
                       f"{name}/f_org": f_org, f"{name}/cell_id": cell_id,
                       f"{name}/r_wet": r_wet, f"{name}/iters": iters, f"{name}/label": label})
    arrays.update(aerosol())
    save("wet_radii", **arrays)


AEROSOL = dict(n_sd=96, kappa=0.61, spectrum=(120e6, 0.04e-6, 1.6), dt=1.0, dv=1e6,
               domain_volume=3e6)


def aerosol():
    """ConstantMultiplicity(Lognormal) -> equilibrate_wet_radii -> one non-adaptive
    `backend.condensation` call of the reference at the same ambient state"""
    cfg = AEROSOL
    formulae = Formulae()
    backend = CPU(formulae)
    const = formulae.constants
    S = backend.Storage
    n_cell, n_sd = 3, cfg["n_sd"]
    rhod = np.asarray([1.0, 1.1, 1.2])
    thd = np.asarray([288.0, 292.0, 296.0])
    T = formulae.state_variable_triplet.T(rhod, thd)
    target_rh = np.asarray([0.80, 0.92, 0.985])
    qv = np.full(n_cell, 0.008)
    for _ in range(30):  # fixed point: p depends on qv
        p = formulae.state_variable_triplet.p(rhod, T, qv)
        pv = target_rh * formulae.saturation_vapour_pressure.pvs_water(T)
        qv = const.eps * pv / (p - pv)
    T_s, p_s, RH_s = (S.from_ndarray(np.zeros(n_cell)) for _ in range(3))
    backend.temperature_pressure_rh(rhod=S.from_ndarray(rhod), thd=S.from_ndarray(thd),
                                    water_vapour_mixing_ratio=S.from_ndarray(qv), T=T_s, p=p_s,
                                    RH=RH_s)
    norm, mode, s_geom = cfg["spectrum"]
    spectrum = spectra.Lognormal(norm_factor=norm, m_mode=mode, s_geom=s_geom)
    r_dry, n_per_kg = ConstantMultiplicity(spectrum).sample(n_sd)
    cell_id = (np.arange(n_sd) % n_cell).astype(np.int64)
    dry_volume = formulae.trivia.volume(radius=r_dry)
    env = Env(formulae, T_s.to_ndarray(), RH_s.to_ndarray())
    r_wet = equilibrate_wet_radii(r_dry=r_dry, environment=env,
                                  kappa_times_dry_volume=cfg["kappa"] * dry_volume,
                                  cell_id=cell_id)
    multiplicity = discretise_multiplicities(n_per_kg * rhod[cell_id] * cfg["domain_volume"])
    water_mass = const.rho_w * formulae.trivia.volume(radius=r_wet)
    idx = np.argsort(cell_id, kind="stable").astype(np.int64)
    cell_start = np.zeros(n_cell + 1, dtype=np.int64)
    cell_start[1:] = np.cumsum(np.bincount(cell_id, minlength=n_cell))
    state = dict(water_mass=water_mass, multiplicity=multiplicity, vdry=dry_volume,
                 kappa=np.full(n_sd, cfg["kappa"]), f_org=np.zeros(n_sd), idx=idx,
                 cell_start_arg=cell_start, cell_id=cell_id, reynolds_number=np.zeros(n_sd),
                 rhod=rhod, thd=thd, water_vapour_mixing_ratio=qv, prhod=rhod.copy(),
                 pthd=thd.copy(), predicted_water_vapour_mixing_ratio=qv.copy(),
                 air_density=rhod * (1 + qv),
                 air_dynamic_viscosity=formulae.air_dynamic_viscosity.eta_air(env["T"].data))
    calls = record_calls(backend, state, env["T"].data, n_cell=n_cell, dt=cfg["dt"],
                         dt_range=(1e-4, cfg["dt"]), modes=(False,))
    after = calls["calls/out_water_mass"][0]
    assert calls["calls/out_success"].all()
    change = float(np.max(np.abs(after - water_mass) / water_mass))
    print("aerosol: largest relative change of a water mass over one condensation call", change,
          "substeps", calls["calls/out_n_substeps"].tolist())
    out = {f"aerosol/{k}": np.asarray(v, dtype=float) for k, v in cfg.items()}
    out.update({"aerosol/rhod": rhod, "aerosol/thd": thd, "aerosol/qv": qv,
                "aerosol/cell_id": cell_id, "aerosol/r_dry": r_dry, "aerosol/n_per_kg": n_per_kg,
                "aerosol/r_wet": r_wet, "aerosol/multiplicity": multiplicity,
                "aerosol/water_mass": water_mass, "aerosol/water_mass_after": after,
                "aerosol/n_substeps": calls["calls/in_n_substeps"][0],
                "aerosol/max_relative_change": np.asarray(change)})
    return out


def fail():
    rng = np.random.default_rng(20261027)
    formulae = Formulae(constants=dict(wc.CONSTANTS), **wc.FAIL_OPTIONS)
    n = 48
    r_dry = np.exp(rng.uniform(np.log(5e-9), np.log(2e-6), n))
    kappa = rng.uniform(0.05, 1.3, n)
    kappa[:6] = 0.0  # (rows that leave early stay at iters = 0)
    cell_id = rng.integers(0, 7, n).astype(np.int64)
    ktdv = kappa * formulae.trivia.volume(radius=r_dry)
    arrays = {"T": T_CELLS, "RH": RH_CELLS, "rtol": np.asarray(1e-12), "r_dry": r_dry,
              "kappa_times_dry_volume": ktdv, "cell_id": cell_id,
              "max_iters": np.asarray([1, 2], dtype=np.int64)}
    for max_iters in (1, 2):
        with np.errstate(all="ignore"):
            r_wet, iters, asserted = reference_rows(
                formulae, r_dry=r_dry, ktdv=ktdv, f_org=np.zeros(n), cell_id=cell_id, T=T_CELLS,
                RH=RH_CELLS, rtol=1e-12, max_iters=max_iters)
        bad = (iters == max_iters) | (iters == -1)
        np.testing.assert_array_equal(bad, asserted)
        print("fail: max_iters", max_iters, "rows at max_iters", int((iters == max_iters).sum()),
              "rows at -1", int((iters == -1).sum()))
        assert bad.sum() >= MIN_ROWS
        arrays.update({f"r_wet/{max_iters}": r_wet, f"iters/{max_iters}": iters,
                       f"asserted/{max_iters}": asserted})
    arrays.update(no_sign_change())
    save("wet_radii_fail", **arrays)


def no_sign_change():
    """the rows left out of wet_radii.npz: the reference's TOMS748 finds no sign change between
    r_dry and r_cr and returns (NaN, -1).  Per set that has such rows: three rows the reference
    solves, the failing rows, two more it solves, with what it returned (default rtol and
    max_iters)"""
    out, total = {}, 0
    for at, (name, options) in enumerate(wc.SETS.items()):
        formulae, columns, asserted = generated_rows(at, options)
        if not asserted.any():
            continue
        r_dry, _, f_org, cell_id, _, ktdv = columns
        good = np.flatnonzero(~asserted & (ktdv > 0) & (RH_CELLS[cell_id] > 0.4)
                              & (r_dry > 2e-8))[:5]
        pick = np.concatenate([good[:3], np.flatnonzero(asserted), good[3:]])
        with np.errstate(all="ignore"):
            r_wet, iters, bad = reference_rows(
                formulae, r_dry=r_dry[pick], ktdv=ktdv[pick], f_org=f_org[pick],
                cell_id=cell_id[pick], T=T_CELLS, RH=RH_CELLS, rtol=wc.RTOL,
                max_iters=wc.MAX_ITERS)
        n_bad = int(asserted.sum())
        np.testing.assert_array_equal(bad, [False] * 3 + [True] * n_bad + [False] * 2)
        assert (iters[bad] == -1).all() and np.isnan(r_wet[bad]).all() and (iters[~bad] > 0).all()
        total += n_bad
        prefix = f"no_sign_change/{name}/"
        out.update({prefix + "r_dry": r_dry[pick], prefix + "kappa_times_dry_volume": ktdv[pick],
                    prefix + "f_org": f_org[pick], prefix + "cell_id": cell_id[pick],
                    prefix + "r_wet": r_wet, prefix + "iters": iters})
    print("no sign change: rows at -1:", total, "in", len(out) // 6, "sets")
    assert total >= 7
    return out


def sampling():
    single = spectra.Lognormal(norm_factor=120e6, m_mode=0.04e-6, s_geom=1.6)
    modes = ((60e6, 0.04e-6, 1.4), (40e6, 0.15e-6, 1.6))
    both = spectra.Sum(tuple(spectra.Lognormal(norm_factor=n, m_mode=m, s_geom=s)
                             for n, m, s in modes))
    arrays = {"single/params": np.asarray([120e6, 0.04e-6, 1.6]),
              "sum/params": np.asarray(modes)}
    probe = np.exp(np.linspace(np.log(1e-9), np.log(5e-6), 200))
    quantiles = np.linspace(1e-5, 0.99999, 201)
    for name, spectrum in (("single", single), ("sum", both)):
        arrays[f"{name}/probe"] = probe
        arrays[f"{name}/cumulative"] = spectrum.cumulative(probe)
        arrays[f"{name}/quantiles"] = quantiles
        arrays[f"{name}/percentiles"] = spectrum.percentiles(quantiles)
        for n_sd in (2 ** 6, 2 ** 10):
            for sampler_name, sampler in (("constant_multiplicity", ConstantMultiplicity),
                                          ("logarithmic", Logarithmic)):
                x, counts = sampler(spectrum).sample(n_sd)
                arrays[f"{name}/{sampler_name}/{n_sd}/x"] = x
                arrays[f"{name}/{sampler_name}/{n_sd}/counts"] = counts
    x, counts = ConstantMultiplicity(single).sample(2 ** 6)
    arrays["discretise/in"] = counts * 3e-3
    arrays["discretise/out"] = discretise_multiplicities(arrays["discretise/in"])
    save("lognormal_sampling", **arrays)


if __name__ == "__main__":
    for item in sys.argv[1:] or ["wet_radii", "fail", "sampling"]:
        {"wet_radii": wet_radii, "fail": fail, "sampling": sampling}[item]()

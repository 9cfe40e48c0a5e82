#!/usr/bin/env python3
"""Generates the freezing goldens (tests/golden/frz_*.npz) by RUNNING THE REFERENCE (PySDM at
/root/reference) in its pure-Python mode, with the same no-JIT import as gen_golden.py (the
stand-ins of tests/golden/standins put in front of it).  Run as:

    PYTHONDONTWRITEBYTECODE=1 CI=1 python3 -B tests/golden/gen_freezing_golden.py

Written:
  frz_methods.npz  direct backend-method calls on a seeded state of 1000 super-droplets over 7
      cells (T above / below T0, RH and RH_ice above / below 1, d_a_w_ice below KOOP_MIN, inside
      the range and above KOOP_MAX; masses of both signs; ~10 % zeros in freezing_temperature and
      immersed_surface_area), `thaw` both ways: freeze_singular; freeze_time_dependent x
      {Constant, ABIFM}; freeze_time_dependent_homogeneous x {Constant, Koop2000,
      Koop_Correction, KoopMurray2016}; record_freezing_temperatures over freeze -> thaw ->
      refreeze; a_w_ice; volume_of_water_mass / mass_of_water_volume.  Inputs, uniforms (one
      array, used by every stochastic call) and outputs; an output mass column is stored as the
      packed mask of the rows whose sign flipped (asserted to be the whole difference).
  frz_box_singular.npz / frz_box_abifm.npz / frz_box_hom.npz  an unmodified Builder + Box +
      Freezing(...) with 256 super-droplets, 20 steps, T / RH / a_w_ice / RH_ice set per step
      along a cooling ramp (stored); the signed water mass after every step.

Asserted (a seed is tried after another until it holds): in every stochastic call every evaluated
droplet has |rand - prob| > 1e-9 * max(prob, 1e-300), so that the recorded decisions do not depend
on the last bit of pow / exp; and between 10 % and 90 % of the eligible droplets (those for which
a probability was evaluated at least once) freeze over a run, so that no test passes on an
all-or-nothing case.
"""
# pylint: disable=wrong-import-position,import-error,too-many-locals,protected-access
import os
import sys

os.environ.setdefault("CI", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "standins"), "/root/reference"]

import numpy as np

from PySDM import Builder, Formulae
from PySDM.backends import CPU
from PySDM.backends.impl_common.freezing_attributes import (
    SingularAttributes, TimeDependentAttributes, TimeDependentHomogeneousAttributes)
from PySDM.dynamics import Freezing
from PySDM.environments import Box
from PySDM.physics import si

OUT = HERE
MARGIN = 1e-9
# Knopf & Alpert 2013, illite
ABIFM = {"ABIFM_M": 54.48, "ABIFM_C": -10.67}
J_HET = 2e10 / si.m ** 2 / si.s
J_HOM = 3e14 / si.m ** 3 / si.s
HET = {"Constant": {"J_HET": J_HET}, "ABIFM": ABIFM}
HOM = {"Constant": {"J_HOM": J_HOM}, "Koop2000": {}, "Koop_Correction": {}, "KoopMurray2016": {}}


class Retry(Exception):
    pass


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


def formulae_for(het="Null", hom="Null", seed=None):
    constants = {**HET.get(het, {}), **HOM.get(hom, {})}
    return Formulae(particle_shape_and_density="MixedPhaseSpheres",
                    heterogeneous_ice_nucleation_rate=het, homogeneous_ice_nucleation_rate=hom,
                    constants=constants, seed=seed)


class Tally:
    """eligible / frozen droplets of the stochastic calls, and the margin condition"""

    def __init__(self):
        self.eligible, self.frozen, self.run = set(), set(), 0  # (run, droplet) pairs

    def next_run(self):
        """what follows is another run over the droplets (a new call on the initial state)"""
        self.run += 1

    def time_dependent(self, formulae, *, rand, mass, area, dt, cell, a_w_ice, T, RH, thaw):
        const = formulae.constants
        for i in range(len(mass)):
            c = cell[i]
            if area[i] == 0 or (thaw and mass[i] < 0 and T[c] > const.T0):
                continue
            if mass[i] > 0 and RH[c] > 1:
                rate = formulae.heterogeneous_ice_nucleation_rate.j_het(a_w_ice[c]) * area[i]
                self._one(formulae, rate, dt, rand[i], i)

    def homogeneous(self, formulae, *, rand, mass, volume, dt, cell, a_w_ice, T, RH_ice, thaw):
        const = formulae.constants
        hom = formulae.homogeneous_ice_nucleation_rate
        for i in range(len(mass)):
            c = cell[i]
            if thaw and mass[i] < 0 and T[c] > const.T0:
                continue
            if mass[i] > 0 and RH_ice[c] > 1:
                d = (RH_ice[c] - 1.0) * a_w_ice[c]
                if hom.d_a_w_ice_within_range(d):
                    rate = hom.j_hom(T[c], hom.d_a_w_ice_maximum(d)) * volume[i]
                    self._one(formulae, rate, dt, rand[i], i)

    def _one(self, formulae, rate, dt, rand, droplet):
        prob = float(1 - formulae.trivia.poissonian_avoidance_function(rate, dt))
        if not abs(rand - prob) > MARGIN * max(prob, 1e-300):
            raise Retry(f"rand {rand!r} too close to prob {prob!r}")
        self.eligible.add((self.run, droplet))
        if rand < prob:
            self.frozen.add((self.run, droplet))

    def check(self, what):
        fraction = len(self.frozen) / max(len(self.eligible), 1)
        print(f"{what}: {len(self.frozen)} of {len(self.eligible)} eligible droplets freeze "
              f"({100 * fraction:.1f} %)")
        if not 0.1 <= fraction <= 0.9:
            raise Retry(f"{what}: {fraction:.3f} of the eligible droplets freeze")


# ---- frz_methods ---------------------------------------------------------------------------------
N_SD, N_CELL = 1000, 7
CELLS = dict(
    T=np.array([280.0, 250.0, 236.0, 234.5, 233.0, 275.0, 240.0]),
    RH=np.array([1.02, 1.05, 0.98, 1.10, 1.20, 0.90, 1.01]),
    RH_ice=np.array([0.95, 1.30, 1.45, 1.50, 1.90, 0.99, 1.35]),
    # d_a_w_ice = (RH_ice - 1) a_w_ice: -, 0.234 (< MIN), 0.315, 0.33, 0.603 (> MAX), -, 0.252
    a_w_ice=np.array([1.05, 0.78, 0.70, 0.66, 0.67, 1.00, 0.72]),
)


def methods(seed):
    rng = np.random.default_rng(seed)
    arrays = {f"cell/{k}": v for k, v in CELLS.items()}
    cell = rng.integers(0, N_CELL, N_SD).astype(np.int64)
    radius = np.exp(rng.uniform(np.log(0.05e-6), np.log(30e-6), N_SD))
    plain = formulae_for()
    const = plain.constants
    mass = const.rho_w * const.PI_4_3 * radius ** 3
    frozen = rng.uniform(size=N_SD) < 0.35
    mass[frozen] = -mass[frozen] * const.rho_i / const.rho_w
    t_fz = rng.uniform(228.0, 262.0, N_SD)
    t_fz[rng.uniform(size=N_SD) < 0.1] = 0.0
    area = np.exp(rng.uniform(np.log(1e-13), np.log(1e-9), N_SD))
    area[rng.uniform(size=N_SD) < 0.1] = 0.0
    volume = np.maximum(0.0, mass) / const.rho_w + np.minimum(0.0, mass) / const.rho_i
    dt = 0.5
    arrays.update(cell=cell, signed_water_mass=mass, freezing_temperature=t_fz,
                  immersed_surface_area=area, volume=volume, timestep=np.asarray(dt),
                  seed=np.asarray(seed))
    tally = Tally()
    calls = []
    shared_rand = rng.uniform(size=N_SD)  # every stochastic call draws these
    arrays["rand"] = shared_rand

    def storages(backend):
        S = backend.Storage
        return S, {k: S.from_ndarray(v.copy()) for k, v in CELLS.items()}

    for thaw in (False, True):
        backend = CPU(plain)
        S, env = storages(backend)
        m = S.from_ndarray(mass.copy())
        backend.freeze_singular(
            attributes=SingularAttributes(freezing_temperature=S.from_ndarray(t_fz.copy()),
                                          signed_water_mass=m),
            temperature=env["T"], relative_humidity=env["RH"], cell=S.from_ndarray(cell),
            thaw=thaw)
        calls.append(("singular", "", thaw, None, m.to_ndarray()))
        for het in HET:
            formulae = formulae_for(het=het)
            backend = CPU(formulae)
            S, env = storages(backend)
            rand = shared_rand
            m = S.from_ndarray(mass.copy())
            if het == "Constant":  # must not be looked at
                env["a_w_ice"] = S.from_ndarray(np.full(N_CELL, np.nan))
            tally.next_run()
            tally.time_dependent(formulae, rand=rand, mass=mass, area=area, dt=dt, cell=cell,
                                 a_w_ice=CELLS["a_w_ice"], T=CELLS["T"], RH=CELLS["RH"],
                                 thaw=thaw)
            backend.freeze_time_dependent(
                rand=S.from_ndarray(rand.copy()),
                attributes=TimeDependentAttributes(
                    immersed_surface_area=S.from_ndarray(area.copy()), signed_water_mass=m),
                timestep=dt, cell=S.from_ndarray(cell), a_w_ice=env["a_w_ice"],
                temperature=env["T"], relative_humidity=env["RH"], thaw=thaw)
            calls.append(("time_dependent", het, thaw, rand, m.to_ndarray()))
        for hom in HOM:
            formulae = formulae_for(hom=hom)
            backend = CPU(formulae)
            S, env = storages(backend)
            rand = shared_rand
            m = S.from_ndarray(mass.copy())
            tally.next_run()
            tally.homogeneous(formulae, rand=rand, mass=mass, volume=volume, dt=dt, cell=cell,
                              a_w_ice=CELLS["a_w_ice"], T=CELLS["T"], RH_ice=CELLS["RH_ice"],
                              thaw=thaw)
            backend.freeze_time_dependent_homogeneous(
                rand=S.from_ndarray(rand.copy()),
                attributes=TimeDependentHomogeneousAttributes(
                    volume=S.from_ndarray(volume.copy()), signed_water_mass=m),
                timestep=dt, cell=S.from_ndarray(cell), a_w_ice=env["a_w_ice"],
                temperature=env["T"], relative_humidity_ice=env["RH_ice"], thaw=thaw)
            calls.append(("homogeneous", hom, thaw, rand, m.to_ndarray()))
    tally.check("frz_methods")
    for number, (kind, rate, thaw, rand, out) in enumerate(calls):
        assert (out != mass).any(), (kind, rate, thaw)
        arrays[f"calls/{number}/kind"] = np.asarray(kind)
        arrays[f"calls/{number}/rate"] = np.asarray(rate)
        arrays[f"calls/{number}/thaw"] = np.asarray(int(thaw))
        # freezing and thawing are m = -1 * m: the output is stored as the mask of flipped rows
        flipped = out != mass
        np.testing.assert_array_equal(out, np.where(flipped, -1 * mass, mass))
        arrays[f"calls/{number}/out_flipped"] = np.packbits(flipped)
    arrays["n_calls"] = np.asarray(len(calls))

    # record_freezing_temperatures over freeze -> thaw -> refreeze (Constant rate, thaw on)
    formulae = formulae_for(het="Constant")
    backend = CPU(formulae)
    S, _ = storages(backend)
    data = S.from_ndarray(np.full(N_SD, np.nan))
    m = S.from_ndarray(mass.copy())
    cell_s, area_s = S.from_ndarray(cell), S.from_ndarray(area.copy())
    cold, warm = CELLS["T"].copy(), CELLS["T"] + 45.0
    colder = CELLS["T"] - 7.5
    for stage, temperature in enumerate((cold, warm, colder)):
        rand = shared_rand
        before = m.to_ndarray()
        T_s = S.from_ndarray(temperature.copy())
        tally_stage = Tally()
        tally_stage.time_dependent(formulae, rand=rand, mass=before, area=area, dt=dt, cell=cell,
                                   a_w_ice=CELLS["a_w_ice"], T=temperature, RH=CELLS["RH"],
                                   thaw=True)
        backend.freeze_time_dependent(
            rand=S.from_ndarray(rand.copy()),
            attributes=TimeDependentAttributes(immersed_surface_area=area_s,
                                               signed_water_mass=m),
            timestep=dt, cell=cell_s, a_w_ice=S.from_ndarray(np.full(N_CELL, np.nan)),
            temperature=T_s, relative_humidity=S.from_ndarray(CELLS["RH"].copy()), thaw=True)
        backend.record_freezing_temperatures(data=data, cell_id=cell_s, temperature=T_s,
                                             signed_water_mass=m)
        arrays[f"record/{stage}/T"] = temperature
        flipped = m.to_ndarray() != mass
        np.testing.assert_array_equal(m.to_ndarray(), np.where(flipped, -1 * mass, mass))
        arrays[f"record/{stage}/out_flipped"] = np.packbits(flipped)
        arrays[f"record/{stage}/out_data"] = data.to_ndarray()
    last = arrays["record/2/out_data"]
    assert np.isnan(last).any() and (last == colder[cell])[~np.isnan(last)].any()
    assert (arrays["record/1/out_data"] != arrays["record/0/out_data"]).any()

    # a_w_ice on a physically consistent ambient state
    backend = CPU(plain)
    S = backend.Storage
    n = 40
    T = rng.uniform(215.0, 285.0, n)
    p = rng.uniform(250e2, 1000e2, n)
    RH = rng.uniform(0.4, 1.3, n)
    pvs = plain.saturation_vapour_pressure.pvs_water(T)
    pv = RH * pvs
    qv = const.eps * pv / (p - pv)
    a_w_ice, RH_ice = S.from_ndarray(np.zeros(n)), S.from_ndarray(np.zeros(n))
    backend.a_w_ice(T=S.from_ndarray(T), p=S.from_ndarray(p), RH=S.from_ndarray(RH),
                    water_vapour_mixing_ratio=S.from_ndarray(qv), a_w_ice=a_w_ice,
                    RH_ice=RH_ice)
    arrays.update({"a_w_ice/T": T, "a_w_ice/p": p, "a_w_ice/RH": RH, "a_w_ice/qv": qv,
                   "a_w_ice/out_a_w_ice": a_w_ice.to_ndarray(),
                   "a_w_ice/out_RH_ice": RH_ice.to_ndarray()})

    # the MixedPhaseSpheres conversions
    conv_mass = np.concatenate([mass[:60], [0.0, -0.0, 1e-300, -1e-300]])
    out_volume = S.from_ndarray(np.zeros_like(conv_mass))
    backend.volume_of_water_mass(out_volume, S.from_ndarray(conv_mass))
    out_mass = S.from_ndarray(np.zeros_like(conv_mass))
    backend.mass_of_water_volume(out_mass, out_volume)
    arrays.update({"conversion/mass": conv_mass, "conversion/out_volume": out_volume.to_ndarray(),
                   "conversion/out_mass": out_mass.to_ndarray()})
    save("frz_methods", **arrays)


# ---- frz_box_* -----------------------------------------------------------------------------------
BOX_N_SD, BOX_STEPS, BOX_DT = 256, 20, 1.0


def _tallied(backend, formulae, tally, dt):
    """the stochastic methods of `backend` wrapped so that every call is tallied first"""
    inner_td, inner_hom = backend.freeze_time_dependent, backend.freeze_time_dependent_homogeneous

    def host(storage):
        return np.array(storage.data, copy=True)

    def time_dependent(**kw):
        att = kw["attributes"]
        tally.time_dependent(formulae, rand=host(kw["rand"]), mass=host(att.signed_water_mass),
                             area=host(att.immersed_surface_area), dt=dt, cell=host(kw["cell"]),
                             a_w_ice=host(kw["a_w_ice"]), T=host(kw["temperature"]),
                             RH=host(kw["relative_humidity"]), thaw=kw["thaw"])
        inner_td(**kw)

    def homogeneous(**kw):
        att = kw["attributes"]
        tally.homogeneous(formulae, rand=host(kw["rand"]), mass=host(att.signed_water_mass),
                          volume=host(att.volume), dt=dt, cell=host(kw["cell"]),
                          a_w_ice=host(kw["a_w_ice"]), T=host(kw["temperature"]),
                          RH_ice=host(kw["relative_humidity_ice"]), thaw=kw["thaw"])
        inner_hom(**kw)

    backend.freeze_time_dependent = time_dependent
    backend.freeze_time_dependent_homogeneous = homogeneous


def box(name, seed, *, het="Null", hom="Null", freezing, ramp, extra_attributes):
    rng = np.random.default_rng(seed)
    formulae = formulae_for(het=het, hom=hom, seed=seed)
    const = formulae.constants
    backend = CPU(formulae)
    tally = Tally()
    _tallied(backend, formulae, tally, BOX_DT)
    builder = Builder(n_sd=BOX_N_SD, backend=backend,
                      environment=Box(dt=BOX_DT, dv=1 * si.m ** 3))
    builder.add_dynamic(Freezing(**freezing))
    radius = np.exp(rng.uniform(np.log(0.5e-6), np.log(25e-6), BOX_N_SD))
    attributes = {"multiplicity": rng.integers(1, 10 ** 6, BOX_N_SD).astype(np.int64),
                  "signed water mass": const.rho_w * const.PI_4_3 * radius ** 3}
    attributes.update(extra_attributes(rng))
    particulator = builder.build(attributes={k: v.copy() for k, v in attributes.items()},
                                 products=())
    masses = []
    for step in range(BOX_STEPS):
        for key, values in ramp.items():
            particulator.environment[key] = values[step]
        particulator.run(steps=1)
        masses.append(particulator.attributes["signed water mass"].to_ndarray(raw=True).copy())
    masses = np.stack(masses)
    if freezing["singular"]:
        n_frozen = int((masses < 0).any(axis=0).sum())
        print(f"{name}: {n_frozen} of {BOX_N_SD} freeze during the run")
        if not 0.1 <= n_frozen / BOX_N_SD <= 0.9:
            raise Retry(name)
    else:
        tally.check(name)
    arrays = {f"init/{k}": v for k, v in attributes.items()}
    arrays.update({f"ramp/{k}": np.asarray(v, dtype=float) for k, v in ramp.items()})
    arrays.update({f"freezing/{k}": np.asarray(int(v)) for k, v in freezing.items()})
    arrays.update({f"constants/{k}": np.asarray(float(v))
                   for k, v in {**HET.get(het, {}), **HOM.get(hom, {})}.items()})
    arrays.update(het=np.asarray(het), hom=np.asarray(hom), seed=np.asarray(seed),
                  dt=np.asarray(BOX_DT), n_steps=np.asarray(BOX_STEPS), masses=masses)
    assert (np.sign(masses[1:]) != np.sign(masses[:-1])).any()
    save(name, **arrays)
    return masses


def _retrying(function, first_seed):
    for seed in range(first_seed, first_seed + 50):
        try:
            return function(seed)
        except Retry as refused:
            print(f"seed {seed} refused: {refused}")
    raise RuntimeError("no seed satisfies the generator's conditions")


def boxes():
    steps = np.arange(BOX_STEPS)
    # singular: freezing temperatures straddle the ramp (the last step warms: thaw)
    T = 262.0 - 1.5 * steps
    RH = np.full(BOX_STEPS, 1.01)
    RH[3] = 0.99  # a subsaturated step: nothing freezes
    T_sing = T.copy()
    T_sing[-1] = 274.0
    _retrying(lambda seed: box(
        "frz_box_singular", seed, freezing=dict(singular=True, thaw=True),
        ramp={"T": T_sing, "RH": RH, "a_w_ice": np.full(BOX_STEPS, np.nan),
              "RH_ice": np.full(BOX_STEPS, np.nan)},
        extra_attributes=lambda rng: {"freezing temperature": np.where(
            rng.uniform(size=BOX_N_SD) < 0.1, 0.0, rng.uniform(225.0, 265.0, BOX_N_SD))}), 101)
    # time-dependent ABIFM with thaw and a final warm step
    a_w_ice = 0.90 - 0.012 * steps
    T_abifm = T.copy()
    T_abifm[-1] = 275.0
    _retrying(lambda seed: box(
        "frz_box_abifm", seed, het="ABIFM",
        freezing=dict(singular=False, thaw=True, immersion_freezing=True,
                      homogeneous_freezing=False),
        ramp={"T": T_abifm, "RH": RH, "a_w_ice": a_w_ice, "RH_ice": 1 / a_w_ice},
        extra_attributes=lambda rng: {"immersed surface area": np.where(
            rng.uniform(size=BOX_N_SD) < 0.1, 0.0,
            np.exp(rng.uniform(np.log(1e-12), np.log(1e-9), BOX_N_SD)))}), 201)
    # homogeneous (Koop2000) after time-dependent immersion freezing (Constant): two stochastic
    # passes per step; d_a_w_ice climbs through KOOP_MIN to 0.30
    RH_ice = 1.30 + 0.0055 * steps
    a_w = np.full(BOX_STEPS, 0.74)
    _retrying(lambda seed: box(
        "frz_box_hom", seed, het="Constant", hom="Koop2000",
        freezing=dict(singular=False, thaw=False, immersion_freezing=True,
                      homogeneous_freezing=True),
        ramp={"T": 240.0 - 0.4 * steps, "RH": RH, "a_w_ice": a_w, "RH_ice": RH_ice},
        extra_attributes=lambda rng: {"immersed surface area": np.where(
            rng.uniform(size=BOX_N_SD) < 0.1, 0.0,
            np.exp(rng.uniform(np.log(1e-14), np.log(3e-12), BOX_N_SD)))}), 301)


if __name__ == "__main__":
    what = sys.argv[1:] or ["methods", "boxes"]
    if "methods" in what:
        _retrying(methods, 20261017)
    if "boxes" in what:
        boxes()

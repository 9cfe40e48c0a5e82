#!/usr/bin/env python3
"""Times one `Freezing.__call__` (time-dependent immersion freezing + homogeneous freezing + thaw
+ the recording of freezing temperatures; ABIFM and Koop2000 rates) on the GPU, at 2^20 and 2^22
super-droplets in one cell and in 32 x 32 cells:

  fused        one `sdm_freezing_step` (rates obtained as the library chooses)
  per_droplet  the same with the nucleation rates evaluated for every eligible super-droplet
  per_cell     the same with the rates evaluated once per cell and workgroup into LDS
  stages       the stage route on the same library: `sdm_pcg64_uniform` + the stage symbol, twice,
               then `sdm_record_freezing_temperatures` (five launches)

Every variant starts each repetition from the same state (the masses are restored outside the
timed window, so a repetition does not run on an all-frozen population), the variants alternate
within a repetition, and the time of a variant is the median over --reps device-event windows of
--calls calls each.  Prints one JSON line per shape; a measurement, not a test: no threshold.

Effective GB/s is the algorithm's traffic over the time: per super-droplet the fused step reads
mass, surface area, cell id and the recorded temperature (the volume is taken from the mass) and
writes only the rows that change: 32 B + 8 B per changed value; the stage route reads and writes
the uniforms (2 x 16 B), reads mass, area or volume and cell id per pass (2 x 24 B) and mass,
cell id and the record in the recording pass (24 B): 104 B + the same writes.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def state(n_sd, n_cell, seed=1):
    rng = np.random.default_rng(seed)
    radius = np.exp(rng.uniform(np.log(0.5e-6), np.log(25e-6), n_sd))
    mass = 1000.0 * 4 / 3 * np.pi * radius ** 3
    mass[rng.uniform(size=n_sd) < 0.2] *= -0.9168  # some ice to start with
    area = np.exp(rng.uniform(np.log(1e-12), np.log(1e-9), n_sd))
    # a cooling column: the lowest cells above T0 (thaw), the rest saturated, a_w_ice falling to
    # where d_a_w_ice has entered Koop's range; the rates stay small enough that most droplets
    # remain liquid - and are evaluated - in every call of a window, as in a run's steady state
    level = np.linspace(0.0, 0.75, n_cell) if n_cell > 1 else np.array([0.712])
    T = 276.0 - 44.0 * level
    a_w_ice = np.minimum(1.0, 0.98 - 0.33 * level)
    return dict(signed_water_mass=mass, immersed_surface_area=area,
                cell=rng.integers(0, n_cell, n_sd).astype(np.int64),
                temperature_of_last_freezing=np.where(mass < 0, 240.0, np.nan),
                T=T, RH=np.full(n_cell, 1.02), a_w_ice=a_w_ice, RH_ice=1.0 / a_w_ice + 0.02)


def main():  # pylint: disable=too-many-locals,too-many-statements
    parser = argparse.ArgumentParser()
    parser.add_argument("--log2-n", type=int, nargs="+", default=[20, 22])
    parser.add_argument("--cells", type=int, nargs="+", default=[1, 1024])
    parser.add_argument("--reps", type=int, default=21)
    parser.add_argument("--calls", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()

    import torch  # pylint: disable=import-outside-toplevel

    from pysdm_amd import freezing as frz  # pylint: disable=import-outside-toplevel
    from pysdm_amd.abi import pcg64_state_inc  # pylint: disable=import-outside-toplevel
    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel
    from pysdm_amd.formulae import Formulae  # pylint: disable=import-outside-toplevel

    eng = HipEngine.get()
    formulae = Formulae(particle_shape_and_density="MixedPhaseSpheres",
                        heterogeneous_ice_nucleation_rate="ABIFM",
                        homogeneous_ice_nucleation_rate="Koop2000",
                        constants={"ABIFM_M": 54.48, "ABIFM_C": -10.67}, seed=44)
    consts = frz.constants_of(formulae)
    state_inc = pcg64_state_inc(formulae.seed)
    dt = 1.0
    for log2_n in args.log2_n:
        for n_cell in args.cells:
            n = 2 ** log2_n
            host = state(n, n_cell)
            dev = {k: eng.upload(v) for k, v in host.items()}
            mass0, last0 = dev["signed_water_mass"].clone(), \
                dev["temperature_of_last_freezing"].clone()
            volume, rand = eng.empty(n, np.float64), eng.empty(n, np.float64)
            eng.call_freezing("sdm_volume_of_signed_water_mass", volume, mass0, n, consts)
            m, last = dev["signed_water_mass"], dev["temperature_of_last_freezing"]
            env = [dev[k] for k in ("T", "RH", "a_w_ice", "RH_ice")]

            def fused(rates, offset, m=m, last=last, dev=dev, env=env, n=n, n_cell=n_cell):
                setup = frz.FreezingSetup(singular=False, homogeneous_freezing=True, thaw=True,
                                          record_freezing_temperature=True, rates=rates)
                cfg = frz.freezing_cfg(setup, formulae, dt, formulae.seed)

                def call():
                    eng.call_freezing("sdm_freezing_step", cfg, offset, n, n_cell, m, None,
                                      dev["immersed_surface_area"], None, dev["cell"], last,
                                      *env, consts)
                return call

            def stages(offset, m=m, last=last, dev=dev, env=env, n=n, volume=volume, rand=rand):
                T, RH, a_w_ice, RH_ice = env

                def call():
                    eng.call("sdm_pcg64_uniform", rand, n, state_inc, offset)
                    eng.call_freezing("sdm_freeze_time_dependent", rand, m,
                                      dev["immersed_surface_area"], dt, dev["cell"], a_w_ice, T,
                                      RH, n, 1, frz.j_het_code(formulae), consts)
                    eng.call("sdm_pcg64_uniform", rand, n, state_inc, offset + n)
                    eng.call_freezing("sdm_freeze_time_dependent_homogeneous", rand, m, volume,
                                      dt, dev["cell"], a_w_ice, T, RH_ice, n, 1,
                                      frz.j_hom_code(formulae), consts)
                    eng.call_freezing("sdm_record_freezing_temperatures", last, dev["cell"], T,
                                      m, n)
                return call

            variants = {"fused": fused("auto", 0), "per_droplet": fused("per_droplet", 0),
                        "stages": stages(0)}
            if n_cell <= 1024:
                variants["per_cell"] = fused("per_cell", 0)
            times = {name: [] for name in variants}
            changed = {}
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for rep in range(args.warmup + args.reps):
                for name, call in variants.items():
                    # every window starts from the same state: call 1 does the freezing, the
                    # calls after it stream over a population that hardly changes any more
                    m.copy_(mass0)
                    last.copy_(last0)
                    torch.cuda.synchronize()
                    begin.record()
                    for _ in range(args.calls):
                        call()
                    end.record()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        times[name].append(begin.elapsed_time(end) / args.calls)
                    changed[name] = int((m != mass0).sum().item())
            result = {"n_sd": n, "n_cell": n_cell, "reps": args.reps,
                      "calls_per_window": args.calls, "changed_rows": changed}
            bytes_per_call = {"stages": 104.0 * n}
            for name, samples in times.items():
                ms = float(np.median(samples))
                traffic = bytes_per_call.get(name, 32.0 * n)
                result[name] = {"ms_per_call": round(ms, 5),
                                "ms_min": round(float(np.min(samples)), 5),
                                "ms_max": round(float(np.max(samples)), 5),
                                "effective_GB_per_s": round(traffic / ms / 1e6, 1)}
            result["stages_over_fused"] = round(
                result["stages"]["ms_per_call"] / result["fused"]["ms_per_call"], 3)
            print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

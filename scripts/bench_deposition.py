#!/usr/bin/env python3
"""Times one `sdm_deposition` call (PySDM's `VapourDepositionOnIce`, default formulae) on the GPU
in both sum modes, at 2^20 and 2^22 rows, in 1 and 1024 cells, with 10 % and 100 % of the rows ice:

  ordered  SDM_DEP_SUM_ORDERED: per cell the contributions are added one by one in row order (the
           reference's bits); with one cell that is one serial chain over every ice row
  blocked  SDM_DEP_SUM_BLOCKED: blocks of 256 contributions reduced in a fixed tree, one workgroup
           each, then the block values added in order

Every window starts from the same masses and predicted columns (restored outside the timed
window), the two variants alternate within a repetition, and the time of a variant is the median
over --reps device-event windows of --calls calls each.  Prints one JSON line per shape (and
appends it to --out); a measurement, not a test: no threshold.

Effective GB/s is the algorithm's traffic over the time: every row's mass, multiplicity and cell
id are read (24 B) and the mass of every ice row is written (8 B); the per-cell columns are
negligible.  What this implementation moves on top of that (sort keys, the identity permutation
and its sorted copy, two contributions per ice row) is not counted.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def state(n_sd, n_cell, ice_fraction, seed=1):
    rng = np.random.default_rng(seed)
    mass = np.exp(rng.uniform(np.log(1e-13), np.log(1e-9), n_sd))
    ice = rng.uniform(size=n_sd) < ice_fraction
    mass[ice] *= -1
    T = np.linspace(238.0, 266.0, n_cell) if n_cell > 1 else np.array([250.0])
    p = np.linspace(45e3, 85e3, n_cell) if n_cell > 1 else np.array([60e3])
    a_w_ice = np.linspace(0.72, 0.94, n_cell) if n_cell > 1 else np.array([0.8])
    s_ice = 1.0 + 0.1 * np.cos(np.arange(n_cell))  # growth and sublimation
    return dict(multiplicity=rng.integers(1, 1000, n_sd).astype(np.int64),
                signed_water_mass=mass, cell_id=rng.integers(0, n_cell, n_sd).astype(np.int64),
                T=T, p=p, RH=a_w_ice * s_ice, a_w_ice=a_w_ice, qv=np.full(n_cell, 1e-3),
                rhod=p / 287.0 / T, thd=T * (1e5 / p) ** 0.2856), int(ice.sum())


def main():  # pylint: disable=too-many-locals
    parser = argparse.ArgumentParser()
    parser.add_argument("--log2-n", type=int, nargs="+", default=[20, 22])
    parser.add_argument("--cells", type=int, nargs="+", default=[1, 1024])
    parser.add_argument("--ice", type=float, nargs="+", default=[0.1, 1.0])
    parser.add_argument("--reps", type=int, default=11)
    parser.add_argument("--calls", type=int, default=3)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = parser.parse_args()

    import torch  # pylint: disable=import-outside-toplevel

    from pysdm_amd import deposition as dep  # pylint: disable=import-outside-toplevel
    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel
    from pysdm_amd.formulae import Formulae  # pylint: disable=import-outside-toplevel

    eng = HipEngine.get()
    formulae = Formulae(particle_shape_and_density="MixedPhaseSpheres")
    consts = dep.constants_of(formulae)
    dt, dv = 1e-3, 1.0
    for log2_n in args.log2_n:
        for n_cell in args.cells:
            for ice_fraction in args.ice:
                n = 2 ** log2_n
                host, n_ice = state(n, n_cell, ice_fraction)
                dev = {k: eng.upload(v) for k, v in host.items()}
                mass0 = dev["signed_water_mass"].clone()
                pqv, pthd = dev["qv"].clone(), dev["thd"].clone()
                count = eng.zeros(1, np.int64)

                def variant(sum_mode, dev=dev, pqv=pqv, pthd=pthd, count=count, n=n,
                            n_cell=n_cell):
                    cfg = dep.deposition_cfg(formulae, dt, dv, sum_mode)

                    def call():
                        eng.call_deposition(
                            "sdm_deposition", cfg, n, n_cell, dev["multiplicity"],
                            dev["signed_water_mass"], dev["cell_id"], dev["T"], dev["p"],
                            dev["RH"], dev["a_w_ice"], dev["qv"], dev["rhod"], dev["thd"], pqv,
                            pthd, count, consts)
                    return call

                variants = {"ordered": variant("ordered"), "blocked": variant("blocked")}
                times = {name: [] for name in variants}
                begin = torch.cuda.Event(enable_timing=True)
                end = torch.cuda.Event(enable_timing=True)
                for rep in range(args.warmup + args.reps):
                    for name, call in variants.items():
                        dev["signed_water_mass"].copy_(mass0)
                        pqv.copy_(dev["qv"])
                        pthd.copy_(dev["thd"])
                        torch.cuda.synchronize()
                        begin.record()
                        for _ in range(args.calls):
                            call()
                        end.record()
                        torch.cuda.synchronize()
                        if rep >= args.warmup:
                            times[name].append(begin.elapsed_time(end) / args.calls)
                traffic = 24.0 * n + 8.0 * n_ice
                result = {"n_sd": n, "n_cell": n_cell, "ice_fraction": ice_fraction,
                          "n_ice": n_ice, "reps": args.reps, "calls_per_window": args.calls,
                          "algorithmic_bytes_per_row": round(traffic / n, 2),
                          "n_exceeded": int(count.item())}
                for name, samples in times.items():
                    ms = float(np.median(samples))
                    result[name] = {"ms_per_call": round(ms, 5),
                                    "ms_min": round(float(np.min(samples)), 5),
                                    "ms_max": round(float(np.max(samples)), 5),
                                    "effective_GB_per_s": round(traffic / ms / 1e6, 1)}
                result["ordered_over_blocked"] = round(
                    result["ordered"]["ms_per_call"] / result["blocked"]["ms_per_call"], 3)
                line = json.dumps(result)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a", encoding="utf-8") as out:
                        out.write(line + "\n")


if __name__ == "__main__":
    main()

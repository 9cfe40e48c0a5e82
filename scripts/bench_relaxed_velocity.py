#!/usr/bin/env python3
"""Times one `RelaxedVelocity.__call__` on the GPU at 2^20 and 2^22 slots (radii log-uniform over
1 um .. 5 mm, the momentum at half of its terminal value, c = 8, tau = c sqrt(r)).

  fused_table   one `sdm_relaxed_velocity_step` with the Gunn-Kinzer table and the velocity column:
                the count of radii above the table top, then the relaxation kernel
  fused_ry      the same with Rogers-Yau: the relaxation kernel alone
  fused_no_u    the table again, without the velocity column (what `fuse(RelaxedVelocity)` issues)
  runner_fused  `RelaxedVelocityRunner(route="fused").step`: fused_table plus the read of the
                status word, a synchronisation per step, as the host API and the plug-in pay it
  stages        `RelaxedVelocityRunner(route="stages")`: the reference's sequence, one launch per
                Storage operation, with the range check of the table (a reduction and a read-back)

Timed with HIP events on the stream around one call, the momentum restored outside the timed
window, the variants alternating within a repetition; a variant's time is the median over --reps
calls.  The algorithmic traffic of the relaxation kernel is 32 bytes a slot (24 without the
velocity column); the table variants read the mass column once more.  Appends one JSON line per
size to profiles/relaxed_velocity_fused_vs_stages.jsonl and prints it; a measurement, not a test:
no threshold.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "relaxed_velocity_fused_vs_stages.jsonl")


def measure(log2_n, reps, warmup):  # pylint: disable=too-many-locals
    import torch  # pylint: disable=import-outside-toplevel

    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel
    from pysdm_amd.population import MOMENTUM_ROW, Population  # pylint: disable=import-outside-toplevel
    from pysdm_amd.relaxed_velocity import (RelaxedVelocityRunner,  # pylint: disable=import-outside-toplevel
                                            init_fall_momenta)

    eng = HipEngine.get()
    n = 2 ** log2_n
    rng = np.random.default_rng(1)
    radius = np.exp(rng.uniform(np.log(1e-6), np.log(5e-3), n))
    mass = 1000.0 * (4 / 3 * np.pi) * radius ** 3
    start = 0.5 * init_fall_momenta(eng, mass)
    population = Population(eng, multiplicity=np.ones(n, dtype=np.int64), mass=mass,
                            more_extensive={MOMENTUM_ROW: start}, velocity_source="momentum")
    momentum0 = population.momentum.clone()
    table = RelaxedVelocityRunner(population, c=8, dt=1.0, route="fused")
    rogers = RelaxedVelocityRunner(population, c=8, dt=1.0, route="fused",
                                   terminal_velocity="RogersYau")
    stages = RelaxedVelocityRunner(population, c=8, dt=1.0, route="stages")
    velocity = eng.empty(n, np.float64)
    status = eng.zeros(2, np.int64)

    def symbol(runner, with_velocity):
        law = runner.law
        eng.relaxed_velocity_call(
            "sdm_relaxed_velocity_step", runner.cfg(), population.mass, population.momentum,
            velocity if with_velocity else None, getattr(law, "a", None), getattr(law, "b", None),
            status)

    variants = {"fused_table": lambda: symbol(table, True),
                "fused_ry": lambda: symbol(rogers, True),
                "fused_no_u": lambda: symbol(table, False),
                "runner_fused": table.step,
                "stages": stages.step}
    times = {name: [] for name in variants}
    for rep in range(warmup + reps):
        for name, call in variants.items():
            population.momentum.copy_(momentum0)
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            begin.record()
            call()
            end.record()
            end.synchronize()
            if rep >= warmup:
                times[name].append(begin.elapsed_time(end))
    assert int(eng.download(status)[0]) == 0
    result = {"n_sd": n, "reps": reps}
    for name, samples in times.items():
        result[name] = {"ms_median": round(float(np.median(samples)), 5),
                        "ms_min": round(float(np.min(samples)), 5),
                        "ms_p10": round(float(np.percentile(samples, 10)), 5),
                        "ms_p90": round(float(np.percentile(samples, 90)), 5)}
    result["GB_per_s_fused_ry_at_32_bytes"] = round(
        32.0 * n / result["fused_ry"]["ms_median"] / 1e6, 1)
    result["GB_per_s_fused_table_at_40_bytes"] = round(
        40.0 * n / result["fused_table"]["ms_median"] / 1e6, 1)
    result["stages_over_fused_table"] = round(
        result["stages"]["ms_median"] / result["fused_table"]["ms_median"], 2)
    result["stages_over_runner_fused"] = round(
        result["stages"]["ms_median"] / result["runner_fused"]["ms_median"], 2)
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--log2-n", type=int, nargs="+", default=[20, 22])
    parser.add_argument("--reps", type=int, default=51)
    parser.add_argument("--warmup", type=int, default=5)
    parser.add_argument("--out", default=OUT)
    args = parser.parse_args()
    for log2_n in args.log2_n:
        line = json.dumps(measure(log2_n, args.reps, args.warmup))
        print(line, flush=True)
        with open(args.out, "a", encoding="utf-8") as out:
            out.write(line + "\n")


if __name__ == "__main__":
    main()

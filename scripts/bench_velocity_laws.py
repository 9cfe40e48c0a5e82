#!/usr/bin/env python3
"""Times the fused collision step under the three fall-velocity laws on the GPU: the `kinematic2d`
configuration (32 x 32 cells, Geometric kernel, adaptive, optimized_random) at 2^22 super-droplets.

  fused     `CollisionRunner(route="fused").run(steps)` per law.  A repetition builds the boxes anew
            from the same initial state, runs --lead untimed time steps and times the --steps after
            them between two synchronisations (host clock); the laws alternate within a repetition.
            So the repetitions of a law time the same time steps.  The laws themselves are
            different physics on different trajectories and take different numbers of sub-steps:
            the time per SUB-STEP is reported beside the time per step, and the ratio to
            Gunn-Kinzer for both - a cost of the law AND of the state it leads to.
  stages    `route="chain"`, one launch per Storage operation, for the same step at --stage-n-sd
            (2^16 by default: a size it finishes in seconds), with the fused step at that size.

Prints one JSON line; with --out FILE also files it as "law_costs" in that JSON document (the
figures of profiles/velocity_laws_bench.json were taken so).  A measurement, not a test: no threshold.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAWS = ("GunnKinzer1949", "RogersYau", "PowerSeries")


def timed(engine, make_boxes, lead, steps, reps, warmup):
    """per law: (ms per step, sub-steps per step, ms per sub-step), medians over `reps`.  Every
    repetition starts from fresh boxes - the same initial state and seed - runs `lead` untimed time
    steps and times the `steps` after them: each repetition of a law times the SAME time steps of the
    same trajectory, so the spread over the repetitions is the machine's, not the state's"""
    laws = list(make_boxes())
    per_step = {law: [] for law in laws}
    per_sub = {law: [] for law in laws}
    subs = {law: [] for law in laws}
    for rep in range(warmup + reps):
        for law, runner in make_boxes().items():
            runner.run(lead)
            before = runner.sub_steps_done
            engine.synchronize()
            begin = time.perf_counter()
            runner.run(steps)
            engine.synchronize()
            ms = (time.perf_counter() - begin) * 1e3
            if rep >= warmup:
                done = runner.sub_steps_done - before
                per_step[law].append(ms / steps)
                per_sub[law].append(ms / max(done, 1))
                subs[law].append(done / steps)
    return {law: {"ms_per_step": float(np.median(per_step[law])),
                  "ms_per_step_min_max": [float(min(per_step[law])), float(max(per_step[law]))],
                  "substeps_per_step": float(np.median(subs[law])),
                  "ms_per_substep": float(np.median(per_sub[law]))} for law in laws}


def with_ratios(rows):
    base = rows["GunnKinzer1949"]
    for row in rows.values():
        row["step_ratio_to_gunn_kinzer"] = row["ms_per_step"] / base["ms_per_step"]
        row["substep_ratio_to_gunn_kinzer"] = row["ms_per_substep"] / base["ms_per_substep"]
    return rows


def main():
    from pysdm_amd.cases import make_box  # pylint: disable=import-outside-toplevel
    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel

    parser = argparse.ArgumentParser(description=__doc__.split("\n", maxsplit=1)[0])
    parser.add_argument("--n-sd", type=int, default=2**22)
    parser.add_argument("--stage-n-sd", type=int, default=2**16)
    parser.add_argument("--lead", type=int, default=5)
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=1)
    parser.add_argument("--laws", nargs="*", default=list(LAWS))
    parser.add_argument("--no-stages", action="store_true")
    parser.add_argument("--out", default="", help="JSON document to update (default: none)")
    args = parser.parse_args()
    engine = HipEngine.get()
    warnings.simplefilter("ignore")

    def boxes(n_sd, route, grid=None):
        return {law: make_box(engine, "kinematic2d", n_sd=n_sd, route=route, grid=grid,
                              terminal_velocity=law) for law in args.laws}

    result = {"what": "fused collision step per fall-velocity law", "workload": "kinematic2d",
              "n_sd": args.n_sd, "untimed_lead_steps": args.lead,
              "steps_per_repetition": args.steps, "repetitions": args.reps,
              "fused": with_ratios(timed(engine, lambda: boxes(args.n_sd, "fused"), args.lead,
                                         args.steps, args.reps, args.warmup))}
    if not args.no_stages:
        # the same 4096 per cell on a smaller grid
        side = max(1, int(round((args.stage_n_sd / 4096) ** 0.5)))
        result["stages"] = {
            "n_sd": args.stage_n_sd, "grid": [side, side], "steps_per_repetition": 2,
            "chain": with_ratios(timed(
                engine, lambda: boxes(args.stage_n_sd, "chain", (side, side)), 1, 2, 3, 1)),
            "fused": with_ratios(timed(
                engine, lambda: boxes(args.stage_n_sd, "fused", (side, side)), 1, 2, 3, 1))}
    line = json.dumps(result)
    print(line)
    if args.out:
        document = {}
        if os.path.exists(args.out):
            with open(args.out, encoding="utf-8") as old:
                document = json.load(old)
        document["law_costs"] = result
        with open(args.out, "w", encoding="utf-8") as out:
            json.dump(document, out, indent=1)
            out.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times one injecting `Seeding.__call__` on the GPU: 2^20 slots of which a quarter are free
(scattered), K = 1024 super-droplets injected from a reservoir of 4096 seeds, one attribute row.

  fused   one `sdm_seeding_step` (shuffle of the seed index, injection, identity, compaction)
  stages  the stage route on the same library, as `SeedingRunner(route="stages")` issues it:
          `sdm_pcg64_uniform`, `sdm_shuffle_global`, `sdm_seeding` and the read of its status,
          `sdm_identity_index`, `sdm_remove_zero_n_or_flagged`
  pair    `sdm_identity_index` + `sdm_remove_zero_n_or_flagged` alone on the same state: what
          every injection has to be followed by, with or without this path

The figure that matters is fused - pair: what the injection itself adds; it should be of the
order of one streaming read of the multiplicity column (8 * n_sd bytes).  Every call ends with
the synchronisation the compaction has anyway, so a call is timed on the host clock, from a
synchronised device to the call's return; the state (multiplicity, attribute rows, permutation,
seed index) is restored outside the timed window, the variants alternate within a repetition, and
a variant's time is the median over --reps calls.  Prints one JSON line; a measurement, not a
test: no threshold.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():  # pylint: disable=too-many-locals,too-many-statements
    parser = argparse.ArgumentParser()
    parser.add_argument("--log2-n", type=int, default=20)
    parser.add_argument("--inject", type=int, default=1024)
    parser.add_argument("--reservoir", type=int, default=4096)
    parser.add_argument("--rows", type=int, default=1)
    parser.add_argument("--free", type=float, default=0.25, help="fraction of free slots")
    parser.add_argument("--reps", type=int, default=51)
    parser.add_argument("--warmup", type=int, default=5)
    args = parser.parse_args()

    import torch  # pylint: disable=import-outside-toplevel

    from pysdm_amd.abi import pcg64_state_inc  # pylint: disable=import-outside-toplevel
    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel

    eng = HipEngine.get()
    n, k, n_seeds, rows = 2 ** args.log2_n, args.inject, args.reservoir, args.rows
    rng = np.random.default_rng(1)
    free = rng.uniform(size=n) < args.free
    multiplicity0 = eng.upload(np.where(free, 0, rng.integers(1, 10 ** 6, n)).astype(np.int64))
    attributes0 = eng.upload(rng.uniform(1e-15, 1e-12, (rows, n)))
    idx0 = eng.upload(rng.permutation(n).astype(np.int64))
    index0 = eng.upload(np.arange(n_seeds, dtype=np.int64))
    seed_multiplicity = eng.upload(rng.integers(1, 10 ** 6, n_seeds).astype(np.int64))
    seed_attributes = eng.upload(rng.uniform(1e-18, 1e-16, (rows, n_seeds)))
    multiplicity, attributes, idx, index = (x.clone() for x in (multiplicity0, attributes0,
                                                                 idx0, index0))
    u01 = eng.empty(n_seeds, np.float64)
    status = eng.zeros(4, np.int64)
    state_inc = pcg64_state_inc(44)
    lengths = {}

    def fused():
        new_length = ctypes.c_int64(-1)
        eng.seeding_call("sdm_seeding_step", idx, multiplicity, attributes, rows, n, index,
                         seed_multiplicity, seed_attributes, n_seeds, k, 1, state_inc, 0,
                         new_length)
        lengths["fused"] = int(new_length.value)

    def pair():
        eng.call("sdm_identity_index", idx, n)
        lengths["pair"] = eng.scalar_out("sdm_remove_zero_n_or_flagged", ctypes.c_int64,
                                         multiplicity, idx, n, n)

    def stages():
        eng.call("sdm_pcg64_uniform", u01, n_seeds, state_inc, 0)
        eng.call("sdm_shuffle_global", index, n_seeds, u01)
        eng.seeding_call("sdm_seeding", idx, multiplicity, attributes, rows, n, index,
                         seed_multiplicity, seed_attributes, n_seeds, k, status)
        assert int(eng.download(status)[1]) == k
        eng.call("sdm_identity_index", idx, n)
        lengths["stages"] = eng.scalar_out("sdm_remove_zero_n_or_flagged", ctypes.c_int64,
                                           multiplicity, idx, n, n)

    variants = {"fused": fused, "stages": stages, "pair": pair}
    times = {name: [] for name in variants}
    for rep in range(args.warmup + args.reps):
        for name, call in variants.items():
            for target, source in ((multiplicity, multiplicity0), (attributes, attributes0),
                                   (idx, idx0), (index, index0)):
                target.copy_(source)
            torch.cuda.synchronize()
            begin = time.perf_counter()
            call()
            elapsed = time.perf_counter() - begin
            if rep >= args.warmup:
                times[name].append(1e3 * elapsed)
    live = n - int(free.sum())
    assert lengths == {"fused": live + k, "stages": live + k, "pair": live}, lengths
    result = {"n_sd": n, "free_slots": int(free.sum()), "inject": k, "reservoir": n_seeds,
              "rows": rows, "reps": args.reps}
    for name, samples in times.items():
        result[name] = {"ms_median": round(float(np.median(samples)), 5),
                        "ms_min": round(float(np.min(samples)), 5),
                        "ms_p10": round(float(np.percentile(samples, 10)), 5),
                        "ms_p90": round(float(np.percentile(samples, 90)), 5),
                        "ms_max": round(float(np.max(samples)), 5)}
    added = result["fused"]["ms_median"] - result["pair"]["ms_median"]
    result["fused_minus_pair_ms"] = round(added, 5)
    result["multiplicity_column_GB_per_s_at_that_time"] = (
        round(8.0 * n / added / 1e6, 1) if added > 0 else None)
    result["stages_over_fused"] = round(
        result["stages"]["ms_median"] / result["fused"]["ms_median"], 3)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

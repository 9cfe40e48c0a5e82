#!/usr/bin/env python3
"""Times one `sdm_equilibrate_wet_radii` on the GPU at 2^20 and 2^22 rows, for PySDM's default
formulae (the instantiation with the constant surface tension) and for CompressedFilmRuehl +
KappaKoehler (the general instantiation with the nested search).

The rows are those of the corresponding set of tests/golden/wet_radii.npz, tiled in the golden's
(shuffled) order: early exits, short and long searches mixed within a wave, as a caller's rows
are.  Timed with HIP events on the stream around one `wet_radii_call` (the outputs taken from
torch's caching allocator, the status kernel and the search kernel), inputs resident, a warm-up
first; the time of a variant is the median over --reps calls.  The work is compute-bound and
divergent, so the figures are rows/s and the mean iteration count, not a bandwidth.  Writes
profiles/wet_radii_timing_<variant>.json and prints it; a measurement, not a test: no threshold.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = {"default": "Constant_KappaKoehlerLeadingTerms",
            "ruehl_kappa_koehler": "CompressedFilmRuehl_KappaKoehler"}


def measure(variant, log2_n, reps, warmup):  # pylint: disable=too-many-locals
    import torch  # pylint: disable=import-outside-toplevel

    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel
    from pysdm_amd.initialisation import wet_radii_call  # pylint: disable=import-outside-toplevel
    from tests import wet_radii_cases as wc  # pylint: disable=import-outside-toplevel
    from tests.condensation_cases import gold  # pylint: disable=import-outside-toplevel

    eng = HipEngine.get()
    data = gold("wet_radii")
    name = VARIANTS[variant]
    rows, formulae = wc.set_arrays(data, name), wc.formulae_of(name)
    n, m = 2 ** log2_n, len(rows["r_dry"])
    i = np.arange(n)
    up = eng.upload
    arrays = dict(r_dry=up(rows["r_dry"][i % m]), f_org=up(rows["f_org"][i % m]),
                  kappa_times_dry_volume=up(rows["kappa_times_dry_volume"][i % m]),
                  cell_id=up(rows["cell_id"][i % m]),
                  T=up(np.array(data["T"])), RH=up(np.array(data["RH"])))
    samples, iters, status = [], None, None
    for rep in range(warmup + reps):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        _, iters, status = wet_radii_call(eng, formulae, **arrays)
        end.record()
        end.synchronize()
        if rep >= warmup:
            samples.append(begin.elapsed_time(end))
    assert [int(w) for w in eng.download(status)] == [0, 0, n, 0]
    iters = eng.download(iters)
    ms = float(np.median(samples))
    return {"variant": variant, "set": name, "n": n, "reps": reps,
            "ms_median": round(ms, 4), "ms_min": round(float(np.min(samples)), 4),
            "ms_p90": round(float(np.percentile(samples, 90)), 4),
            "rows_per_s": round(n / ms * 1e3), "mean_iters": round(float(iters.mean()), 3),
            "mean_iters_of_searched_rows": round(float(iters[iters > 0].mean()), 3),
            "share_of_rows_searched": round(float((iters > 0).mean()), 3)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--log2-n", type=int, nargs="+", default=[20, 22])
    parser.add_argument("--reps", type=int, default=21)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = parser.parse_args()
    for variant in VARIANTS:
        results = [measure(variant, log2_n, args.reps, args.warmup) for log2_n in args.log2_n]
        text = json.dumps({"variant": variant, "results": results}, indent=1)
        print(text, flush=True)
        path = os.path.join(args.out_dir, f"wet_radii_timing_{variant}.json")
        with open(path, "w", encoding="utf-8") as out:
            out.write(text + "\n")


if __name__ == "__main__":
    main()

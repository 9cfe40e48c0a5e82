#!/usr/bin/env python3
"""Times one `AqueousChemistry.__call__` on the GPU, at 2^20 and 2^22 super-droplets in 1 and in
1024 cells, open and closed system, 1 and 5 sub-steps:

  fused          one `sdm_chemistry_step` (ordered sum where the system is closed), the cell's
                 constants evaluated per row (SDM_CHEM_CONSTS_PER_ROW)
  fused_per_cell the same with the constants evaluated once per cell and workgroup into LDS
                 (SDM_CHEM_CONSTS_PER_CELL; up to 256 cells)
  fused_blocked  the same with the blocked sum (closed system only)
  stages         `ChemistryRunner.step_by_stages()`: the stage symbols over columns in memory,
                 conc = moles / volume by torch (1 + 6 x n_substep library launches, 10 x n_substep
                 torch kernels)

Every variant starts each repetition from the same state (restored outside the timed window), the
variants alternate within a repetition, and the time of a variant is the median over --reps
device-event windows of --calls calls each.  Prints one JSON line per shape; a measurement, not a
test: no threshold.  What SDM_CHEM_CONSTS_AUTO takes (chemistry.hip: SDM_CHEM_AUTO_PER_CELL) is the
faster of fused and fused_per_cell in the recorded lines.

Algorithmic bytes per row and step.  Fused, open system: 7 amounts, pH, volume, cell id and
multiplicity read (88 B) and the flag (1 B); 7 amounts, pH and the flag written (65 B): 154 B
whatever n_substep is.  Fused, closed system: that per sub-step (the row kernel runs once per
sub-step) plus 6 differences and a marker written and read again and the index read by the sum:
154 + 106 = 260 B per sub-step.  Stage route, per sub-step: two passes of conc (5 amounts and the
volume read, 5 conc written: 88 B), equilibrate_H (5 conc, cell id, pH read; pH and flag written:
65 B) and drop data (pH, cell id read, 6 factors written: 64 B), one dissolution (index, flag, 6
amounts, 6 factors, volume, multiplicity read, 6 amounts written: ~170 B, + 106 B closed) and one
oxidation (~90 B): ~700 B.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def state(n_sd, n_cell, seed=1):
    """ammonium-sulphate-like droplets of 0.5 .. 15 um with traces of the other species; most rows
    stay under the ionic-strength threshold"""
    rng = np.random.default_rng(seed)
    volume = 4 / 3 * np.pi * np.exp(rng.uniform(np.log(5e-7), np.log(1.5e-5), n_sd)) ** 3
    salt = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), n_sd))
    moles = {"S_VI": salt * volume, "N_mIII": 2 * salt * volume * rng.uniform(0.8, 1.0, n_sd)}
    for key in ("S_IV", "O3", "H2O2", "C_IV", "N_V"):
        moles[key] = np.exp(rng.uniform(np.log(1e-6), np.log(1e-3), n_sd)) * volume
    return dict(cell=rng.integers(0, n_cell, n_sd).astype(np.int64), volume=volume, moles=moles,
                multiplicity=rng.integers(100, 10000, n_sd),
                T=np.linspace(278.0, 296.0, n_cell) if n_cell > 1 else np.array([285.0]),
                p=np.full(n_cell, 95e3))


MOLE_FRACTIONS = {"HNO3": 1e-10, "H2O2": 5e-10, "NH3": 1e-10, "SO2": 2e-10, "CO2": 3.6e-4,
                  "O3": 5e-8}


def main():  # pylint: disable=too-many-locals,too-many-statements
    parser = argparse.ArgumentParser()
    parser.add_argument("--log2-n", type=int, nargs="+", default=[20, 22])
    parser.add_argument("--cells", type=int, nargs="+", default=[1, 256, 1024])
    parser.add_argument("--systems", nargs="+", default=["open", "closed"])
    parser.add_argument("--substeps", type=int, nargs="+", default=[1, 5])
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--calls", type=int, default=2)
    parser.add_argument("--warmup", type=int, default=1)
    args = parser.parse_args()

    import torch  # pylint: disable=import-outside-toplevel

    from pysdm_amd import chemistry as chem  # pylint: disable=import-outside-toplevel
    from pysdm_amd.condensation import AmbientColumns  # pylint: disable=import-outside-toplevel
    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel
    from pysdm_amd.formulae import Formulae  # pylint: disable=import-outside-toplevel
    from pysdm_amd.population import Population  # pylint: disable=import-outside-toplevel

    eng = HipEngine.get()
    formulae = Formulae()
    for log2_n in args.log2_n:
        for n_cell in args.cells:
            n = 2 ** log2_n
            host = state(n, n_cell)
            rows = {f"moles_{k}": host["moles"][k] for k in chem.AQUEOUS}
            pop = Population(eng, multiplicity=host["multiplicity"], volume=host["volume"],
                             cell_id=host["cell"], n_cell=n_cell, more_extensive=rows)
            rhod = host["p"] / formulae.constants.Rd / host["T"]
            ambient = AmbientColumns(eng, formulae, rhod=rhod, thd=np.full(n_cell, 300.0),
                                     qv=np.full(n_cell, 1e-3))
            eng.assign(ambient.T, eng.upload(host["T"]))
            eng.assign(ambient.p, eng.upload(host["p"]))
            pop.sorted_cell_start()
            for system in args.systems:
                for n_substep in args.substeps:
                    sums = ("ordered", "blocked") if system == "closed" else ("ordered",)
                    runners = {
                        s: chem.ChemistryRunner(
                            pop, chem.ChemistrySetup(system, n_substep, sum=s,
                                                     constants="per_row"), ambient, dt=1.0,
                            dv=1.0 * n / 2 ** 20, mole_fractions=MOLE_FRACTIONS)
                        for s in sums}
                    if n_cell <= chem.LDS_CELLS:
                        runners["per_cell"] = chem.ChemistryRunner(
                            pop, chem.ChemistrySetup(system, n_substep, constants="per_cell"),
                            ambient, dt=1.0, dv=1.0 * n / 2 ** 20, mole_fractions=MOLE_FRACTIONS)
                    first = runners["ordered"]
                    variants = {"fused": (first, first.step),
                                "stages": (first, first.step_by_stages)}
                    if "per_cell" in runners:
                        variants["fused_per_cell"] = (runners["per_cell"],
                                                      runners["per_cell"].step)
                    if "blocked" in runners:
                        variants["fused_blocked"] = (runners["blocked"], runners["blocked"].step)
                    extensive0 = pop.extensive.clone()
                    ratios0 = [c.clone() for c in first.mixing_ratios]
                    times = {name: [] for name in variants}
                    flagged = {}
                    begin = torch.cuda.Event(enable_timing=True)
                    end = torch.cuda.Event(enable_timing=True)
                    for rep in range(args.warmup + args.reps):
                        for name, (runner, call) in variants.items():
                            pop.extensive.copy_(extensive0)
                            runner.pH.fill_(7.0)
                            runner.do_chemistry_flag.fill_(0)
                            for column, start in zip(runner.mixing_ratios, ratios0):
                                column.copy_(start)
                            torch.cuda.synchronize()
                            begin.record()
                            for _ in range(args.calls):
                                call()
                            end.record()
                            torch.cuda.synchronize()
                            if rep >= args.warmup:
                                times[name].append(begin.elapsed_time(end) / args.calls)
                            flagged[name] = int(runner.do_chemistry_flag.sum().item())
                    # (what the reference would assert on, over all windows: recorded, not fatal)
                    events = {s: [int(c) for c in runner.counts.tolist()]
                              for s, runner in runners.items()}
                    result = {"n_sd": n, "n_cell": n_cell, "system": system,
                              "n_substep": n_substep, "reps": args.reps,
                              "calls_per_window": args.calls, "flagged_rows": flagged,
                              "failed_negative_exceeded": events}
                    fused_bytes = 154.0 if system == "open" else 260.0 * n_substep
                    traffic = {"fused": fused_bytes, "fused_blocked": fused_bytes,
                               "fused_per_cell": fused_bytes,
                               "stages": (700.0 + (106.0 if system == "closed" else 0.0))
                               * n_substep}
                    for name, samples in times.items():
                        ms = float(np.median(samples))
                        result[name] = {
                            "ms_per_call": round(ms, 4), "ms_min": round(float(np.min(samples)), 4),
                            "ms_max": round(float(np.max(samples)), 4),
                            "bytes_per_row": traffic[name],
                            "effective_GB_per_s": round(traffic[name] * n / ms / 1e6, 1)}
                    result["stages_over_fused"] = round(
                        result["stages"]["ms_per_call"] / result["fused"]["ms_per_call"], 3)
                    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

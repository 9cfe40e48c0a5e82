#!/usr/bin/env python3
"""Times `sdm_condensation` (include/sdm_condensation.h) on the GPU: CELLS x CELLS cells of
PER_CELL super-droplets (lognormal aerosol near equilibrium, an ambient state near saturation
with a per-step cooling and moistening as a kinematic step prescribes it), adaptive sub-steps.
Prints one JSON line: ms per time step (HIP events around the call, median over --steps calls)
and the per-cell sub-step counts.

The serial sum's share: run once with the product library and once with the measurement build
`SDM_COND_SERIAL_TWICE` (every serial n * m walk done twice, numerics unchanged):

    bash scripts/build_variant.sh cond_serial2 -DSDM_COND_SERIAL_TWICE
    python scripts/condensation_timing.py
    SDM_HIP_LIB=build_variants/libsdm_cond_serial2.so python scripts/condensation_timing.py

the difference of the two times is the cost of one serial chain per pass.

`--formulae` picks what is timed: `default` (PySDM's default formulae through `sdm_condensation`),
`default-through-general-kernel` (the same formulae through `sdm_condensation_f`: what the
option switches, the staged f_org / Reynolds columns and the larger kernel cost by themselves),
`lowe2019` (organic film of Ovadnevaite, Lowe et al. 2019 kinetics, thermics and latent heat,
August-Roche-Magnus) and `ventilated` (Pruppacher & Rasmussen 1979, Fick, Grabowski et al. 2011
thermics, Murphy & Koop 2005, constant latent heat), on the same state.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMULAE = {
    "default": {},
    "default-through-general-kernel": {},
    "lowe2019": {"surface_tension": "CompressedFilmOvadnevaite",
                 "diffusion_kinetics": "LoweEtAl2019", "diffusion_thermics": "LoweEtAl2019",
                 "latent_heat_vapourisation": "Lowe2019",
                 "saturation_vapour_pressure": "AugustRocheMagnus"},
    "ventilated": {"ventilation": "PruppacherAndRasmussen1979", "drop_growth": "Fick",
                   "diffusion_thermics": "GrabowskiEtAl2011",
                   "saturation_vapour_pressure": "MurphyKoop2005",
                   "latent_heat_vapourisation": "Constant"},
}


def state(cells, per_cell, seed=1):
    from pysdm_amd.physics import constants as k  # pylint: disable=import-outside-toplevel

    rng = np.random.default_rng(seed)
    n_cell, n_sd = cells * cells, cells * cells * per_cell
    cell_id = np.repeat(np.arange(n_cell), per_cell)
    idx = rng.permutation(n_sd).astype(np.int64)
    idx = idx[np.argsort(cell_id[idx], kind="stable")]
    cell_start = np.arange(n_cell + 1, dtype=np.int64) * per_cell
    r_dry = np.exp(rng.normal(np.log(0.04e-6), np.log(1.4), n_sd))
    vdry = k.PI_4_3 * r_dry ** 3
    kappa = np.full(n_sd, 1.28)
    r_wet = r_dry * rng.uniform(1.5, 6, n_sd)
    water_mass = k.rho_w * k.PI_4_3 * r_wet ** 3
    rhod = np.full(n_cell, 1.1) + rng.uniform(-0.01, 0.01, n_cell)
    thd = np.full(n_cell, 290.0) + rng.uniform(-0.5, 0.5, n_cell)
    T = thd * np.power(rhod * thd / k.p1000 * k.Rd, k.Rd_over_c_pd / (1 - k.Rd_over_c_pd))
    qv = np.full(n_cell, 0.01)
    for _ in range(30):  # RH = 0.999: qv from p(qv)
        p = rhod * (1 + qv) * (k.Rv / (1 / qv + 1) + k.Rd / (1 + qv)) * T
        d = T - k.T0
        pvs = k.FWC_C0 + d * (k.FWC_C1 + d * (k.FWC_C2 + d * (k.FWC_C3 + d * (k.FWC_C4 + d * (
            k.FWC_C5 + d * (k.FWC_C6 + d * (k.FWC_C7 + d * k.FWC_C8)))))))
        qv = k.eps * 0.999 * pvs / (p - 0.999 * pvs)
    r_cr = np.sqrt(3 * kappa * (vdry / k.PI_4_3) / (2 * k.sgm_w / k.Rv / T[cell_id] / k.rho_w))
    return dict(n_cell=n_cell, n_sd=n_sd, cell_start=cell_start, idx=idx, vdry=vdry, kappa=kappa,
                water_mass=water_mass, multiplicity=rng.integers(10 ** 6, 10 ** 8, n_sd),
                rhod=rhod, thd=thd, qv=qv, v_cr=k.PI_4_3 * r_cr ** 3,
                air_density=rhod * (1 + qv), eta=np.full(n_cell, 1.8e-5),
                f_org=rng.uniform(0, 1, n_sd), reynolds_number=rng.uniform(0, 1, n_sd) ** 8 * 300)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cells", type=int, default=32)
    parser.add_argument("--per-cell", type=int, default=4096)
    parser.add_argument("--steps", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=1)
    parser.add_argument("--dt", type=float, default=1.0)
    parser.add_argument("--formulae", choices=sorted(FORMULAE), default="default")
    args = parser.parse_args()

    import torch  # pylint: disable=import-outside-toplevel

    from pysdm_amd.condensation import COUNTERS, condensation_call  # pylint: disable=import-outside-toplevel
    from pysdm_amd.engine import HipEngine  # pylint: disable=import-outside-toplevel
    from pysdm_amd.formulae import Formulae  # pylint: disable=import-outside-toplevel

    eng = HipEngine.get()
    s = state(args.cells, args.per_cell)
    up = eng.upload
    d = {k: up(np.asarray(v)) for k, v in s.items() if isinstance(v, np.ndarray)}
    n_cell = s["n_cell"]
    counters = {k: up(np.full(n_cell, -1, dtype=np.int64)) for k in COUNTERS}
    RH_max = up(np.zeros(n_cell))
    success = up(np.zeros(n_cell, dtype=np.uint8))
    pthd, pqv = up(s["thd"]), up(s["qv"])
    cell_order = up(np.arange(n_cell, dtype=np.int64))
    # (a choice `Formulae` refuses travels in an explicit descriptor)
    from pysdm_amd.condensation import descriptor_of  # pylint: disable=import-outside-toplevel
    from pysdm_amd.physics.condensation_formulae import HOST_REFUSED  # pylint: disable=import-outside-toplevel

    choices = FORMULAE[args.formulae]
    formulae = Formulae(constants={"sgm_org": 0.04, "delta_min": 1e-10},
                        **{option: choice for option, choice in choices.items()
                           if choice not in HOST_REFUSED.get(option, ())})
    descriptor = descriptor_of(choices, formulae.constants)
    general = args.formulae == "default-through-general-kernel"
    times, substeps = [], []
    for step in range(args.warmup + args.steps):
        # a kinematic step's prediction: 0.05 K cooling, 0.1 % more vapour
        eng.assign(pthd, d["thd"] - 0.05)
        eng.assign(pqv, d["qv"] * 1.001)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        condensation_call(
            eng, formulae=formulae, n_sd=s["n_sd"], n_cell=n_cell, cell_start=d["cell_start"],
            water_mass=d["water_mass"], v_cr=d["v_cr"], multiplicity=d["multiplicity"],
            vdry=d["vdry"], idx=d["idx"], rhod=d["rhod"], thd=d["thd"],
            water_vapour_mixing_ratio=d["qv"], dv=1.0, prhod=d["rhod"], pthd=pthd,
            predicted_water_vapour_mixing_ratio=pqv, kappa=d["kappa"],
            f_org=d["f_org"], rtol_x=1e-6, rtol_thd=1e-6,
            timestep=args.dt, counters=counters, cell_order=cell_order, RH_max=RH_max,
            success=success, reynolds_number=d["reynolds_number"],
            air_density=d["air_density"],
            air_dynamic_viscosity=d["eta"], dt_range=(1e-4, args.dt), adaptive=True, fuse=32,
            multiplier=2, RH_rtol=1e-7, max_iters=16, general=general,
            descriptor=descriptor)
        stop.record()
        stop.synchronize()
        if not bool(success.all()):
            raise RuntimeError(f"condensation failed in step {step}")
        eng.assign(d["thd"], pthd)
        eng.assign(d["qv"], pqv)
        if step >= args.warmup:
            times.append(start.elapsed_time(stop))
            substeps.append(eng.download(counters["n_substeps"]))
    n = np.stack(substeps)
    print(json.dumps({
        "formulae": args.formulae,
        "library": os.path.basename(os.environ.get("SDM_HIP_LIB") or "libsdm_hip.so"),
        "cells": n_cell, "per_cell": args.per_cell, "n_sd": s["n_sd"], "dt": args.dt,
        "ms_per_step_median": float(np.median(times)), "ms_per_step": [round(t, 3) for t in times],
        "n_substeps_min": int(n.min()), "n_substeps_mean": float(n.mean()),
        "n_substeps_max": int(n.max()),
        "n_substeps_mean_per_step": [round(float(v), 1) for v in n.mean(axis=1)],
    }))


if __name__ == "__main__":
    main()

"""Shared by the condensation tests: replay of the recorded `backend.condensation` calls of
tests/golden/cond_*.npz (gen_condensation_golden.py) through a PySDM-shaped backend class, and
seeded multi-cell cases for HIP / checker parity."""
import os

import numpy as np

from pysdm_amd.condensation import COUNTERS
from pysdm_amd.formulae import Formulae
from pysdm_amd.physics import constants as const

HERE = os.path.dirname(os.path.abspath(__file__))
# Against the reference's goldens: integers exactly; floats within these relative tolerances.
# The reference ran with NumPy's exp / log / power, which are not correctly rounded (NumPy's exp
# differs from a correctly rounded one in ~5 % of arguments); a one-ulp difference inside TOMS748
# moves its iterates anywhere within its own tolerance (rtol_x = 1e-6 on x = ln m, i.e. up to
# ~3e-5 of m at |ln m| ~ 35).  With the same libm on both sides the checker reproduces the
# reference's box calls bit for bit.  HIP and checker agree bit for bit.
GOLDEN_RTOL = {"water_mass": 5e-5, "pthd": 1e-9, "predicted_water_vapour_mixing_ratio": 1e-9,
               "RH_max": 1e-9}
OUT_FLOATS = ("water_mass", "pthd", "predicted_water_vapour_mixing_ratio", "RH_max")
OUT_INTS = (*COUNTERS, "success")


def gold(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def _arg(data, key, call):
    """per-call array if recorded per call, else the run's constant one"""
    per_call = f"calls/{key}"
    return data[per_call][call] if per_call in data.files else data[key]


def solver_of(data):
    if "solver/dt_range" in data.files:  # a recorded Parcel run
        return dict(timestep=float(data["solver/timestep"]),
                    dt_range=tuple(data["solver/dt_range"]),
                    adaptive=bool(data["solver/adaptive"]), fuse=int(data["solver/fuse"]),
                    multiplier=int(data["solver/multiplier"]),
                    RH_rtol=float(data["solver/RH_rtol"]),
                    max_iters=int(data["solver/max_iters"]))
    return dict(timestep=float(data["timestep"]), dt_range=tuple(data["dt_range"]),
                adaptive=None, fuse=int(data["fuse"]), multiplier=int(data["multiplier"]),
                RH_rtol=float(data["RH_rtol"]), max_iters=int(data["max_iters"]))


def replay(backend, data, call):
    """runs recorded call number `call` on `backend` (an instance); returns its outputs"""
    S = backend.Storage
    solver_args = solver_of(data)
    if solver_args["adaptive"] is None:
        solver_args["adaptive"] = bool(data["calls/adaptive"][call])
    timestep = solver_args.pop("timestep")
    n_cell = int(_arg(data, "rhod", call).shape[0])
    solver = backend.make_condensation_solver(timestep, n_cell, **solver_args)
    st = {}
    for key in ("water_mass", "v_cr", "multiplicity", "vdry", "kappa", "f_org", "idx",
                "cell_start_arg", "cell_id", "reynolds_number", "rhod", "thd",
                "water_vapour_mixing_ratio", "prhod", "pthd",
                "predicted_water_vapour_mixing_ratio", "air_density", "air_dynamic_viscosity"):
        st[key] = S.from_ndarray(np.array(_arg(data, key, call)))
    counters = {k: S.from_ndarray(np.array(data[f"calls/in_{k}"][call], dtype=np.int64))
                for k in COUNTERS}
    RH_max = S.from_ndarray(np.full(n_cell, np.nan))
    success = S.from_ndarray(np.zeros(n_cell, dtype=bool))
    dv = float(data["calls/dv"][call]) if "calls/dv" in data.files else float(data["dv"])
    rtol_x = float(data["calls/rtol_x"][call]) if "calls/rtol_x" in data.files \
        else float(data["rtol_x"])
    rtol_thd = float(data["calls/rtol_thd"][call]) if "calls/rtol_thd" in data.files \
        else float(data["rtol_thd"])
    backend.condensation(
        solver=solver, n_cell=n_cell, cell_start_arg=st["cell_start_arg"],
        water_mass=st["water_mass"], multiplicity=st["multiplicity"], vdry=st["vdry"],
        idx=st["idx"], rhod=st["rhod"], thd=st["thd"],
        water_vapour_mixing_ratio=st["water_vapour_mixing_ratio"], dv=dv, prhod=st["prhod"],
        pthd=st["pthd"], predicted_water_vapour_mixing_ratio=st[
            "predicted_water_vapour_mixing_ratio"],
        kappa=st["kappa"], f_org=st["f_org"], rtol_x=rtol_x, rtol_thd=rtol_thd, v_cr=st["v_cr"],
        timestep=timestep, counters=counters, cell_order=data["calls/cell_order"][call],
        RH_max=RH_max, success=success, cell_id=st["cell_id"],
        reynolds_number=st["reynolds_number"], air_density=st["air_density"],
        air_dynamic_viscosity=st["air_dynamic_viscosity"])
    out = {k: counters[k].to_ndarray() for k in COUNTERS}
    out.update(water_mass=st["water_mass"].to_ndarray(), pthd=st["pthd"].to_ndarray(),
               predicted_water_vapour_mixing_ratio=st[
                   "predicted_water_vapour_mixing_ratio"].to_ndarray(),
               RH_max=RH_max.to_ndarray(), success=success.to_ndarray().astype(np.int64))
    return out


def assert_matches_golden(out, data, call):
    for key in OUT_INTS:
        np.testing.assert_array_equal(out[key], data[f"calls/out_{key}"][call],
                                      err_msg=f"call {call}: {key}")
    for key in OUT_FLOATS:
        np.testing.assert_allclose(out[key], data[f"calls/out_{key}"][call], rtol=GOLDEN_RTOL[key],
                                   atol=0, err_msg=f"call {call}: {key}")


# ---- seeded cases for HIP / checker parity --------------------------------------------------------
def seeded_case(seed, counts, *, bad_rows=True, dt=1.0, max_iters=16):
    """a multi-cell state: `counts` super-droplets per cell (0 = empty cell), shuffled
    permutation, ambient state near saturation with prescribed predictions.  `bad_rows` adds
    multiplicity-0 and water-mass <= 0 rows; a small `max_iters` makes bracket searches and
    TOMS748 runs fail in some cells (success == 0 there)."""
    rng = np.random.default_rng(seed)
    formulae = Formulae()
    counts = np.asarray(counts, dtype=np.int64)
    n_cell, n_sd = counts.shape[0], int(counts.sum())
    cell_id = rng.permutation(np.repeat(np.arange(n_cell), counts)).astype(np.int64)
    idx = rng.permutation(n_sd).astype(np.int64)
    idx = idx[np.argsort(cell_id[idx], kind="stable")]
    cell_start = np.zeros(n_cell + 1, dtype=np.int64)
    cell_start[1:] = np.cumsum(counts)
    r_dry = np.exp(rng.uniform(np.log(0.01e-6), np.log(0.5e-6), n_sd))
    vdry = const.PI_4_3 * r_dry ** 3
    kappa = rng.uniform(0.2, 1.3, n_sd)
    multiplicity = rng.integers(1, 10 ** 9, n_sd).astype(np.int64)
    r_wet = r_dry * rng.uniform(1.5, 20, n_sd)
    r_wet[rng.uniform(size=n_sd) < 0.1] *= 50
    water_mass = const.rho_w * const.PI_4_3 * r_wet ** 3
    if bad_rows and n_sd > 8:
        pick = rng.choice(n_sd, 6, replace=False)
        multiplicity[pick[:2]] = 0
        water_mass[pick[2]] = 0.0
        water_mass[pick[3:5]] *= -1
    rhod = rng.uniform(1.0, 1.2, n_cell)
    thd = rng.uniform(285, 300, n_cell)
    k = const
    T = thd * np.power(rhod * thd / k.p1000 * k.Rd, k.Rd_over_c_pd / (1 - k.Rd_over_c_pd))
    target = rng.uniform(0.97, 1.01, n_cell)
    qv = np.full(n_cell, 0.01)
    for _ in range(30):  # fixed point: p depends on qv
        p = rhod * (1 + qv) * (k.Rv / (1 / qv + 1) + k.Rd / (1 + qv)) * T
        d = T - k.T0
        pvs = k.FWC_C0 + d * (k.FWC_C1 + d * (k.FWC_C2 + d * (k.FWC_C3 + d * (k.FWC_C4 + d * (
            k.FWC_C5 + d * (k.FWC_C6 + d * (k.FWC_C7 + d * k.FWC_C8)))))))
        pv = target * pvs
        qv = k.eps * pv / (p - pv)
    scale = 10.0 ** rng.integers(0, 3, n_cell)
    prhod = rhod * (1 + rng.uniform(-2e-4, 0, n_cell))
    pthd = thd + rng.uniform(-0.05, 0.05, n_cell) * scale
    pqv = qv * (1 + rng.uniform(-5e-4, 5e-4, n_cell) * scale)
    air_density = rhod * (1 + qv)
    eta = (k.ZOGRAFOS_1987_COEFF_T3 * T ** 3 + k.ZOGRAFOS_1987_COEFF_T2 * T ** 2
           + k.ZOGRAFOS_1987_COEFF_T1 * T + k.ZOGRAFOS_1987_COEFF_T0)
    r_cr = np.sqrt(3 * kappa * (vdry / k.PI_4_3) / (2 * k.sgm_w / k.Rv / T[cell_id] / k.rho_w))
    v_cr = k.PI_4_3 * r_cr ** 3
    return {
        "formulae": formulae, "n_sd": n_sd, "n_cell": n_cell, "cell_start": cell_start,
        "water_mass": water_mass, "v_cr": v_cr, "multiplicity": multiplicity, "vdry": vdry,
        "idx": idx, "rhod": rhod, "thd": thd, "water_vapour_mixing_ratio": qv, "dv": 1e6,
        "prhod": prhod, "pthd": pthd, "predicted_water_vapour_mixing_ratio": pqv,
        "kappa": kappa, "f_org": np.zeros(n_sd), "rtol_x": 1e-6, "rtol_thd": 1e-9,
        "timestep": dt, "cell_order": rng.permutation(n_cell).astype(np.int64),
        "reynolds_number": np.zeros(n_sd), "air_density": air_density,
        "air_dynamic_viscosity": eta, "dt_range": (1e-4, dt), "fuse": 32, "multiplier": 2,
        "RH_rtol": 1e-7, "max_iters": int(max_iters),
    }


def run_case(engine, case, *, adaptive, n_substeps_in=None):
    """one sdm_condensation call on `engine`; returns host copies of everything it writes"""
    from pysdm_amd.condensation import condensation_call  # pylint: disable=import-outside-toplevel

    up = engine.upload
    arrays = {k: up(np.asarray(v)) for k, v in case.items()
              if isinstance(v, np.ndarray) and k != "cell_order"}
    n_cell = case["n_cell"]
    start = -1 if adaptive else 3
    counters = {k: up(np.full(n_cell, start if k == "n_substeps" else -1, dtype=np.int64))
                for k in COUNTERS}
    if n_substeps_in is not None:
        counters["n_substeps"] = up(np.asarray(n_substeps_in, dtype=np.int64))
    RH_max = up(np.full(n_cell, np.nan))
    success = up(np.zeros(n_cell, dtype=np.uint8))
    scalars = {k: case[k] for k in ("formulae", "n_sd", "n_cell", "dv", "rtol_x", "rtol_thd",
                                    "timestep", "dt_range", "fuse", "multiplier", "RH_rtol",
                                    "max_iters")}
    condensation_call(
        engine, **scalars, adaptive=adaptive, counters=counters,
        cell_order=up(case["cell_order"]), RH_max=RH_max, success=success,
        **{k: v for k, v in arrays.items()})
    down = engine.download
    out = {k: down(v) for k, v in counters.items()}
    out.update(water_mass=down(arrays["water_mass"]), pthd=down(arrays["pthd"]),
               predicted_water_vapour_mixing_ratio=down(
                   arrays["predicted_water_vapour_mixing_ratio"]),
               RH_max=down(RH_max), success=down(success))
    return out

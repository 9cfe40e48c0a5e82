"""Shared by tests/test_chemistry_checker.py (the CPU checker) and tests/test_hip_chemistry.py
(the GPU): the recorded reference calls of tests/golden/chem_methods.npz and chem_steps.npz
(tests/golden/gen_chemistry_golden.py), the calls that replay them on an engine, and the bounds.

Bounds.
  RTOL_ARITHMETIC  outputs that are plain arithmetic plus exp / pow - the cell data, the
      dissociation factors, the amounts after dissolution and oxidation, the mixing-ratio
      decrements - agree with the reference within the project's 1e-12 relative (the bound of
      tests/deposition_cases.py and the breakup paths): a few dozen roundings of 1.1e-16 each and
      sdm_math.h's exp / pow, which differ from NumPy's in the last bit now and then.
  RTOL_PH  pH after equilibrate_H has no bound from first principles: TOMS748's iterates depend
      continuously on pH2H of the start, and sdm_pow differs from NumPy's power in the last bit in
      a few per cent of the arguments; the solver then stops at another point inside its
      tolerance.  MEASURED: the checker against chem_methods.npz differs by at most 2.9e-13
      relative in pH (eq1: 2.8e-16, the default bracket does not depend on the start; eq2:
      2.9e-13).  The bound is ten times that, for the shares of arguments that differ on other
      inputs; it is far below 1e-8, where a wrong branch would begin to hide (the solver's own
      promise is 1e-6 in H).
  RTOL_STEPS  the ten recorded steps of chem_steps.npz pass through 40 solves; MEASURED: the
      checker's `ChemistryRunner.step()`, summing in the recorded `idx` order, differs from the
      recording by at most 7.1e-11 relative (amounts; pH 5.7e-12, mixing ratios 1.2e-13).  Ten times that, below 1e-8.  The recording
      uses pH_rtol = 1e-12: with the default 1e-6 the reference does not reproduce ITSELF to 1e-8
      on such a state (one solve's start moved by one ulp changes its own pH by 4.5e-9, because
      which bracket's midpoint the solver returns hangs on the sign of a residual that is rounding
      noise; gen_chemistry_golden.py: STEPS_RTOL), and the checker then differed from it by 1.3e-6.
Flags are compared for equality with no row left out: the generator keeps every ionic strength
1e-9 clear of its threshold.
"""
import os

import numpy as np

from pysdm_amd import chemistry as chem
from pysdm_amd.abi import ChemistryCfg
from pysdm_amd.condensation import AmbientColumns
from pysdm_amd.formulae import Formulae
from pysdm_amd.population import Population

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL_ARITHMETIC = 1e-12
RTOL_PH = 2.9e-12
RTOL_STEPS = 7.1e-10
assert RTOL_PH < 1e-8 and RTOL_STEPS < 1e-8


def gold(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as data:
        return {key: data[key] for key in data.files}


def worst(got, want):
    """largest relative difference (0 where both are 0)"""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    scale = np.maximum(np.abs(got), np.abs(want))
    diff = np.abs(got - want)
    return float(np.max(np.where(scale > 0, diff / np.where(scale > 0, scale, 1), 0), initial=0))


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=what)


def limits_cfg(limits, system="open", sum_mode="ordered", timestep=0.0, dv=0.0, n_substep=1):
    cfg = ChemistryCfg()
    cfg.n_substep = n_substep
    cfg.system_type, cfg.sum = chem.SYSTEM_TYPES[system], chem.SUMS[sum_mode]
    cfg.timestep, cfg.cell_volume = float(timestep), float(dv)
    cfg.H_min, cfg.H_max = float(limits["H_min"]), float(limits["H_max"])
    cfg.ionic_strength_threshold = float(limits["ionic_strength_threshold"])
    cfg.rtol = float(limits["rtol"])
    return cfg


def limits_of(data):
    return {k: float(data[f"limits/{k}"]) for k in ("H_min", "H_max", "ionic_strength_threshold",
                                                    "rtol")}


def ups(engine, columns):
    return [engine.upload(np.array(c, dtype=float)) for c in columns]


def downs(engine, columns):
    return np.stack([np.asarray(engine.download(c)) for c in columns])


def count_of(engine, counter):
    return int(np.asarray(engine.download(counter))[0])


# ---- the stage symbols on an engine, host arrays in and out ---------------------------------------
def call_cell_data(engine, T, consts):
    n_cell = T.shape[0]
    eq, kin, henry = (ups(engine, np.zeros((n, n_cell))) for n in (7, 4, 6))
    engine.call_chemistry("sdm_chem_recalculate_cell_data", n_cell, engine.upload(T), eq, kin,
                          henry, list(consts))
    return downs(engine, eq), downs(engine, kin), downs(engine, henry)


def call_drop_data(engine, pH, cell, eq, consts):
    df = ups(engine, np.zeros((6, pH.shape[0])))
    engine.call_chemistry("sdm_chem_recalculate_drop_data", pH.shape[0], engine.upload(pH),
                          engine.upload(cell), ups(engine, eq), df, list(consts))
    return downs(engine, df)


def call_equilibrate(engine, cell, conc, eq, pH, flag, limits, consts):
    """conc: the five columns in chem.CONC order; returns (pH, flag, n_failed)"""
    d_pH, d_flag = engine.upload(pH), engine.upload(flag.astype(np.uint8))
    n_failed = engine.upload(np.array([-7], dtype=np.int64))
    engine.call_chemistry("sdm_equilibrate_H", limits_cfg(limits), pH.shape[0],
                          engine.upload(cell), ups(engine, conc), ups(engine, eq), d_pH, d_flag,
                          n_failed, list(consts))
    return (np.asarray(engine.download(d_pH)), np.asarray(engine.download(d_flag)).astype(bool),
            count_of(engine, n_failed))


def call_dissolution(engine, case, system, sum_mode="ordered", consts=None):
    """case: idx, cell_start, flag, moles (6, gas order), mixing_ratio (6, n_cell), T, p, rhod,
    henry, df, volume, multiplicity, dt, dv; returns (moles, mixing ratios, n_negative,
    n_exceeded)"""
    cfg = limits_cfg(dict(H_min=0, H_max=0, ionic_strength_threshold=0, rtol=0), system,
                     sum_mode, case["dt"], case["dv"])
    up = engine.upload
    moles, ratios = ups(engine, case["moles"]), ups(engine, case["mixing_ratio"])
    counters = [up(np.array([-7], dtype=np.int64)) for _ in range(2)]
    n_sd = case["volume"].shape[0]
    engine.call_chemistry(
        "sdm_dissolution", cfg, n_sd, case["cell_start"].shape[0] - 1, up(case["idx"]),
        up(case["cell_start"]), up(case["flag"].astype(np.uint8)), moles, ratios, up(case["T"]),
        up(case["p"]), up(case["rhod"]), ups(engine, case["henry"]), ups(engine, case["df"]),
        up(case["volume"]), up(case["multiplicity"]), counters[0], counters[1],
        list(case["consts"] if consts is None else consts))
    return (downs(engine, moles), downs(engine, ratios), count_of(engine, counters[0]),
            count_of(engine, counters[1]))


def call_oxidation(engine, cell, flag, kin, eq, dt, volume, pH, df_so2, moles, consts):
    """moles: O3, H2O2, S_IV, S_VI; returns the four columns"""
    cols = ups(engine, moles)
    engine.call_chemistry("sdm_oxidation", cell.shape[0], engine.upload(cell),
                          engine.upload(flag.astype(np.uint8)), ups(engine, kin),
                          ups(engine, eq), float(dt), engine.upload(volume), engine.upload(pH),
                          engine.upload(df_so2), *cols, list(consts))
    return downs(engine, cols)


# ---- chem_methods.npz -------------------------------------------------------------------------------
def methods_conc(data, which):
    conc = np.stack([data[f"eq1/conc/{k}"] for k in chem.CONC])
    return conc if which == 1 else conc * data["eq2/scale"]


def methods_moles_in(data):
    """the seven amounts before the recorded dissolution, in chem.AQUEOUS order"""
    conc2 = dict(zip(chem.CONC, methods_conc(data, 2)))
    moles = {k: conc2[k] * data["volume"] for k in chem.CONC}
    moles["O3"], moles["H2O2"] = data["dis/moles_O3_in"], data["dis/moles_H2O2_in"]
    return moles


def methods_dissolution_case(data):
    moles = methods_moles_in(data)
    return dict(idx=data["dis/idx"], cell_start=data["dis/cell_start"], flag=data["eq2/flag"],
                moles=np.stack([moles[k] for k in chem.GAS_KEYS]),
                mixing_ratio=data["dis/mixing_ratio_in"], T=data["ambient/T"],
                p=data["ambient/p"], rhod=data["ambient/rhod"], henry=data["cell/henry"],
                df=data["drop/df"], volume=data["volume"], multiplicity=data["multiplicity"],
                dt=float(data["dis/dt"]), dv=float(data["dis/dv"]), consts=data["consts"])


def methods_oxidation_in(data):
    """O3, H2O2, S_IV, S_VI after the recorded dissolution"""
    moles = methods_moles_in(data)
    moles.update(dict(zip(chem.GAS_KEYS, data["dis/moles_out"])))
    return np.stack([moles[k] for k in ("O3", "H2O2", "S_IV", "S_VI")])


# ---- synthetic cases ----------------------------------------------------------------------------------
def counted_case(seed, counts, unflagged=300):
    """a dissolution case whose cell c has counts[c] flagged rows (plus `unflagged` rows spread
    over the cells with the flag off), in a random order inside each cell; physically plausible
    values, consts of the default formulae"""
    rng = np.random.default_rng(seed)
    n_cell = len(counts)
    cell = np.concatenate([np.full(n, c) for c, n in enumerate(counts)]
                          + [rng.integers(0, n_cell, unflagged)]).astype(np.int64)
    flag = np.concatenate([np.ones(sum(counts), dtype=bool), np.zeros(unflagged, dtype=bool)])
    order = rng.permutation(cell.shape[0])
    cell, flag = cell[order], flag[order]
    return seeded_case(rng, cell, flag, n_cell)


def scale_dv(engine, case, target=0.1):
    """sets the case's cell volume so that the largest decrement of a closed system is `target` of
    its mixing ratio (the decrements are proportional to 1 / dv)"""
    _, ratios, _, _ = call_dissolution(engine, case, "closed")
    largest = np.abs(ratios / case["mixing_ratio"] - 1).max()
    case["dv"] = case["dv"] * largest / target
    return case


def seeded_case(rng, cell, flag, n_cell):
    n = cell.shape[0]
    consts = np.array(chem.constants_of(Formulae()))
    T = rng.uniform(275, 298, n_cell)
    p = rng.uniform(85e3, 100e3, n_cell)
    volume = 4.1887902047863905 * np.exp(rng.uniform(np.log(1e-6), np.log(2e-5), n)) ** 3
    idx = np.lexsort((rng.uniform(size=n), cell)).astype(np.int64)
    cell_start = np.searchsorted(cell[idx], np.arange(n_cell + 1)).astype(np.int64)
    henry = np.stack([consts[42 + g] * np.exp(consts[48 + g] * (1 / T - 1 / 298.15))
                      for g in range(6)])
    return dict(idx=idx, cell_start=cell_start, flag=flag, cell_id=cell,
                moles=np.exp(rng.uniform(np.log(1e-5), np.log(1e-1), (6, n))) * volume,
                mixing_ratio=np.exp(rng.uniform(np.log(1e-10), np.log(1e-7), (6, n_cell))),
                T=T, p=p, rhod=p / 287.0421396862956 / T, henry=henry,
                df=1 + np.exp(rng.uniform(0, 8, (6, n))), volume=volume,
                multiplicity=rng.integers(1, 1000, n).astype(np.int64), dt=0.5, dv=1e-9,
                consts=consts)


# ---- ChemistryRunner over a recorded or drawn state ------------------------------------------------------
# mole fractions whose mixing ratios are the recorded ones are not needed: the runner's mixing
# ratios are overwritten with the recorded start
_ANY_FRACTIONS = {g: 1e-9 for g in chem.GASES}


def runner_for(engine, *, cell, n_cell, multiplicity, volume, moles, pH, flag, T, p, mixing_ratio,
               system, n_substep, sum_mode, dt, dv, limits=None, constants="auto", idx=None):
    """a ChemistryRunner whose state is the given host arrays (moles: chem.AQUEOUS order)"""
    formulae = Formulae()
    rows = {f"moles_{k}": np.array(moles[at], dtype=float) for at, k in enumerate(chem.AQUEOUS)}
    pop = Population(engine, multiplicity=multiplicity, volume=volume, cell_id=cell,
                     n_cell=n_cell, more_extensive=rows)
    rhod = p / formulae.constants.Rd / T
    ambient = AmbientColumns(engine, formulae, rhod=rhod, thd=np.full(n_cell, 300.0),
                             qv=np.full(n_cell, 1e-3))
    # (the chemistry path reads T, p, rhod of the ambient only; set to the case's values)
    engine.assign(ambient.T, engine.upload(np.array(T, dtype=float)))
    engine.assign(ambient.p, engine.upload(np.array(p, dtype=float)))
    limits = limits or {}
    if idx is not None:  # the recorded order inside the cells (one cell: cell_start is [0, n])
        assert n_cell == 1
        pop.sorted_cell_start()
        engine.assign(pop.perm, engine.upload(np.array(idx, dtype=np.int64)))
    setup = chem.ChemistrySetup(system, n_substep, sum=sum_mode, constants=constants,
                                pH_H_min=limits.get("H_min"), pH_H_max=limits.get("H_max"),
                                ionic_strength_threshold=limits.get("ionic_strength_threshold"),
                                pH_rtol=limits.get("rtol", 1e-6))
    runner = chem.ChemistryRunner(pop, setup, ambient, dt=dt, dv=dv, mole_fractions=_ANY_FRACTIONS,
                                  volume=volume)
    engine.assign(runner.pH, engine.upload(np.array(pH, dtype=float)))
    engine.assign(runner.do_chemistry_flag, engine.upload(np.asarray(flag).astype(np.uint8)))
    for column, values in zip(runner.mixing_ratios, mixing_ratio):
        engine.assign(column, engine.upload(np.array(values, dtype=float)))
    return runner


def steps_runner(engine, data, sum_mode="ordered"):
    return runner_for(engine, cell=data["cell_id"], n_cell=1, multiplicity=data["multiplicity"],
                      volume=data["volume"], moles=data["moles"], pH=data["pH"],
                      flag=data["flag"], T=data["ambient/T"], p=data["ambient/p"],
                      mixing_ratio=data["mixing_ratio"], system="closed",
                      n_substep=int(data["n_substep"]), sum_mode=sum_mode, dt=float(data["dt"]),
                      dv=float(data["dv"]), limits=limits_of(data), idx=data["idx"])


def drawn_state(seed, n_sd, n_cell):
    """a state for step() against step_by_stages(): amounts that keep most rows under the
    ionic-strength threshold, every cell populated"""
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, n_cell, n_sd).astype(np.int64)
    volume = 4.1887902047863905 * np.exp(rng.uniform(np.log(5e-7), np.log(1.5e-5), n_sd)) ** 3
    salt = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), n_sd))
    moles = {"S_VI": salt * volume, "N_mIII": 2 * salt * volume * rng.uniform(0.8, 1.0, n_sd)}
    for k in ("S_IV", "O3", "H2O2", "C_IV", "N_V"):
        moles[k] = np.exp(rng.uniform(np.log(1e-6), np.log(1e-3), n_sd)) * volume
    return dict(cell=cell, n_cell=n_cell, multiplicity=rng.integers(100, 10000, n_sd),
                volume=volume, moles=np.stack([moles[k] for k in chem.AQUEOUS]),
                pH=np.full(n_sd, 7.0), flag=np.zeros(n_sd, dtype=bool),
                T=rng.uniform(278, 296, n_cell), p=rng.uniform(88e3, 99e3, n_cell),
                mixing_ratio=np.exp(rng.uniform(np.log(1e-10), np.log(1e-7), (6, n_cell))))

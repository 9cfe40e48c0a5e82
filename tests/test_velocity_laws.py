"""Fall-velocity laws in the collision step, without a GPU: the planted input is what it claims to
be, the CPU checker's stage route reproduces the goldens recorded from the reference with
Rogers-Yau and the power series, a fused route refuses a law its engine lacks (by name, and only
where a velocity is needed), the step description carries the law and its numbers, and the PySDM
plug-in reads the law from the formulae."""
import ctypes
import types
import warnings

import numpy as np
import pytest

from pysdm_amd import abi
from pysdm_amd import recipe as R
from pysdm_amd.physics import constants as const
from pysdm_amd.population import Population
from pysdm_amd.collisions import CollisionRunner
from pysdm_amd.terminal_velocity import GunnKinzerTable, PowerSeries, RogersYau

from . import relaxed_velocity_cases as rc
from . import velocity_law_cases as vc
from .trajectory import compare

COALESCENCE_GOLDENS = [name for name, (_, breakup) in vc.GOLDENS.items() if not breakup]
BREAKUP_GOLDENS = [name for name, (_, breakup) in vc.GOLDENS.items() if breakup]


# ---- the planted input ----------------------------------------------------------------------------
def test_planted_input_straddles_both_limits_of_rogers_yau(oracle_engine):
    """in the radius the library derives from the mass column (the checker's stage symbols, so
    sdm_pow): rows on each limit and beside it on either side.  "Beside": within 16 ulps - the
    plants lie within 8 * 2**-52 of the limit, which is at most 9.2 ulps of these two numbers, and
    mass -> volume -> radius is four roundings and a pow good to an ulp"""
    volume, multiplicity = vc.planted()
    population = Population(oracle_engine, multiplicity=multiplicity, volume=volume)
    radius = oracle_engine.download(population.radius())
    for at, limit in enumerate(vc.LIMITS):
        near = radius[at * 17:(at + 1) * 17]
        ulps = np.round((near - limit) / np.spacing(limit)).astype(int)
        print(f"limit {limit}: below {(near < limit).sum()}, on {(near == limit).sum()}, "
              f"above {(near > limit).sum()}; ulps {ulps.tolist()}")
        assert (near == limit).any()
        assert ((ulps < 0) & (ulps >= -16)).any() and ((ulps > 0) & (ulps <= 16)).any()
        assert np.abs(ulps).max() <= 16
    regimes = vc.rogers_yau_regimes(radius)
    print("rows per regime:", regimes)
    assert min(regimes) >= 100 and sum(regimes) == len(radius)
    assert multiplicity.min() == 1 and multiplicity.max() == 3


@pytest.mark.parametrize("name", ["traj_velocity_rogers_yau", "traj_velocity_power_series"])
def test_recorded_box_runs_collide_and_kill_without_dying_out(name):
    gold = np.load(vc.GOLDEN + "/" + name + ".npz")
    np.testing.assert_array_equal(gold["init/volume"], vc.planted()[0])
    np.testing.assert_array_equal(gold["init/multiplicity"], vc.planted()[1])
    coalescences, alive = int(gold["step4/coalescence_rate"].sum()), int(gold["step4/length"])
    print(f"{name}: coalescences {coalescences}, alive {alive} of 1024, sub-steps "
          f"{gold['step4/stats_n_substep'].max()}")
    assert coalescences >= 500
    assert 512 <= alive < 1024


def test_the_laws_differ_on_the_planted_input():
    last = [np.load(vc.GOLDEN + f"/traj_velocity_{tag}.npz")["step4/multiplicity"]
            for tag in ("rogers_yau", "power_series")]
    assert (last[0] != last[1]).any()


# ---- the checker's stage route against the reference -----------------------------------------------
@pytest.mark.parametrize("name", COALESCENCE_GOLDENS)
def test_checker_chain_reproduces_the_reference_exactly(name, oracle_engine):
    runner, gold, steps = vc.golden_runner(name, oracle_engine, "chain")
    for step in steps:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runner.run(step - runner.steps_done)
        compare(runner.snapshot(), gold, step)


@pytest.mark.parametrize("name", BREAKUP_GOLDENS)
def test_checker_chain_reproduces_the_reference_breakup_run(name, oracle_engine):
    runner, gold, steps = vc.golden_runner(name, oracle_engine, "chain")
    assert gold[f"step{steps[-1]}/breakup_rate"].sum() > 0
    for step in steps:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runner.run(step - runner.steps_done)
        compare(runner.snapshot(), gold, step, float_rtol=1e-12)


# ---- the refusal -----------------------------------------------------------------------------------
@pytest.mark.parametrize("law", ["RogersYau", "PowerSeries", PowerSeries(**vc.TWO_TERMS)],
                         ids=["RogersYau", "PowerSeries", "PowerSeries-object"])
def test_fused_route_refuses_a_law_the_engine_lacks(law, oracle_engine):
    assert oracle_engine.fused_velocity_laws == ("GunnKinzer1949",)
    name = law if isinstance(law, str) else "PowerSeries"
    with pytest.raises(NotImplementedError) as refusal:
        vc.box_runner(oracle_engine, law, route="fused", adaptive=True)
    assert name in str(refusal.value) and "route='chain'" in str(refusal.value)
    assert oracle_engine.name in str(refusal.value)
    # no velocity in the set-up: any law will do, on any engine
    volume, multiplicity = vc.planted(64)
    population = Population(oracle_engine, multiplicity=multiplicity, volume=volume)
    runner = CollisionRunner(population, R.CollisionSetup.coalescence(R.Golovin(b=1.5e3), seed=1),
                             dt=1.0, dv=1.0, route="fused", terminal_velocity=law)
    assert runner.step_cfg().velocity_law == 0 and not runner._step_state().velocity_params  # pylint: disable=protected-access
    vc.box_runner(oracle_engine, law, route="chain", adaptive=True)


def test_unknown_law_is_refused_by_name(oracle_engine):
    with pytest.raises(ValueError, match="Beard1976"):
        vc.box_runner(oracle_engine, "Beard1976", route="chain", adaptive=True)
    with pytest.raises(ValueError, match="not a terminal-velocity law"):
        vc.box_runner(oracle_engine, object(), route="chain", adaptive=True)


# ---- the step description --------------------------------------------------------------------------
class AnnouncingEngine:
    """an engine that only announces the capability: arrays are numpy, nothing is ever called"""

    name = "announcing"
    fused_momentum_velocity = False
    fused_velocity_laws = ("GunnKinzer1949", "RogersYau", "PowerSeries")

    def __init__(self, inner):
        self.inner = inner

    def call(self, symbol, *args):
        raise AssertionError(f"nothing is run here: {symbol}")

    def __getattr__(self, name):
        if name in ("empty", "upload", "download", "zeros", "full", "fill", "assign", "size"):
            return getattr(self.inner, name)
        raise AttributeError(name)


def _doubles(pointer, count):
    return np.ctypeslib.as_array(ctypes.cast(pointer, ctypes.POINTER(ctypes.c_double)),
                                 shape=(count,)).copy()


def test_step_description_carries_rogers_yau_with_the_runners_constants(oracle_engine):
    changed = const.namespace({"ROGERS_YAU_TERM_VEL_MEDIUM_K": 7.5e3})
    volume, multiplicity = vc.planted(64)
    population = Population(AnnouncingEngine(oracle_engine), multiplicity=multiplicity,
                            volume=volume)
    runner = CollisionRunner(population, R.CollisionSetup.coalescence(R.Geometric(), seed=1),
                             dt=1.0, dv=1.0, route="fused", terminal_velocity="RogersYau",
                             constants=changed)
    cfg, state = runner.step_cfg(), runner._step_state()  # pylint: disable=protected-access
    assert (cfg.velocity_law, cfg.velocity_terms, cfg.gk_table_len) == (1, 0, 0)
    assert not state.gk_a and not state.gk_b and state.velocity_params
    np.testing.assert_array_equal(_doubles(state.velocity_params, 5), [
        const.ROGERS_YAU_TERM_VEL_SMALL_K, 7.5e3, const.ROGERS_YAU_TERM_VEL_LARGE_K,
        const.ROGERS_YAU_TERM_VEL_SMALL_R_LIMIT, const.ROGERS_YAU_TERM_VEL_MEDIUM_R_LIMIT])
    # the stage route evaluates the same object
    assert runner.law.consts[1] == 7.5e3 and isinstance(runner.law, RogersYau)


def test_step_description_carries_the_users_power_series(oracle_engine):
    law = PowerSeries(**vc.TWO_TERMS)
    volume, multiplicity = vc.planted(64)
    population = Population(AnnouncingEngine(oracle_engine), multiplicity=multiplicity,
                            volume=volume)
    runner = CollisionRunner(population, R.CollisionSetup.coalescence(R.Geometric(), seed=1),
                             dt=1.0, dv=1.0, route="fused", terminal_velocity=law)
    cfg, state = runner.step_cfg(), runner._step_state()  # pylint: disable=protected-access
    assert (cfg.velocity_law, cfg.velocity_terms, cfg.gk_table_len) == (2, 2, 0)
    assert not state.gk_a and not state.gk_b and state.velocity_params
    powers = np.asarray(vc.TWO_TERMS["powers"])
    scaled = np.asarray(vc.TWO_TERMS["prefactors"]) * const.PI_4_3 ** powers / 1e-6 ** (3 * powers)
    np.testing.assert_array_equal(_doubles(state.velocity_params, 4),
                                  np.concatenate([scaled, powers]))
    assert runner.law is law
    with pytest.raises(ValueError, match="16"):
        CollisionRunner(population, R.CollisionSetup.coalescence(R.Geometric(), seed=1), dt=1.0,
                        dv=1.0, route="fused", terminal_velocity=PowerSeries(
                            prefactors=[1.0] * 17, powers=[0.5] * 17)).step_cfg()


def test_gunn_kinzer_gives_todays_step_description(oracle_engine):
    volume, multiplicity = vc.planted(64)
    population = Population(oracle_engine, multiplicity=multiplicity, volume=volume)
    runner = CollisionRunner(population, R.CollisionSetup.coalescence(R.Geometric(), seed=1),
                             dt=1.0, dv=1.0, route="fused")
    cfg, state = runner.step_cfg(), runner._step_state()  # pylint: disable=protected-access
    assert (cfg.velocity_law, cfg.velocity_terms) == (0, 0)
    assert cfg.gk_table_len == 601 and cfg.gk_factor == 1e5
    assert state.gk_a and state.gk_b and not state.velocity_params
    assert isinstance(runner.law, GunnKinzerTable)
    # the new members lie behind the ones there were
    assert abi.StepCfg.velocity_law.offset == abi.StepCfg.momentum_attr.offset + 4
    assert abi.StepState.velocity_params.offset == abi.StepState.cell_id_by_id.offset + 8


# ---- the PySDM plug-in -----------------------------------------------------------------------------
@pytest.fixture(scope="module", name="ref")
def reference_modules():
    return rc.import_reference()


def test_velocity_law_from_pysdm(ref):
    from pysdm_amd.pysdm_plugin import velocity_law_from_pysdm  # pylint: disable=import-outside-toplevel

    formulae = ref["PySDM"].Formulae
    assert velocity_law_from_pysdm(formulae(terminal_velocity="GunnKinzer1949")) == "GunnKinzer1949"
    law = velocity_law_from_pysdm(formulae(terminal_velocity="RogersYau"))
    assert isinstance(law, RogersYau) and law.consts == RogersYau().consts
    law = velocity_law_from_pysdm(formulae(
        terminal_velocity="RogersYau", constants={"ROGERS_YAU_TERM_VEL_MEDIUM_R_LIMIT": 5e-4}))
    assert law.consts[4] == 5e-4 and law.consts[:4] == RogersYau().consts[:4]
    law = velocity_law_from_pysdm(formulae(terminal_velocity="PowerSeries"))
    theirs = formulae(terminal_velocity="PowerSeries").terminal_velocity_class(None)
    assert isinstance(law, PowerSeries)
    np.testing.assert_array_equal(law.prefactors, theirs.prefactors)
    np.testing.assert_array_equal(law.powers, theirs.powers)
    with pytest.raises(NotImplementedError, match="TpDependent"):
        velocity_law_from_pysdm(types.SimpleNamespace(terminal_velocity="TpDependent"))


def test_fused_collisions_refuse_a_law_of_the_formulae_the_engine_lacks(ref, oracle_backend_class):
    """before: ran Gunn-Kinzer under Formulae(terminal_velocity="RogersYau") without a word"""
    from pysdm_amd.pysdm_plugin import as_pysdm_backend, fuse  # pylint: disable=import-outside-toplevel

    volume, multiplicity = vc.planted(64)
    formulae = ref["PySDM"].Formulae(seed=44, terminal_velocity="RogersYau")
    builder = ref["PySDM"].Builder(
        n_sd=64, backend=as_pysdm_backend(oracle_backend_class)(formulae),
        environment=ref["Box"](dt=1.0, dv=0.1))
    builder.add_dynamic(fuse(ref["Coalescence"](collision_kernel=ref["Geometric"]())))
    particulator = builder.build(attributes={"multiplicity": multiplicity.astype(float),
                                             "volume": volume}, products=())
    with pytest.raises(NotImplementedError) as refusal:
        particulator.run(steps=1)
    assert "RogersYau" in str(refusal.value) and "route='chain'" in str(refusal.value)

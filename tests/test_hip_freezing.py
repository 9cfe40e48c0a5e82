"""The freezing path on the MI355X: include/sdm_freezing.h through libsdm_hip.so.

(i) the HIP class replays the recorded calls of frz_methods.npz and the three recorded Box runs
with the equality the CPU checker is held to (the reference's bits), (ii) HIP and the checker
agree bit for bit on seeded states - 1 to 70001 super-droplets (one wave, the workgroup and
PCG_ELEMS edges, an unaligned tail, several workgroups), 1 and 7 cells, every stage symbol, the
fused step in all flag combinations, stream offsets up to 2^33 + 5 -, (iii) the fused step equals
the stage sequence on HIP, also over two steps, with and without the recording column and however
the rates are obtained, (iv) NaN activities do not matter to the Constant rates."""
import numpy as np
import pytest

from tests import freezing_cases as fc
from tests.test_freezing_checker import BOXES, METHODS, run_pysdm_box

pytestmark = pytest.mark.gpu
STOCHASTIC = [flags for flags in fc.FLAGS if flags[2] or (flags[1] and not flags[0])]
# (singular, immersion, homogeneous, thaw): two stochastic passes, one of either kind, singular +
# homogeneous
FAR_OFFSET_FLAGS = [(False, True, True, True), (False, True, False, False),
                    (False, False, True, False), (True, True, True, True)]


@pytest.fixture(scope="module", name="checker")
def checker_engine():
    from tests.freezing_checker import FreezingCheckerEngine  # pylint: disable=import-outside-toplevel

    return FreezingCheckerEngine.get()


def _same(got, want, what):
    fc.assert_same_bits(got[0], want[0], f"{what} mass")
    if want[1] is not None:
        fc.assert_same_values(got[1], want[1], f"{what} temperature of last freezing")


def test_hip_replays_recorded_method_calls(hip_backend_class):
    for number in range(int(METHODS["n_calls"])):
        got, expected = fc.replay_method_call(hip_backend_class, METHODS, number)
        fc.assert_same_bits(got, expected, f"call {number}")
    for stage, (mass, want_mass, data, want_data) in enumerate(
            fc.replay_record_sequence(hip_backend_class, METHODS)):
        fc.assert_same_bits(mass, want_mass, f"stage {stage} mass")
        fc.assert_same_values(data, want_data, f"stage {stage} data")
    a_w_ice, RH_ice = fc.replay_a_w_ice(hip_backend_class, METHODS)
    fc.assert_same_bits(a_w_ice, METHODS["a_w_ice/out_a_w_ice"], "a_w_ice")
    fc.assert_same_bits(RH_ice, METHODS["a_w_ice/out_RH_ice"], "RH_ice")
    volume, mass = fc.replay_conversions(hip_backend_class, METHODS)
    fc.assert_same_bits(volume, METHODS["conversion/out_volume"], "volume")
    fc.assert_same_bits(mass, METHODS["conversion/out_mass"], "mass")


@pytest.mark.parametrize("name", BOXES)
def test_hip_runner_reproduces_recorded_box_run(hip_engine, name):
    data = fc.gold(name)
    masses = fc.run_box(hip_engine, data)
    for step, (got, want) in enumerate(zip(masses, data["masses"])):
        fc.assert_same_bits(got, want, f"{name} step {step}")


@pytest.mark.parametrize("n_sd", [1, 3, 63, 64, 65, 1000, 4097, 70001])
def test_hip_equals_checker_bitwise(hip_engine, checker, n_sd):
    formulae = fc.formulae_for(het="ABIFM", hom="Koop_Correction")
    for n_cell in (1, 7):
        state = fc.seeded_state(100 + n_sd + n_cell, n_sd, n_cell)
        got = fc.stage_symbols(hip_engine, state, formulae)
        want = fc.stage_symbols(checker, state, formulae)
        for key, value in want.items():
            fc.assert_same_values(got[key], value, f"{key} n_sd={n_sd} n_cell={n_cell}")
        cases = [(flags, 0) for flags in fc.FLAGS]
        cases += [(flags, offset) for flags in FAR_OFFSET_FLAGS for offset in fc.OFFSETS[1:]]
        for flags, offset in cases:
            _same(fc.fused_steps(hip_engine, state, formulae, flags, offset),
                  fc.fused_steps(checker, state, formulae, flags, offset),
                  f"n_sd={n_sd} n_cell={n_cell} flags={flags} offset={offset}")


@pytest.mark.parametrize("hom", ["Constant", "Koop2000", "KoopMurray2016"])
def test_hip_equals_checker_for_the_other_rates(hip_engine, checker, hom):
    formulae = fc.formulae_for(het="Constant", hom=hom)
    state = fc.seeded_state(9, 4097, 7)
    flags = (False, True, True, True)
    _same(fc.fused_steps(hip_engine, state, formulae, flags, 12345),
          fc.fused_steps(checker, state, formulae, flags, 12345), hom)


@pytest.mark.parametrize("n_cell", [1, 7, 1024, 1025])
def test_fused_step_equals_stage_sequence_on_hip(hip_engine, n_cell):
    """one and two steps, the volume given or taken from the mass, the rates per droplet or per
    cell (1024 cells: the most that are kept per cell; 1025: per droplet whatever is asked)"""
    formulae = fc.formulae_for(het="ABIFM", hom="Koop2000")
    state = fc.seeded_state(21 + n_cell, 4097, n_cell)
    for flags in fc.FLAGS:
        for n_steps, own_volume in ((1, True), (2, False)):
            want = fc.stage_sequence(hip_engine, state, formulae, flags, 12345, n_steps=n_steps,
                                     own_volume=own_volume)
            for rates in ("auto", "per_droplet", "per_cell")[:3 if n_cell <= 1024 else 2]:
                got = fc.fused_steps(hip_engine, state, formulae, flags, 12345, n_steps=n_steps,
                                     own_volume=own_volume, rates=rates)
                _same(got, want, f"flags={flags} steps={n_steps} rates={rates}")
    changed = fc.fused_steps(hip_engine, state, formulae, (False, True, True, True), 12345)[0]
    assert (changed != state["signed_water_mass"]).any()


def test_masses_do_not_depend_on_the_recording_column(hip_engine):
    formulae = fc.formulae_for(het="ABIFM", hom="Koop2000")
    state = fc.seeded_state(33, 4097, 7)
    for flags in STOCHASTIC:
        with_column = fc.fused_steps(hip_engine, state, formulae, flags, 5, record=True)
        without = fc.fused_steps(hip_engine, state, formulae, flags, 5, record=False)
        assert without[1] is None
        fc.assert_same_bits(with_column[0], without[0], str(flags))


def test_nan_activity_does_not_matter_to_constant_rates(hip_engine):
    formulae = fc.formulae_for(het="Constant", hom="Constant")
    state = fc.seeded_state(34, 4097, 7)
    flags = (False, True, True, True)
    nan = np.full(7, np.nan)
    for rates in ("per_droplet", "per_cell"):
        want = fc.fused_steps(hip_engine, state, formulae, flags, 7, rates=rates)
        _same(fc.fused_steps(hip_engine, state, formulae, flags, 7, rates=rates, a_w_ice=nan),
              want, rates)
        assert (want[0] != state["signed_water_mass"]).any()


def test_per_cell_rates_refuse_more_cells_than_fit(hip_engine):
    formulae = fc.formulae_for(het="ABIFM", hom="Koop2000")
    state = fc.seeded_state(35, 64, 1025)
    with pytest.raises(RuntimeError, match="error -"):
        fc.fused_steps(hip_engine, state, formulae, (False, True, True, True), 0,
                       rates="per_cell")
    fc.fused_steps(hip_engine, state, formulae, (False, True, True, True), 0)


@pytest.mark.parametrize("name", BOXES)
def test_pysdm_box_runs_on_the_hip_class(hip_backend_class, name):
    """an unmodified PySDM Builder + Box + Freezing on the HIP class reproduces the recorded run"""
    pytest.importorskip("PySDM")
    from PySDM import Builder  # pylint: disable=import-outside-toplevel,import-error
    from PySDM import Formulae as PySDMFormulae  # pylint: disable=import-outside-toplevel,import-error
    from PySDM.dynamics import Freezing  # pylint: disable=import-outside-toplevel,import-error
    from PySDM.environments import Box  # pylint: disable=import-outside-toplevel,import-error

    from pysdm_amd.pysdm_plugin import as_pysdm_backend  # pylint: disable=import-outside-toplevel

    data = fc.gold(name)
    masses = run_pysdm_box(as_pysdm_backend(hip_backend_class), data, Builder, PySDMFormulae,
                           Freezing, Box)
    for step, (got, want) in enumerate(zip(masses, data["masses"])):
        fc.assert_same_bits(got, want, f"{name} step {step}")

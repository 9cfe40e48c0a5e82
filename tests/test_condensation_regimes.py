"""The condensation formulae against a 50-digit reference, regime by regime
(tests/condensation_regime_cases.py, tests/golden/condensation_regimes.npz): T, p and RH of
`sdm_temperature_pressure_rh[_f]`, the critical volume of `sdm_critical_volume[_f]`, the wet
radii of `sdm_equilibrate_wet_radii` and one
fixed sub-step of `sdm_condensation[_f]` on cells of one to three super-droplets with a tight
solver - each check once against the CPU checkers (no marker) and once against the HIP library
(`-m gpu`), which is also held to the checkers bit for bit.  Every bound is per row and derived
(four times the formulation's own rounding error plus the solvers' contracts)."""
import os
import subprocess
import sys

import pytest

from . import condensation_regime_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = pytest.mark.parametrize("group", sorted(rc.GROUPS))
POINTWISE = pytest.mark.parametrize("group", ["tprh", "vcr"])


def test_every_label_is_planted():
    rc.check_coverage()


def test_max_ulp_is_what_the_math_tests_pin():
    from . import test_sdm_math  # pylint: disable=import-outside-toplevel

    for name, value in rc.MAX_ULP.items():
        assert test_sdm_math.MAX_ULP[name] == value, name


def test_committed_fixture_is_the_generated_one():
    """regenerates the rows, their labels (both precisions agree on every row compared at 50
    digits, or the row would not be generated), the 50-digit values and the bounds; the float64
    run of the restatement has to stay within its own bounds"""
    pytest.importorskip("mpmath")
    subprocess.check_call([sys.executable, os.path.join(
        ROOT, "tests", "golden", "gen_condensation_regimes.py"), "--check"])


# ---- the CPU checkers ----------------------------------------------------------------------------
@GROUPS
def test_checker_regimes(group):
    """the default formulae through the default checker, every other set through the formulae
    checker"""
    worst = rc.check_group(rc.checker_engine(group), group)
    committed = rc.measured()
    for key, value in worst.items():  # the committed measurements are these
        assert value <= committed[key] * 1.01 + 1e-12, (key, value, committed[key])


@POINTWISE
def test_formulae_checker_serves_the_default_rows_too(group):
    rc.check_group(rc.checker_engine(group), group, general=True)


def test_checker_keeps_a_droplet_at_equilibrium():
    rc.check_equilibrium_rows(rc.checker_engine("cond"))


# ---- the HIP library -----------------------------------------------------------------------------
@pytest.mark.gpu
@GROUPS
def test_hip_regimes(group, hip_engine):
    rc.check_group(hip_engine, group)


@pytest.mark.gpu
@POINTWISE
def test_hip_general_symbols_serve_the_default_rows_too(group, hip_engine):
    rc.check_group(hip_engine, group, general=True)


@pytest.mark.gpu
@GROUPS
def test_hip_returns_the_checkers_bits(group, hip_engine):
    """float-only rows included"""
    rc.check_same_bits(hip_engine, rc.checker_engine(group), group)


@pytest.mark.gpu
def test_hip_keeps_a_droplet_at_equilibrium(hip_engine):
    rc.check_equilibrium_rows(hip_engine)


# ---- the reading of the reference ----------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference/PySDM"),
                    reason="reference tree not present")
def test_restatement_reads_the_reference():
    """the reference's own formula functions on the planted inputs against the float64 run of the
    restatement at rtol 1e-12 (tests/helpers/reference_condensation_regimes.py)"""
    done = subprocess.run(
        [sys.executable, "-B", os.path.join(ROOT, "tests", "helpers",
                                            "reference_condensation_regimes.py")],
        capture_output=True, text=True, timeout=600, cwd=ROOT, check=False)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]

"""Every regime of the breakup physics against a 50-digit reference (tests/breakup_regime_cases.py,
tests/golden/breakup_regimes.npz): each check once against the oracle (no marker) and once against
the HIP library (`-m gpu`), which is also held to the oracle bit for bit."""
import os
import subprocess
import sys

import pytest

from . import breakup_regime_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = pytest.mark.parametrize("group", sorted(bc.E))


def test_every_label_is_planted():
    bc.check_coverage()


def test_committed_fixture_is_the_generated_one():
    """regenerates the rows and their 50-digit values: the inputs, the labels (both precisions
    agree on every row compared at 50 digits, or the row would not be generated), the expected
    values, and E within the constants the bounds are made of"""
    pytest.importorskip("mpmath")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "golden",
                                                        "gen_breakup_regimes.py"), "--check"])


# ---- the oracle ---------------------------------------------------------------------------------
@GROUPS
def test_oracle_regimes(group, oracle_engine):
    bc.check_group(oracle_engine, group)


def test_oracle_lengths(oracle_engine):
    bc.check_lengths(oracle_engine)


# ---- the HIP library ----------------------------------------------------------------------------
@pytest.mark.gpu
@GROUPS
def test_hip_regimes(group, hip_engine):
    bc.check_group(hip_engine, group)


@pytest.mark.gpu
@GROUPS
def test_hip_returns_the_oracles_bits(group, hip_engine, oracle_engine):
    bc.check_same_bits(hip_engine, oracle_engine, group)


@pytest.mark.gpu
def test_hip_lengths(hip_engine):
    bc.check_lengths(hip_engine)


# ---- the fused step's copy of the energetics: fused == chain (== oracle), every pair known ---------
FUSED = pytest.mark.parametrize("fragmentation", sorted(bc.FUSED_FRAGMENTATIONS))
EFFICIENCIES = pytest.mark.parametrize("efficiency", ("berry", "lowlist", "straub"))


@FUSED
def test_oracle_fused_copy(fragmentation, oracle_engine):
    bc.check_fused([oracle_engine], fragmentation)


@EFFICIENCIES
def test_oracle_fused_copy_of_the_efficiencies(efficiency, oracle_engine):
    bc.check_fused([oracle_engine], "lowlist", efficiency)


@pytest.mark.gpu
@FUSED
def test_hip_fused_copy(fragmentation, hip_engine, oracle_engine):
    bc.check_fused([hip_engine, oracle_engine], fragmentation)


@pytest.mark.gpu
@EFFICIENCIES
def test_hip_fused_copy_of_the_efficiencies(efficiency, hip_engine, oracle_engine):
    bc.check_fused([hip_engine, oracle_engine], "lowlist", efficiency)


# ---- the reading of the reference -------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference/PySDM"),
                    reason="reference tree not present")
def test_restatement_reads_the_reference():
    """the reference's own functions on the planted inputs against the float64 run of the
    restatement at rtol 1e-12 (tests/helpers/reference_breakup_regimes.py)"""
    done = subprocess.run(
        [sys.executable, "-B", os.path.join(ROOT, "tests", "helpers",
                                            "reference_breakup_regimes.py")],
        capture_output=True, text=True, timeout=600, cwd=ROOT, check=False)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]

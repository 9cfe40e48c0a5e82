"""Displacement at cell faces, at the precipitation level, at the top of the column and past one
pass of the precipitation kernel, and the fall-velocity laws at their knots
(tests/displacement_edge_cases.py): every check once against the oracle (no marker: proves the
cases and their NumPy reference without a GPU) and once against the HIP library (`-m gpu`)."""
import pytest

from . import displacement_edge_cases as dc

STEPS = pytest.mark.parametrize("route", ("fused", "chain"))
STEP_CASES = pytest.mark.parametrize("name", dc.STEP_CASES)
EDGE_CASES = pytest.mark.parametrize("name", dc.EDGE_CASES)
LENGTHS = pytest.mark.parametrize("n", dc.INTERPOLATION_LENGTHS)


# ---- the oracle ---------------------------------------------------------------------------------
@STEP_CASES
@STEPS
def test_oracle_displacement(name, route, oracle_engine):
    dc.check_displacement(oracle_engine, name, route)


@EDGE_CASES
def test_oracle_displacement_one_step(name, oracle_engine):
    dc.check_displacement(oracle_engine, name, "fused", steps=1)


@LENGTHS
def test_oracle_interpolation(n, oracle_engine):
    dc.check_interpolation(oracle_engine, n)


def test_oracle_rogers_yau(oracle_engine):
    dc.check_rogers_yau(oracle_engine)


# ---- the HIP library ----------------------------------------------------------------------------
@pytest.mark.gpu
@STEP_CASES
@STEPS
def test_hip_displacement(name, route, hip_engine):
    dc.check_displacement(hip_engine, name, route)


@pytest.mark.gpu
@EDGE_CASES
def test_hip_displacement_one_step(name, hip_engine):
    dc.check_displacement(hip_engine, name, "fused", steps=1)


@pytest.mark.gpu
@LENGTHS
def test_hip_interpolation(n, hip_engine):
    dc.check_interpolation(hip_engine, n)


@pytest.mark.gpu
def test_hip_rogers_yau(hip_engine):
    dc.check_rogers_yau(hip_engine)

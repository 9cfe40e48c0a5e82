"""The read-out kernels at the shapes where their fast paths run (tests/readout_cases.py): every
check once against the oracle (no marker: proves the cases and their NumPy / math.fsum references
without a GPU) and once against the HIP library (`-m gpu`)."""
import pytest

from . import readout_cases as rc


@pytest.fixture(scope="module", name="oracle_kit")
def oracle_kit_fixture(oracle_backend_class):
    return rc.Kit(oracle_backend_class)


@pytest.fixture(scope="module", name="hip_kit")
def hip_kit_fixture(hip_backend_class):
    return rc.Kit(hip_backend_class)


def _ids(cases):
    return ["-".join(str(v) for v in case if v is not None) for case in cases]


MOMENTS = pytest.mark.parametrize("layout,length", rc.MOMENTS_EXACT_CASES,
                                  ids=_ids(rc.MOMENTS_EXACT_CASES))
TOLERANCE = pytest.mark.parametrize("layout", ["sorted_ragged", "random"])
SPECTRUM = pytest.mark.parametrize("edges,length,n_sd", rc.SPECTRUM_CASES,
                                   ids=_ids(rc.SPECTRUM_CASES))
EXTREMES = pytest.mark.parametrize("n", rc.EXTREME_SIZES)
PRECIPITATION = pytest.mark.parametrize("n_dims,length", rc.PRECIPITATION_CASES)


# ---- the oracle ---------------------------------------------------------------------------------
@MOMENTS
def test_oracle_moments_exact(layout, length, oracle_kit):
    rc.check_moments_exact(oracle_kit, layout, length)


@TOLERANCE
def test_oracle_moments_tolerance(layout, oracle_kit):
    rc.check_moments_tolerance(oracle_kit, layout)


def test_oracle_moments_backend(oracle_kit):
    rc.check_moments_backend(oracle_kit)


def test_oracle_moments_in_use(oracle_engine):
    rc.check_moments_in_use(oracle_engine)


@SPECTRUM
def test_oracle_spectrum_exact(edges, length, n_sd, oracle_kit):
    rc.check_spectrum_exact(oracle_kit, edges, length, n_sd)


def test_oracle_spectrum_one_bin_too_many(oracle_kit):
    rc.check_spectrum_one_bin_too_many(oracle_kit)


@EXTREMES
def test_oracle_extremes(n, oracle_kit):
    rc.check_extremes(oracle_kit, n)


def test_oracle_extremes_refuse_empty(oracle_kit):
    rc.check_extremes_refuse_empty(oracle_kit)


@PRECIPITATION
def test_oracle_flag_precipitated(n_dims, length, oracle_kit):
    rc.check_flag_precipitated(oracle_kit, n_dims, length)


# ---- the HIP library ----------------------------------------------------------------------------
@pytest.mark.gpu
@MOMENTS
def test_hip_moments_exact(layout, length, hip_kit):
    rc.check_moments_exact(hip_kit, layout, length)


@pytest.mark.gpu
@TOLERANCE
def test_hip_moments_tolerance(layout, hip_kit):
    rc.check_moments_tolerance(hip_kit, layout)


@pytest.mark.gpu
def test_hip_moments_backend(hip_kit):
    rc.check_moments_backend(hip_kit)


@pytest.mark.gpu
def test_hip_moments_in_use(hip_engine):
    rc.check_moments_in_use(hip_engine)


@pytest.mark.gpu
@SPECTRUM
def test_hip_spectrum_exact(edges, length, n_sd, hip_kit):
    rc.check_spectrum_exact(hip_kit, edges, length, n_sd)


@pytest.mark.gpu
def test_hip_spectrum_one_bin_too_many(hip_kit):
    rc.check_spectrum_one_bin_too_many(hip_kit)


@pytest.mark.gpu
@EXTREMES
def test_hip_extremes(n, hip_kit):
    rc.check_extremes(hip_kit, n)


@pytest.mark.gpu
def test_hip_extremes_refuse_empty(hip_kit):
    rc.check_extremes_refuse_empty(hip_kit)


@pytest.mark.gpu
@PRECIPITATION
def test_hip_flag_precipitated(n_dims, length, hip_kit):
    rc.check_flag_precipitated(hip_kit, n_dims, length)

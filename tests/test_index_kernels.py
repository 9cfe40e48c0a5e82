"""The index kernels where their tiles join (tests/index_cases.py): every check once against the
oracle (no marker: proves the cases and their Python / NumPy references without a GPU) and once
against the HIP library (`-m gpu`)."""
import pytest

from . import index_cases as ic


@pytest.fixture(scope="module", name="oracle_kit")
def oracle_kit_fixture(oracle_backend_class):
    return ic.Kit(oracle_backend_class)


@pytest.fixture(scope="module", name="hip_kit")
def hip_kit_fixture(hip_backend_class):
    return ic.Kit(hip_backend_class)


def _ids(cases):
    return ["-".join(str(v) for v in case) for case in cases]


LOCAL = pytest.mark.parametrize("name", ic.LOCAL_CASES)
GLOBAL = pytest.mark.parametrize("draws,length,extra", ic.GLOBAL_CASES, ids=_ids(ic.GLOBAL_CASES))
SORT = pytest.mark.parametrize("length,n_cell,order", ic.SORT_CASES, ids=_ids(ic.SORT_CASES))
COMPACT = pytest.mark.parametrize("length,n_sd,pattern", ic.COMPACT_CASES,
                                  ids=_ids(ic.COMPACT_CASES))
SORT_BY_KEY = pytest.mark.parametrize("n,order", ic.SORT_BY_KEY_CASES,
                                      ids=_ids(ic.SORT_BY_KEY_CASES))
CELL_COUNTS = pytest.mark.parametrize("n_cell", ic.CELL_COUNTS)


# ---- the oracle ---------------------------------------------------------------------------------
@LOCAL
def test_oracle_shuffle_local(name, oracle_kit):
    ic.check_shuffle_local(oracle_kit, name)


@GLOBAL
def test_oracle_shuffle_global(draws, length, extra, oracle_kit):
    ic.check_shuffle_global(oracle_kit, draws, length, extra)


@SORT
def test_oracle_counting_sort(length, n_cell, order, oracle_kit):
    ic.check_counting_sort(oracle_kit, length, n_cell, order)


@COMPACT
def test_oracle_remove_zero(length, n_sd, pattern, oracle_kit):
    ic.check_remove_zero(oracle_kit, length, n_sd, pattern)


@SORT_BY_KEY
def test_oracle_sort_by_key(n, order, oracle_kit):
    ic.check_sort_by_key(oracle_kit, n, order)


@CELL_COUNTS
def test_oracle_adaptive_sdm_end(n_cell, oracle_kit):
    ic.check_adaptive_sdm_end(oracle_kit, n_cell)


# ---- the HIP library ----------------------------------------------------------------------------
@pytest.mark.gpu
@LOCAL
def test_hip_shuffle_local(name, hip_kit):
    ic.check_shuffle_local(hip_kit, name)


@pytest.mark.gpu
@GLOBAL
def test_hip_shuffle_global(draws, length, extra, hip_kit):
    ic.check_shuffle_global(hip_kit, draws, length, extra)


@pytest.mark.gpu
@SORT
def test_hip_counting_sort(length, n_cell, order, hip_kit):
    ic.check_counting_sort(hip_kit, length, n_cell, order)


@pytest.mark.gpu
@COMPACT
def test_hip_remove_zero(length, n_sd, pattern, hip_kit):
    ic.check_remove_zero(hip_kit, length, n_sd, pattern)


@pytest.mark.gpu
@SORT_BY_KEY
def test_hip_sort_by_key(n, order, hip_kit):
    ic.check_sort_by_key(hip_kit, n, order)


@pytest.mark.gpu
@CELL_COUNTS
def test_hip_adaptive_sdm_end(n_cell, hip_kit):
    ic.check_adaptive_sdm_end(hip_kit, n_cell)

"""The pair kernels' tile-by-tile block order and k_pair_all_sort's first look-up from LDS
(SDM_OPT_WALK_LOCAL = 0, the default) and the grid order with every look-up from global memory
(= 1) against the oracle, bit for bit, where the block map changes shape: fewer workgroups than
one group of 8 tiles, exactly one group, a group plus an identity tail, lengths that shrink through
group and tile boundaries, the 256-thread kernels (8 workgroups per 4096-event tile, 32 per
16384-event tile), the colliding-pair lists of the breakup route, and the multi-cell generic route,
which the map must leave alone.  The map itself is checked on the host for every shape in use."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

from pysdm_amd import abi
from pysdm_amd.cases import make_box

pytestmark = pytest.mark.gpu

SDM_OPT_NO_PRESORT, SDM_OPT_WALK_LOCAL = 4, 6

# two tiles (no complete group of 8) | exactly one group | a group, an identity tail and a last
# tile of 2 positions | three groups less 3 positions | two groups and 5 positions
SIZES = [8190, 2**15, 2**15 + 4096 + 2, 3 * 2**15 - 3, 2**16 + 5]
CHUNKS = (1, 6, 3)  # `run(6)`: five steps whose tile sort rode in the pair kernel before


def run(runner, chunks):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for steps in chunks:
            runner.run(steps)
    return runner.snapshot()


def assert_same(a, b):
    length = int(a["length"])
    assert length == int(b["length"])
    for key, value in a.items():
        ref = b[key]
        if key == "idx":
            value, ref = value[:length], ref[:length]
        np.testing.assert_array_equal(value, ref, err_msg=key)


@functools.lru_cache(maxsize=None)
def expected(name, n_sd, adaptive, thin, chunks):
    """the oracle's result, computed once per case and shared (read only)"""
    from oracle.engine import OracleEngine  # pylint: disable=import-outside-toplevel

    return run(box(OracleEngine.get(), name, n_sd, adaptive, thin), chunks)


def box(engine, name, n_sd, adaptive, thin):
    return make_box(engine, name, n_sd=n_sd, adaptive=adaptive, thin=thin,
                    dt=200.0 if thin else None)


def both_orders(hip_engine, name, n_sd, adaptive, thin, chunks, no_presort=0):
    """the HIP run with SDM_OPT_WALK_LOCAL at 0 and at 1 (both options restored)"""
    ref = expected(name, n_sd, adaptive, thin, chunks)
    try:
        hip_engine.call("sdm_ctx_set_option", SDM_OPT_NO_PRESORT, no_presort)
        for value in (0, 1):
            hip_engine.call("sdm_ctx_set_option", SDM_OPT_WALK_LOCAL, value)
            assert_same(run(box(hip_engine, name, n_sd, adaptive, thin), chunks), ref)
    finally:
        hip_engine.call("sdm_ctx_set_option", SDM_OPT_WALK_LOCAL, 0)
        hip_engine.call("sdm_ctx_set_option", SDM_OPT_NO_PRESORT, 0)
    return ref


@pytest.mark.parametrize("n_sd", SIZES)
def test_pair_all_sort(n_sd, hip_engine):
    """one cell, non-adaptive, several steps per call: k_pair_all_sort, two workgroups per tile"""
    ref = both_orders(hip_engine, "shima", n_sd, False, None, CHUNKS)
    assert ref["collision_rate"].sum() > 0


@pytest.mark.parametrize("n_sd", SIZES)
def test_pair_all_sort_shrinking(n_sd, hip_engine):
    """multiplicities of 1..3: the length falls through group and tile boundaries while the build's
    prologue compacts and sorts again"""
    ref = both_orders(hip_engine, "shima", n_sd, False, 0.02, CHUNKS)
    assert int(ref["length"]) < n_sd


@pytest.mark.parametrize("n_sd", SIZES)
def test_pair_all(n_sd, hip_engine):
    """SDM_OPT_NO_PRESORT: k_pair_all, 256-thread workgroups, 8 per tile"""
    both_orders(hip_engine, "shima", n_sd, False, None, CHUNKS, no_presort=1)


def test_pair_prob_with_pair_lists(hip_engine):
    """adaptive with breakup: k_pair_prob in block order, k_pair_update and the colliding-pair
    lists by pair slot"""
    ref = both_orders(hip_engine, "berry_breakup", 2**15 + 4096 + 2, None, None, (3,))
    assert ref["collision_rate"].sum() > 0


def test_large_tile(hip_engine):
    """successor words from tiles of 16384 events: 32 workgroups of k_pair_prob per tile"""
    both_orders(hip_engine, "shima", 2**20 + 4096 + 3, True, None, (3,))


def test_cells_above_the_cell_kernels_capacity(hip_engine, oracle_engine):
    """2 x 2 cells of ~8000: the multi-cell generic route, where the pair kernels do not walk and
    the block order stays the grid's"""
    n_sd = 4 * 8000 + 3

    def snap(engine):
        runner = make_box(engine, "shima", n_sd=n_sd, adaptive=False, grid=(2, 2))
        sizes = np.diff(runner.snapshot()["cell_start"])
        assert len(sizes) == 4 and sizes.min() > 6144
        return run(runner, (1, 5, 2))
    ref = snap(oracle_engine)
    assert ref["collision_rate"].sum() > 0
    try:
        for value in (0, 1):
            hip_engine.call("sdm_ctx_set_option", SDM_OPT_WALK_LOCAL, value)
            assert_same(snap(hip_engine), ref)
    finally:
        hip_engine.call("sdm_ctx_set_option", SDM_OPT_WALK_LOCAL, 0)


@pytest.mark.parametrize("g", [2, 8, 32])
def test_block_map(g, hip_engine):  # pylint: disable=unused-argument
    """a permutation of the grid for every size; in a complete group of 8 g blocks the g logical
    blocks of a tile come from physical blocks that are congruent mod 8; the tail is the identity"""
    lib = abi.hip_library().cdll
    for n_blocks in (1, 7, 8 * g - 1, 8 * g, 8 * g + 1, 3 * 8 * g + 5):
        out = (ctypes.c_int * n_blocks)()
        assert lib.sdm_debug_walk_block_map(n_blocks, g, out) == 0
        logical = np.array(out[:], dtype=np.int64)
        assert sorted(logical.tolist()) == list(range(n_blocks))
        whole = n_blocks // (8 * g) * (8 * g)
        np.testing.assert_array_equal(logical[whole:], np.arange(whole, n_blocks))
        physical = np.empty(n_blocks, dtype=np.int64)
        physical[logical] = np.arange(n_blocks)
        for tile in range(whole // g):
            of_tile = physical[tile * g:(tile + 1) * g]
            assert len(set((of_tile % 8).tolist())) == 1, (n_blocks, tile, of_tile)
            # ... and stay inside the tile's own group of 8 tiles
            assert set((of_tile // (8 * g)).tolist()) == {tile // 8}

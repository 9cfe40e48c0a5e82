"""The binned shuffle's packed events and its `loc`-only successor-word route against the oracle,
bit for bit, where the layout is at risk: lengths that end a tile or a bin after 1..5 events and
are no multiples of 4 (the tile sort stores `loc` and the packed events 16 bytes at a time),
lengths that shrink through every residue mod 4 while super-droplets die (the build's prologue
compacts and sorts again), the 16384-event tile, the record formats (which keep `jarr`), and
several cells in one build (a position without an event of its own at every cell's start).

All one-cell sizes are above the per-cell kernels' capacity (6144), so the binned shuffle runs.
That the several-step `run` calls of the first form launch k_pair_all_sort at the smallest size,
8190, follows from the launch code (fused.hip: `sort_ahead` needs one cell off the per-cell route,
as many tiles as bins - 2 and 2 - and a following step); the kernel trace that was to confirm it
(rocprofv3 --kernel-trace on a run of 1 + 6 + 3 steps at 8190) has NOT been taken: no MI355X run
of this file exists yet (profiles/README.md, round 6)."""
import warnings

import numpy as np
import pytest

from pysdm_amd.cases import make_box

pytestmark = pytest.mark.gpu

SDM_OPT_REC_FORMAT, SDM_OPT_NO_PRESORT = 3, 4

# odd or not multiples of 4; the last tile / bin holds 1..5 positions or lacks 2..3
EDGE_SIZES = [8190, 8193, 3 * 4096 + 2, 2**16 - 3, 2**16 + 5]


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


def both_ways(hip_engine, option, expected, make):
    """the HIP run with `option` off and on (restored to off)"""
    try:
        for value in (0, 1):
            hip_engine.call("sdm_ctx_set_option", option, value)
            assert_same(run(make(hip_engine), CHUNKS), expected)
    finally:
        hip_engine.call("sdm_ctx_set_option", option, 0)


CHUNKS = (1, 6, 3)  # `run(6)`: five steps whose tile sort was done by the step before


@pytest.mark.parametrize("n_sd", EDGE_SIZES)
def test_lengths_at_tile_and_bin_edges(n_sd, hip_engine, oracle_engine):
    """one cell, non-adaptive, several steps per call: the sort rides in the pair kernel
    (k_pair_all_sort) and, with SDM_OPT_NO_PRESORT, runs on its own (k_bin_sort) - same format"""
    def make(engine):
        return make_box(engine, "shima", n_sd=n_sd, adaptive=False)
    expected = run(make(oracle_engine), CHUNKS)
    assert expected["collision_rate"].sum() > 0
    both_ways(hip_engine, SDM_OPT_NO_PRESORT, expected, make)


@pytest.mark.parametrize("n_sd", EDGE_SIZES)
def test_lengths_shrinking_through_every_residue(n_sd, hip_engine, oracle_engine):
    """the same with multiplicities of 1..3: super-droplets die in every step, the build's
    prologue compacts and sorts again for the new length, in the packed format"""
    def make(engine):
        return make_box(engine, "shima", n_sd=n_sd, adaptive=False, dt=200.0, thin=0.02)
    expected = run(make(oracle_engine), CHUNKS)
    assert int(expected["length"]) < n_sd - 8
    both_ways(hip_engine, SDM_OPT_NO_PRESORT, expected, make)


@pytest.mark.parametrize("n_sd,adaptive,thin", [
    (2**20 + 4096 + 3, True, None),   # successor words from tiles of 16384 events
    (2**16 + 5, False, None),
    (2**16 + 5, False, 0.02),
    (2**15 + 1, True, 0.02),
])
def test_record_formats_and_the_large_tile(n_sd, adaptive, thin, hip_engine, oracle_engine):
    """successor words (as is) and, with SDM_OPT_REC_FORMAT = records, the packed records built
    from the same packed events with `jarr` still in use"""
    def make(engine):
        return make_box(engine, "shima", n_sd=n_sd, adaptive=adaptive, thin=thin,
                        dt=(50.0 if adaptive else 200.0) if thin else None)
    chunks = (3,) if n_sd > 2**20 else CHUNKS
    expected = run(make(oracle_engine), chunks)
    if thin:
        assert int(expected["length"]) < n_sd
    try:
        for value in (0, 1):
            hip_engine.call("sdm_ctx_set_option", SDM_OPT_REC_FORMAT, value)
            assert_same(run(make(hip_engine), chunks), expected)
    finally:
        hip_engine.call("sdm_ctx_set_option", SDM_OPT_REC_FORMAT, 0)


@pytest.mark.parametrize("name,adaptive,thin", [("shima", False, None), ("shima", True, None),
                                                ("shima", True, 0.02),
                                                ("kinematic2d", True, None)])
def test_cells_above_the_cell_kernels_capacity(name, adaptive, thin, hip_engine, oracle_engine):
    """2 x 2 cells of ~8000 super-droplets (uniform-random cell ids): too large for the per-cell
    kernels, so all four go through one binned build, where the first position of every cell -
    not only position 0 - has no event of its own"""
    n_sd = 4 * 8000 + 3
    snaps = []
    for engine in (hip_engine, oracle_engine):
        runner = make_box(engine, name, n_sd=n_sd, adaptive=adaptive, grid=(2, 2), thin=thin,
                          dt=200.0 if thin else None)
        # (for both engines: reading cell_start sorts by cell, at the same point of both histories)
        sizes = np.diff(runner.snapshot()["cell_start"])
        assert len(sizes) == 4 and sizes.min() > 6144
        snaps.append(run(runner, (1, 5, 2)))
    assert snaps[1]["collision_rate"].sum() > 0
    assert_same(snaps[0], snaps[1])
    if thin:
        assert int(snaps[0]["length"]) < n_sd

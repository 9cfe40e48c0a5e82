"""Tags beside the 32-bit ids between the steps of one call (pysdm_amd/csrc/pair_tag.h), against the
oracle, bit for bit.

Inside a call of several steps (one cell, non-adaptive, Golovin, no breakup, n_sd < 2^21)
k_pair_all_sort<Golovin> writes nine bits of bounds on {multiplicity, mass} beside each id; the
next build carries them to the walks' ends, and the next pair kernel decides the pairs whose order
is known from the classes and that cannot collide without gathering their state.  The chunks
(1, 2, 6, 3) give a call that never tags, and calls that go untagged -> tagged, tagged -> tagged and
tagged -> untagged.  The thinned box loses super-droplets inside the calls (the prologue compacts
tagged words, the dead tail is copied in all width combinations); the spread box has
multiplicities over several octaves that are no halvings of the largest, and a time step at which
the collision test goes both ways inside a wavefront.

Control word 6 of the population holds, after a call whose steps carried tags, the pairs of
tagged steps that skipped the gather (low 32 bits) and that gathered (high 32 bits): no case
passes with the tags idle.  The share asserted for the default box, 0.8, is what
tests/test_pair_tag_model.py confirms with the CPU model on the same boxes.
"""
import functools
import warnings

import numpy as np
import pytest

from pysdm_amd import recipe as R
from pysdm_amd.cases import make_box
from pysdm_amd.collisions import CollisionRunner
from pysdm_amd.population import Population

SDM_OPT_REC_FORMAT, SDM_OPT_NO_PRESORT, SDM_OPT_NARROW_STEP, SDM_OPT_PAIR_TAGS = 3, 4, 7, 8

SIZES = [7, 4097, 4099, 8190, 8193, 12290, 2**16 + 5]
CHUNKS = (1, 2, 6, 3)
THIN = 0.02
NO_ROOM = 2**21 + 3  # bit_length 22: eight free bits in a terminal word


def spread_box(engine, n_sd=8193, dt=2000.0):
    """multiplicities log-uniform over five octaves below 9e6 + 1 (none a halving of the
    largest but by accident), volumes of the Shima box; dt such that the bound of the probability
    lies on both sides of the draws"""
    rng = np.random.default_rng(5)
    multiplicity = np.floor((9e6 + 1) * 2.0 ** (-5 * rng.random(n_sd))).astype(np.int64)
    multiplicity[0] = 9_000_001
    radius = 30.531e-6
    volume = rng.exponential(4 / 3 * np.pi * radius**3, n_sd)
    population = Population(engine, multiplicity=multiplicity, volume=volume)
    setup = R.CollisionSetup.coalescence(R.Golovin(b=1.5e3), adaptive=False, seed=44)
    return CollisionRunner(population, setup, dt=dt, dv=1e6 * n_sd / 2**20, route="fused")


def box(engine, kind, n_sd):
    if kind == "spread":
        return spread_box(engine, n_sd)
    if kind == "thin":
        return make_box(engine, "shima", n_sd=n_sd, adaptive=False, thin=THIN, dt=200.0)
    if kind == "adaptive":
        return make_box(engine, "shima", n_sd=n_sd, adaptive=True)
    if kind == "breakup":
        return make_box(engine, "berry_breakup", n_sd=n_sd)
    return make_box(engine, "shima", n_sd=n_sd, adaptive=False)


def run(runner, chunks, counts=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for steps in chunks:
            runner.run(steps)
            if counts is not None:
                word = int(runner.engine.download(runner.population.ctl)[6])
                counts.append((word & 0xFFFFFFFF, word >> 32))
                runner.population.ctl[6] = 0
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
def expected(kind, n_sd, chunks):
    """the oracle's result, computed once per case and shared (read only)"""
    from oracle.engine import OracleEngine  # pylint: disable=import-outside-toplevel

    return run(box(OracleEngine.get(), kind, n_sd), chunks)


def tagged_pairs(n_sd, chunks):
    """pairs of the steps that both read and write tags, per call, for a box that loses nobody:
    the interior steps of a call"""
    return [max(steps - 2, 0) * (n_sd // 2) for steps in chunks]


@pytest.mark.gpu
@pytest.mark.parametrize("n_sd", SIZES)
def test_default_box(n_sd, hip_engine):
    """nearly every pair skips the gather"""
    counts = []
    result = run(box(hip_engine, "shima", n_sd), CHUNKS, counts)
    assert_same(result, expected("shima", n_sd, CHUNKS))
    print("skipped, gathered per call:", counts)
    for (skipped, gathered), pairs in zip(counts, tagged_pairs(n_sd, CHUNKS)):
        assert skipped + gathered == pairs
        assert skipped >= 0.8 * pairs


@pytest.mark.gpu
@pytest.mark.parametrize("n_sd", SIZES)
def test_thinned_box(n_sd, hip_engine):
    """multiplicities 1..3: super-droplets die inside the calls, tagged words are compacted"""
    ref = expected("thin", n_sd, CHUNKS)
    assert int(ref["length"]) < n_sd
    counts = []
    assert_same(run(box(hip_engine, "thin", n_sd), CHUNKS, counts), ref)
    print("skipped, gathered per call:", counts)
    assert counts[0] == (0, 0) and counts[1] == (0, 0)
    if n_sd > 7:
        assert counts[2][0] > 0 and counts[2][1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_sd", [4099, 8193])
def test_spread_box(n_sd, hip_engine):
    """the order by class, equal classes without `ex` gather, the collision test both ways"""
    ref = expected("spread", n_sd, CHUNKS)
    assert ref["multiplicity"].min() >= 0
    counts = []
    assert_same(run(box(hip_engine, "spread", n_sd), CHUNKS, counts), ref)
    print("skipped, gathered per call:", counts)
    for call in (2, 3):
        assert counts[call][0] > 0 and counts[call][1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["shima", "thin", "spread"])
@pytest.mark.parametrize("option", [SDM_OPT_PAIR_TAGS, SDM_OPT_NARROW_STEP, SDM_OPT_NO_PRESORT,
                                    SDM_OPT_REC_FORMAT])
def test_switches(option, kind, hip_engine):
    """the option off, wide steps, no ride-along sort, records: no tags, the same results"""
    n_sd = 8193
    ref = expected(kind, n_sd, CHUNKS)
    counts = []
    try:
        hip_engine.call("sdm_ctx_set_option", option, 1)
        assert_same(run(box(hip_engine, kind, n_sd), CHUNKS, counts), ref)
    finally:
        hip_engine.call("sdm_ctx_set_option", option, 0)
    assert all(c == (0, 0) for c in counts), counts


@pytest.mark.gpu
@pytest.mark.parametrize("kind,chunks", [("breakup", (3,)), ("adaptive", CHUNKS)])
def test_routes_that_do_not_change(kind, chunks, hip_engine):
    n_sd = 8193
    ref = expected(kind, n_sd, chunks)
    counts = []
    assert_same(run(box(hip_engine, kind, n_sd), chunks, counts), ref)
    assert all(c == (0, 0) for c in counts), counts


@pytest.mark.gpu
def test_no_room_for_nine_bits(hip_engine):
    """n_sd of 22 bits: the narrow step stays, the tags do not"""
    chunks = (3,)
    ref = expected("shima", NO_ROOM, chunks)
    counts = []
    assert_same(run(box(hip_engine, "shima", NO_ROOM), chunks, counts), ref)
    assert counts == [(0, 0)]

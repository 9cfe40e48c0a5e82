"""The steady-state collision step with a 32-bit permutation between the steps of one call,
against the oracle, bit for bit.

Inside a call of several steps (one cell, non-adaptive) the pair kernel that sorts the next step's
events (k_pair_all_sort) leaves the permutation as int32_t ids; the next build, the compaction in
its prologue and the dead-tail copy of the next pair kernel read that form, and the last step of
the call (k_pair_all) writes int64_t again.  The chunks (1, 2, 6, 3) give a call that never goes
narrow, one that is wide -> narrow, narrow -> wide only, and longer ones with narrow -> narrow
steps.  The thinned cases lose super-droplets inside the calls, so the prologue compacts and
re-sorts the narrow buffer, the dead tail is copied in all three width combinations and the
`n_sd` flag is written in the narrow form.  The routes that stay wide run beside them: adaptive
steps (k_bin_sort with tiles of 4096 events and, above 2^20 positions, of 16384:
shuffle_binned_async takes the large tile from 257 bins on, where the ride-along route ends -
2^20 + 1 is the smallest such size), breakup, and the ride-along sort switched off.  (The 16-bit
`loc` these cases were also meant for was measured and taken out: profiles/README.md, round 9.)"""
import functools
import warnings

import numpy as np
import pytest

from pysdm_amd.cases import make_box

SDM_OPT_REC_FORMAT, SDM_OPT_NO_PRESORT, SDM_OPT_NARROW_STEP = 3, 4, 7

# fewer positions than one group of four | a last tile of 1 and 3 positions | two bins less 2,
# plus 1 | three bins plus 2 | sixteen bins plus 5
SIZES = [7, 4097, 4099, 8190, 8193, 12290, 2**16 + 5]
CHUNKS = (1, 2, 6, 3)
THIN = 0.02
BIG_TILE = 2**20 + 1  # 257 bins: the smallest size with 16384-event tiles


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


def box(engine, name, n_sd, adaptive, thin):
    return make_box(engine, name, n_sd=n_sd, adaptive=adaptive, thin=thin,
                    dt=200.0 if thin else None)


@functools.lru_cache(maxsize=None)
def expected(name, n_sd, adaptive, thin, chunks):
    """the oracle's result, computed once per case and shared (read only)"""
    from oracle.engine import OracleEngine  # pylint: disable=import-outside-toplevel

    return run(box(OracleEngine.get(), name, n_sd, adaptive, thin), chunks)


@functools.lru_cache(maxsize=None)
def thinned_lengths(n_sd):
    """the oracle stepped one step at a time through CHUNKS: the live length after every step,
    one tuple per call"""
    from oracle.engine import OracleEngine  # pylint: disable=import-outside-toplevel

    runner = box(OracleEngine.get(), "shima", n_sd, False, THIN)
    calls = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for steps in CHUNKS:
            after = []
            for _ in range(steps):
                runner.run(1)
                after.append(int(runner.snapshot()["length"]))
            calls.append(tuple(after))
    return tuple(calls)


@pytest.mark.gpu
@pytest.mark.parametrize("n_sd", SIZES)
def test_non_adaptive(n_sd, hip_engine):
    ref = expected("shima", n_sd, False, None, CHUNKS)
    assert_same(run(box(hip_engine, "shima", n_sd, False, None), CHUNKS), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n_sd", SIZES)
def test_shrinking(n_sd, hip_engine):
    """multiplicities of 1..3: super-droplets die inside the calls"""
    ref = expected("shima", n_sd, False, THIN, CHUNKS)
    assert int(ref["length"]) < n_sd
    assert_same(run(box(hip_engine, "shima", n_sd, False, THIN), CHUNKS), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("thin", [None, THIN])
@pytest.mark.parametrize("option", [SDM_OPT_REC_FORMAT, SDM_OPT_NO_PRESORT, SDM_OPT_NARROW_STEP])
def test_options(option, thin, hip_engine):
    """records instead of successor words (the narrow permutation applies, `jarr` is written
    instead of `loc`); no ride-along sort (the route stays wide); the new option off (the
    parent's widths)"""
    n_sd = 8193
    ref = expected("shima", n_sd, False, thin, CHUNKS)
    try:
        hip_engine.call("sdm_ctx_set_option", option, 1)
        assert_same(run(box(hip_engine, "shima", n_sd, False, thin), CHUNKS), ref)
    finally:
        hip_engine.call("sdm_ctx_set_option", option, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_sd", [8193, 2**16 + 5])
def test_adaptive(n_sd, hip_engine):
    """k_bin_sort and the build on every sub-step, int64_t throughout"""
    ref = expected("shima", n_sd, True, None, CHUNKS)
    assert_same(run(box(hip_engine, "shima", n_sd, True, None), CHUNKS), ref)


@pytest.mark.gpu
def test_adaptive_large_tile(hip_engine):
    """tiles of 16384 events, a last tile of one position"""
    ref = expected("shima", BIG_TILE, True, None, (2,))
    assert_same(run(box(hip_engine, "shima", BIG_TILE, True, None), (2,)), ref)


@pytest.mark.gpu
def test_breakup(hip_engine):
    ref = expected("berry_breakup", 8193, None, None, (3,))
    assert ref["collision_rate"].sum() > 0
    assert_same(run(box(hip_engine, "berry_breakup", 8193, None, None), (3,)), ref)


def test_thinned_cases_lose_droplets_where_it_matters():
    """what keeps the thinned cases honest (the oracle alone, one step at a time through the same
    chunks): every size ends shorter than it began; over all sizes the length fell in the first
    step of a multi-step call (wide in, narrow out, flagged narrow), in an interior step (narrow
    both ways) and in the last step (narrow in, wide out); and the lengths the narrow builds start
    from - the length after the step before, within a call - cover every residue mod 4"""
    fell = {"first": False, "interior": False, "last": False}
    residues = set()
    for n_sd in SIZES:
        calls = thinned_lengths(n_sd)
        assert calls[-1][-1] < n_sd, n_sd
        assert calls[-1][-1] == int(expected("shima", n_sd, False, THIN, CHUNKS)["length"]), n_sd
        before = n_sd
        for after in calls:
            for k, length in enumerate(after):
                if len(after) > 1 and length < before:
                    where = "first" if k == 0 else ("last" if k == len(after) - 1 else "interior")
                    fell[where] = True
                if k > 0:
                    residues.add(before % 4)  # step k's build reads the narrow form
                before = length
    assert all(fell.values()), fell
    assert residues == {0, 1, 2, 3}

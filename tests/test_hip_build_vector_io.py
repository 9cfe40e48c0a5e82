"""k_bin_build2<SDM_REC_CHAIN> with position-major records in LDS, four consecutive positions per
thread at the end and 16-byte stores of first / tsucc, against the oracle, bit for bit, where
groups of four and 16-byte stores meet an edge: a last bin of 1, 2 and 3 positions, lengths just below and above two
and three bins, the sizes where the pair kernels' block map changes shape, and a box smaller than
two groups.  Each size runs non-adaptive (the build after a tile sort that rode in the pair
kernel), thinned (the build's prologue compacts and sorts again while the length falls through
every residue mod 4) and adaptive (k_bin_sort + build every sub-step)."""
import functools
import warnings

import numpy as np
import pytest

from pysdm_amd.cases import make_box

# a last bin of 1..3 positions | two bins less 2, plus 1 | three bins plus 2 | nine bins plus 2 |
# sixteen bins plus 5 | fewer positions than two groups of four
SIZES = [4097, 4098, 4099, 8190, 8193, 12290, 2**15 + 4096 + 2, 2**16 + 5, 7]
CHUNKS = (1, 6, 3)
THIN = 0.02


def run(runner, chunks, lengths=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for steps in chunks:
            runner.run(steps)
            if lengths is not None:
                lengths.append(int(runner.snapshot()["length"]))
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
    """the oracle's result and its lengths at the chunk ends, computed once per case and shared
    (read only)"""
    from oracle.engine import OracleEngine  # pylint: disable=import-outside-toplevel

    lengths = []
    snap = run(box(OracleEngine.get(), name, n_sd, adaptive, thin), chunks, lengths)
    return snap, tuple(lengths)


@pytest.mark.gpu
@pytest.mark.parametrize("n_sd", SIZES)
def test_non_adaptive(n_sd, hip_engine):
    ref, _ = expected("shima", n_sd, False, None, CHUNKS)
    assert_same(run(box(hip_engine, "shima", n_sd, False, None), CHUNKS), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n_sd", SIZES)
def test_shrinking(n_sd, hip_engine):
    """multiplicities of 1..3: super-droplets die, the build's prologue runs"""
    ref, _ = expected("shima", n_sd, False, THIN, CHUNKS)
    assert int(ref["length"]) < n_sd
    assert_same(run(box(hip_engine, "shima", n_sd, False, THIN), CHUNKS), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n_sd", SIZES)
def test_adaptive(n_sd, hip_engine):
    ref, _ = expected("shima", n_sd, True, None, CHUNKS)
    assert_same(run(box(hip_engine, "shima", n_sd, True, None), CHUNKS), ref)


@pytest.mark.gpu
def test_breakup(hip_engine):
    ref, _ = expected("berry_breakup", 8193, None, None, (3,))
    assert ref["collision_rate"].sum() > 0
    assert_same(run(box(hip_engine, "berry_breakup", 8193, None, None), (3,)), ref)


def test_shrinking_lengths_cover_every_residue():
    """what keeps the shrinking cases honest (the oracle alone): every one of them loses
    super-droplets, and the lengths the builds run at end in every residue mod 4"""
    residues = set()
    for n_sd in SIZES:
        ref, lengths = expected("shima", n_sd, False, THIN, CHUNKS)
        assert int(ref["length"]) < n_sd, n_sd
        residues.update(length % 4 for length in lengths)
    assert residues == {0, 1, 2, 3}

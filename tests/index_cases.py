"""The index kernels (shuffle_local, shuffle_global, the counting sort by cell, the compaction
remove_zero_n_or_flagged, sort_by_key, adaptive_sdm_end) at the shapes where their tiles join,
written once and run with the oracle backend (CPU) and the HIP backend (GPU).  The references are
plain Python / NumPy restatements of the reference's serial algorithms, computed here; the oracle is
a second system under test, not the reference.  Every quantity is an integer (permutations, lengths,
cell_start): every comparison is assert_array_equal.

Contract on the shuffle's inputs.  The HIP kernels clamp a target into its cell (memory safety); the
reference and the oracle do not.  In double arithmetic lo + u * (hi - lo) rounds up to hi for a u
within a few ulp of 1 (u = nextafter(1, 0), lo = 23490, hi - lo = 8191 does), so "the last slot" is
drawn with u = 1 - 2^-20 and every case asserts on the host that all its targets lie in
[lo, hi - 1] (global: j <= i) - a difference could otherwise be a legitimate one.

Constants of the kernels and the case that crosses each (a change of a constant shows here which
case has to move):

  constant                      where                       crossed by
  BIN_POS = 4096                shuffle_build.h:16          local A (cell == one bin, cell edges on
                                                            bin edges, a cell over four bins), local
                                                            B 4095 / 4096 / 4097 / 8191 / 8193 /
                                                            12289
  EV_TILE = 4096                shuffle_build.h:21          the same cases (events of one tile for
                                                            several bins: the 12293- and the
                                                            8191-cell of A, B from 4097 on)
  BIN_THREADS = 1024 bins per   shuffle_build.h:238         local D (1027 bins and event tiles: two
  round of the bin scan, tiles  index.hip:968, :1019        rounds per thread in the scan, and in
  per round of the gathering                                k_bin_build2's walk over the tiles)
  2 inline hit slots, then the  index.hip:928 (SLOTS),      local A: 0, 1, 2 and 3 hits planted in
  overflow list                 index.hip:111-113 (global)  the 64-cell, 2999 on one slot (u01 = 0),
                                                            8190 on a last slot; global 6000 with
                                                            u01 = 0
  SDM_BLOCK * SHUF_ELEMS = 1024 index.hip:54                global 1023 / 1024 / 1025 / 4097 / 20001
  positions per build workgroup
  SORT_TILE = 1024              index.hip:1483              sort 1023 / 1024 / 1025, 4999
  SORT_UNROLL = 4 (x 64)        index.hip:1506              sort 255 / 256 / 257
  1024 cells per scan chunk     index.hip:1582              sort 4999 with 1024 / 1025 / 2049 cells
  1024 tiles per round of the   index.hip:1557              sort 2^20 + 1025 with 7 cells (1026
  column scan                                               tiles)
  H below 64 Mi entries, else   index.hip:1665              sort 2^20 + 1 with 65537 cells (1023
  the tile doubles                                          rows allowed, 1025 needed: tile 2048)
  64 positions per compaction   index.hip:569 (SDM_WAVE)    compaction 63 / 64 / 65
  tile
  2048 wavefront chunks         index.hip:586, :751         compaction 2^17 + 65 (2050 tiles: two
  (128 workgroups of 1024;                                  per wavefront, the last wavefronts idle)
  COMPACT_WAVES is the table)
  COMPACT_UNROLL = 8            index.hip:676               compaction 2^20 + 2^17 + 37 (10 tiles
                                                            per wavefront: a full round and a masked
                                                            one)
  SDM_BLOCK = 256 keys per      index.hip:519               sort_by_key 255 / 256 / 257 / 1025 /
  round of a rank count                                     9216
  64 cells per ballot           collisions.hip:337          adaptive_sdm_end: last entry at 0, 255,
                                                            256, n_cell - 1

What was tried against these cases.  Edits of the oracle, one at a time, and the checks that then
fail: equal keys of the counting sort emitted in reverse, or the cell_start prefix one cell short -
every counting-sort case; fillers of the compaction taken ascending - every pattern with two holes
to fill (not `none`, `all`, `tail_only`, nor one dead position); ties of sort_by_key in ascending
index order - `equal` from 2 keys, `ties` from 255; global target int(u * i) - every `random` case
and `last` (no longer the identity); the local target of a cell's first event over the previous
cell's size - A, C, D.
Edits of index.hip that keep every index in range: k_sort_cellstart keeping only the last chunk's
carry - the 1025-, 2049- and 65537-cell sorts and no other; k_sort_colscan with one round per
thread - the four sorts of 2^20 + 1025 and no other; k_bin_build2 gathering only the first 1024
event tiles - local D and no other.
"""
import functools

import numpy as np

from .micro_cases import Kit  # noqa: F401  pylint: disable=unused-import

LAST_SLOT = 1 - 2.0**-20  # "u01 = 1" that stays inside the cell (see above)
BIN_POS = 4096


class Case:  # pylint: disable=too-few-public-methods
    """host arrays of one case (read-only: shared between the oracle and the HIP test)"""

    def __init__(self, **members):
        for name, value in members.items():
            if isinstance(value, np.ndarray):
                value.setflags(write=False)
            setattr(self, name, value)


# ---- shuffle_local --------------------------------------------------------------------------
LOCAL_A_SIZES = (4096, 0, 1, 4095, 1, 0, 0, 3 * 4096 + 5, 2, 3000, 1, 1, 8191, 64, 37)
LOCAL_A_EXTRA = 11
# offsets inside the 64-cell and the number of events that hit them
LOCAL_A_PLANTED = ((9, 0), (40, 1), (17, 2), (5, 3), (0, 3))
LOCAL_B_LENGTHS = (2, 3, 4095, 4096, 4097, 8191, 8193, 3 * 4096 + 1)
LOCAL_B_CASES = tuple((length, extra) for length in LOCAL_B_LENGTHS for extra in (0, 5))
LOCAL_D_N = 2**22 + 2 * 4096 + 10
# (first position, size) of the larger cells of D, all even: the first lies over bins 1023 - 1025,
# the second in the last, partial bin; then one that is exactly a bin, and nine anywhere
LOCAL_D_LARGE = ((1023 * BIN_POS + 4000, 96 + BIN_POS + 100), (LOCAL_D_N - 8, 8),
                 (500 * BIN_POS, BIN_POS), (4000, 3000), (350002, 2500), (700000, 1000),
                 (1050000, 6000), (1400000, 514), (1750000, 130), (2100000, 66), (2450000, 5000),
                 (2800000, 3500))
LOCAL_CASES = ("A", "C", "D") + tuple(f"B-{length}-{extra}" for length, extra in LOCAL_B_CASES)


def local_targets(u01, cell_start):
    """j of every position's own event, -1 where it has none (the first slot of its cell), as the
    reference computes it: int(lo + u * (hi - lo)) in float64.  Asserts the contract above"""
    sizes = np.diff(cell_start)
    lo = np.repeat(cell_start[:-1], sizes)
    width = np.repeat(sizes, sizes)
    length = int(cell_start[-1])
    j = (lo.astype(np.float64) + u01[:length] * width.astype(np.float64)).astype(np.int64)
    own = np.arange(length) > lo
    assert ((j >= lo) & (j <= lo + width - 1))[own].all(), "a target outside its cell"
    return np.where(own, j, -1)


def _chain(idx, u01, lo, hi):
    """index_methods.py:32-43 for one cell, on Python lists, in place"""
    width = hi - lo
    for i in range(hi - 1, lo, -1):
        j = int(lo + u01[i] * width)
        idx[i], idx[j] = idx[j], idx[i]


def shuffle_local_expected(idx0, u01, cell_start):
    idx, u01 = idx0.tolist(), u01.tolist()
    bounds = cell_start.tolist()
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        _chain(idx, u01, lo, hi)
    return np.asarray(idx, dtype=np.int64)


def shuffle_local_expected_pairs(idx0, u01, cell_start):
    """the same where nearly every cell holds two positions: a cell [lo, lo + 2) has the one event
    i = lo + 1, which swaps iff int(lo + 2 u) == lo - NumPy for those, the serial chain for the
    rest"""
    out = idx0.copy()
    sizes = np.diff(cell_start)
    assert sizes.min() >= 2
    lo = cell_start[:-1][sizes == 2]
    j = (lo.astype(np.float64) + u01[lo + 1] * 2.0).astype(np.int64)
    assert ((j == lo) | (j == lo + 1)).all()
    swap = lo[j == lo]
    out[swap], out[swap + 1] = idx0[swap + 1], idx0[swap]
    for c in np.flatnonzero(sizes > 2):
        first, last = int(cell_start[c]), int(cell_start[c + 1])
        part, draws = out[first:last].tolist(), u01[first:last].tolist()
        width = last - first
        for i in range(width - 1, 0, -1):
            j = int(first + draws[i] * width) - first
            part[i], part[j] = part[j], part[i]
        out[first:last] = part
    return out


def _local_a(rng):
    sizes = np.asarray(LOCAL_A_SIZES, dtype=np.int64)
    cell_start = np.concatenate([[0], np.cumsum(sizes)])
    length = int(cell_start[-1])
    u01 = rng.uniform(0, 1, length + LOCAL_A_EXTRA)
    first = {int(size): int(cell_start[k]) for k, size in enumerate(sizes)}
    u01[first[3000]:first[3000] + 3000] = 0.0
    u01[first[8191]:first[8191] + 8191] = LAST_SLOT
    # the 64-cell: u = (k + 1/2) / 64 sends an event to offset k exactly
    lo = first[64]
    wanted = [k for k, hits in LOCAL_A_PLANTED for _ in range(hits)]
    free = sorted(set(range(64)) - {k for k, _ in LOCAL_A_PLANTED})
    wanted += rng.choice(free, 63 - len(wanted)).tolist()
    u01[lo + 1:lo + 64] = (rng.permutation(wanted) + 0.5) / 64
    hits = np.bincount(local_targets(u01, cell_start)[lo + 1:lo + 64] - lo, minlength=64)
    for k, count in LOCAL_A_PLANTED:
        assert hits[k] == count
    all_hits = np.bincount(local_targets(u01, cell_start)[local_targets(u01, cell_start) >= 0],
                           minlength=length)
    assert all_hits[first[3000]] == 2999 and all_hits[first[8191] + 8190] == 8190
    return cell_start, u01, LOCAL_A_EXTRA


def _local_c(rng):
    sizes = np.tile([1, 2, 3], 20000 // 6 + 1)
    cell_start = np.concatenate([[0], np.minimum(np.cumsum(sizes), 20000)])
    cell_start = cell_start[:np.argmax(cell_start == 20000) + 1]
    assert len(cell_start) - 1 > 20000 // 2
    return cell_start, rng.uniform(0, 1, 20003), 3


def _local_d(rng):
    inside = np.zeros(LOCAL_D_N + 1, dtype=bool)  # boundaries a larger cell swallows
    for first, size in LOCAL_D_LARGE:
        assert first % 2 == 0 and size % 2 == 0 and not inside[first:first + size + 1].any()
        inside[first + 1:first + size] = True
    cell_start = np.flatnonzero(~inside[::2]) * 2
    assert cell_start[-1] == LOCAL_D_N and sum(s for _, s in LOCAL_D_LARGE) > 30000
    u01 = rng.uniform(0, 1, LOCAL_D_N + 6)
    u01[1:2000:4], u01[3:2000:4] = 0.0, LAST_SLOT  # (pairs that do and do not swap, for certain)
    return cell_start.astype(np.int64), u01, 6


@functools.lru_cache(maxsize=2)
def local_case(name):
    """A, C, D, or B-<length>-<extra> (one cell).  idx0 is a random permutation of all ids, the
    positions beyond the live length included"""
    rng = np.random.default_rng([1, len(name)] + [ord(ch) for ch in name])
    if name[0] == "B":
        length, extra = (int(v) for v in name.split("-")[1:])
        cell_start, u01 = np.asarray([0, length], dtype=np.int64), rng.uniform(0, 1, length + extra)
    else:
        cell_start, u01, extra = {"A": _local_a, "C": _local_c, "D": _local_d}[name](rng)
    length = int(cell_start[-1])
    idx0 = rng.permutation(length + extra).astype(np.int64)
    local_targets(u01, cell_start)
    expected = (shuffle_local_expected_pairs if name == "D" else shuffle_local_expected)(
        idx0, u01, cell_start)
    return Case(name=name, length=length, idx0=idx0, u01=u01, cell_start=cell_start,
                expected=expected)


def check_shuffle_local(kit, name):
    case = local_case(name)
    idx = kit.Index.from_ndarray(case.idx0.copy())
    kit.backend.shuffle_local(idx=idx.data, u01=kit.Storage.from_ndarray(case.u01.copy()).data,
                              cell_start=kit.Storage.from_ndarray(case.cell_start.copy()).data)
    got = idx.to_ndarray()
    np.testing.assert_array_equal(got[case.length:], case.idx0[case.length:],
                                  err_msg=f"local {name}: beyond the length")
    np.testing.assert_array_equal(got[:case.length], case.expected[:case.length],
                                  err_msg=f"local {name}")


# ---- shuffle_global -------------------------------------------------------------------------
GLOBAL_CASES = (("random", 1023, 7), ("random", 1024, 7), ("random", 1025, 0), ("random", 1025, 7),
                ("random", 4097, 7), ("random", 20001, 7), ("zero", 6000, 7), ("last", 6000, 7))


def shuffle_global_expected(idx0, u01, length):
    idx, u01 = idx0.tolist(), u01.tolist()
    for i in range(length - 1, 0, -1):
        j = int(u01[i] * (i + 1))
        idx[i], idx[j] = idx[j], idx[i]
    return np.asarray(idx, dtype=np.int64)


@functools.lru_cache(maxsize=2)
def global_case(draws, length, extra):
    rng = np.random.default_rng([2, length, extra])
    u01 = {"random": rng.uniform(0, 1, length + extra), "zero": np.zeros(length + extra),
           "last": np.full(length + extra, LAST_SLOT)}[draws]
    i = np.arange(length)
    j = (u01[:length] * (i + 1).astype(np.float64)).astype(np.int64)
    assert (j <= i).all() and (j >= 0).all(), "a target beyond its event"
    idx0 = rng.permutation(length + extra).astype(np.int64)
    expected = shuffle_global_expected(idx0, u01, length)
    if draws == "last":  # j == i: every swap a no-op
        assert (j == i).all()
        np.testing.assert_array_equal(expected, idx0)
    if draws == "zero":
        assert (j == 0).all()
    return Case(length=length, idx0=idx0, u01=u01, expected=expected)


def check_shuffle_global(kit, draws, length, extra):
    case = global_case(draws, length, extra)
    idx = kit.Index.from_ndarray(case.idx0.copy())
    idx.length = int(length)
    kit.backend.shuffle_global(idx=idx.data, length=length,
                               u01=kit.Storage.from_ndarray(case.u01.copy()).data)
    got = idx.to_ndarray()
    tag = f"global {draws} {length}"
    np.testing.assert_array_equal(got[length:], case.idx0[length:], err_msg=tag + ": the tail")
    np.testing.assert_array_equal(got[:length], case.expected[:length], err_msg=tag)


# ---- make_cell_caretaker / sdm_counting_sort_by_cell_id -------------------------------------
SORT_EXTRA = 9
SORT_ORDERS = ("random", "ascending", "descending", "one_cell")
SORT_CASES = tuple((length, 3, "random") for length in (255, 256, 257)) + tuple(
    (length, 2, "random") for length in (1023, 1024, 1025)) + (
        (4999, 1024, "random"), (4999, 2049, "random")) + tuple(
            (length, n_cell, order) for length, n_cell in ((4999, 1025), (2**20 + 1025, 7),
                                                           (2**20 + 1, 65537))
            for order in SORT_ORDERS)


def counting_sort_expected(idx, cell_id, cell_idx, length):
    keys = cell_idx[cell_id[idx[:length]]]
    counts = np.bincount(keys, minlength=len(cell_idx))
    return idx[:length][np.argsort(keys, kind="stable")], np.concatenate([[0], np.cumsum(counts)])


@functools.lru_cache(maxsize=2)
def sort_case(length, n_cell, order):
    """cell_idx a random permutation, idx a random permutation of the ids; the entries of idx beyond
    `length` hold the flag n_sd and cell_id has exactly n_sd entries: they cannot be looked up"""
    rng = np.random.default_rng([3, length, n_cell, SORT_ORDERS.index(order)])
    n_sd = length + SORT_EXTRA
    ids = rng.permutation(n_sd).astype(np.int64)
    idx = np.concatenate([ids[:length], np.full(SORT_EXTRA, n_sd, dtype=np.int64)])
    cell_idx = rng.permutation(n_cell).astype(np.int64)
    key_of_position = rng.integers(0, n_cell, length)
    if order == "ascending":
        key_of_position = np.sort(key_of_position)
    elif order == "descending":
        key_of_position = np.sort(key_of_position)[::-1]
    elif order == "one_cell":
        key_of_position = np.full(length, n_cell * 2 // 3)
    cell_of_key = np.empty(n_cell, dtype=np.int64)
    cell_of_key[cell_idx] = np.arange(n_cell)
    cell_id = rng.integers(0, n_cell, n_sd).astype(np.int64)
    cell_id[ids[:length]] = cell_of_key[key_of_position]
    new_idx, cell_start = counting_sort_expected(idx, cell_id, cell_idx, length)
    if order == "ascending":  # stability is all that is left: nothing moves
        np.testing.assert_array_equal(new_idx, idx[:length])
    return Case(length=length, n_cell=n_cell, idx=idx, cell_id=cell_id, cell_idx=cell_idx,
                new_idx=new_idx, cell_start=cell_start)


def check_counting_sort(kit, length, n_cell, order):
    case = sort_case(length, n_cell, order)
    idx = kit.Index.from_ndarray(case.idx.copy())
    idx.length = int(length)
    cell_start = kit.Storage.from_ndarray(np.full(n_cell + 1, -1, dtype=np.int64))
    caretaker = kit.backend.make_cell_caretaker(idx.shape, idx.dtype, n_cell + 1)
    caretaker(kit.Storage.from_ndarray(case.cell_id.copy()),
              kit.Index.from_ndarray(case.cell_idx.copy()), cell_start, idx)
    tag = f"sort {length} {n_cell} {order}"
    np.testing.assert_array_equal(cell_start.to_ndarray(), case.cell_start, err_msg=tag)
    np.testing.assert_array_equal(idx.to_ndarray()[:length], case.new_idx, err_msg=tag)


# ---- remove_zero_n_or_flagged ---------------------------------------------------------------
COMPACT_TILE = 64
COMPACT_WAVEFRONTS = 2048  # 128 workgroups of 1024 threads
SERIAL_MAX = 2**18  # the serial loop is the reference up to here (and checks the closed form)
COMPACT_SIZES = ((1, 6), (63, 68), (64, 69), (65, 70), (2**17 + 65, 2**17 + 100),
                 (2**20 + 2**17 + 37, 2**20 + 2**17 + 50))
COMPACT_PATTERNS = ("none", "all", "one_percent", "forty_percent", "tail_only", "first_half",
                    "boundary_dead", "boundary_alive", "multiple_of_64", "multiple_of_chunk")


def _wave_chunk(length):
    """positions a wavefront of the compaction kernel owns"""
    tiles = -(-length // COMPACT_TILE)
    return -(-tiles // COMPACT_WAVEFRONTS) * COMPACT_TILE


def _applies(pattern, length):
    if length == 1:
        return pattern in ("none", "all")
    if pattern == "multiple_of_64":
        return length > COMPACT_TILE
    if pattern == "multiple_of_chunk":  # (another multiple than 64 only)
        return _wave_chunk(length) > COMPACT_TILE
    return True


COMPACT_CASES = tuple((length, n_sd, pattern) for length, n_sd in COMPACT_SIZES
                      for pattern in COMPACT_PATTERNS if _applies(pattern, length))


def _some(rng, length, count, without=None):
    """`count` distinct positions of [0, length), none of them `without`"""
    pool = np.arange(length) if without is None else np.delete(np.arange(length), without)
    return rng.choice(pool, count, replace=False)


def _dead_positions(rng, pattern, length):  # pylint: disable=too-many-return-statements
    if pattern == "none":
        return np.empty(0, dtype=np.int64)
    if pattern == "all":
        return np.arange(length)
    if pattern == "one_percent":
        return _some(rng, length, max(length // 100, 1))
    if pattern == "forty_percent":
        return _some(rng, length, length * 2 // 5)
    if pattern == "tail_only":  # the last tenth, all of it: no holes, no fillers
        return np.arange(length - max(length // 10, 1), length)
    if pattern == "first_half":
        return _some(rng, length // 2, max(length // 20, 1))
    if pattern in ("boundary_dead", "boundary_alive"):
        count = max(length // 5, 2)
        rest = _some(rng, length, count - (pattern == "boundary_dead"), without=length - count)
        return np.append(rest, length - count) if pattern == "boundary_dead" else rest
    if pattern == "multiple_of_64":  # about three quarters, and no multiple of 128
        new = (length * 3 // 4 // COMPACT_TILE or (length - 1) // COMPACT_TILE) * COMPACT_TILE
        new -= COMPACT_TILE if new % (2 * COMPACT_TILE) == 0 and new > COMPACT_TILE else 0
        return _some(rng, length, length - new)
    if pattern == "multiple_of_chunk":
        return _some(rng, length, length - 700 * _wave_chunk(length))
    raise ValueError(pattern)


def compact_serial(idx, mult, length, flag):
    """collisions_methods.py:664-680: the swap from the end, on Python lists"""
    idx, mult = idx.tolist(), mult.tolist()
    i, end = 0, length
    while i < end:
        if idx[i] == flag or mult[idx[i]] == 0:
            end -= 1
            idx[i] = idx[end]
            idx[end] = flag
        else:
            i += 1
    return np.asarray(idx, dtype=np.int64), end


def compact_closed_form(idx, mult, length, flag):
    """the same without the loop: the r-th dead position below the new length (ascending) takes the
    r-th live element at or above it (descending); [new, length) holds the flag"""
    live = idx[:length]
    dead = live == flag
    dead[~dead] = mult[live[~dead]] == 0
    new = length - int(dead.sum())
    holes = np.flatnonzero(dead[:new])
    fillers = (new + np.flatnonzero(~dead[new:]))[::-1]
    out = idx.copy()
    out[holes] = idx[fillers]
    out[new:length] = flag
    return out, new


@functools.lru_cache(maxsize=2)
def compact_case(length, n_sd, pattern):
    """idx a permutation of all n_sd ids (the entries beyond `length` are ids too, every other one
    with multiplicity zero: they must stay as they are); of the dead positions up to five are
    flagged (idx == n_sd), the others lose their multiplicity"""
    rng = np.random.default_rng([4, length, COMPACT_PATTERNS.index(pattern)])
    idx = rng.permutation(n_sd).astype(np.int64)
    mult = rng.integers(1, 1000, n_sd).astype(np.int64)
    mult[idx[length::2]] = 0
    dead = _dead_positions(rng, pattern, length)
    assert len(np.unique(dead)) == len(dead) and (len(dead) == 0 or dead.max() < length)
    flagged = dead[rng.permutation(len(dead))[:5]]
    mult[idx[dead]] = 0
    idx[flagged] = n_sd
    want_idx, want_len = compact_closed_form(idx, mult, length, n_sd)
    assert want_len == length - len(dead)
    if length <= SERIAL_MAX:
        serial_idx, serial_len = compact_serial(idx, mult, length, n_sd)
        assert serial_len == want_len
        np.testing.assert_array_equal(want_idx, serial_idx)
    boundary = want_len < length and (idx[want_len] == n_sd or mult[idx[want_len]] == 0)
    if pattern in ("boundary_dead", "boundary_alive"):
        assert boundary == (pattern == "boundary_dead")
    if pattern == "multiple_of_64":
        assert want_len > 0 and want_len % COMPACT_TILE == 0
    if pattern == "multiple_of_chunk":
        assert want_len > 0 and want_len % _wave_chunk(length) == 0
    if pattern == "tail_only":
        np.testing.assert_array_equal(want_idx[:want_len], idx[:want_len])
    return Case(length=length, n_sd=n_sd, idx=idx, mult=mult, want_idx=want_idx, want_len=want_len)


def check_remove_zero(kit, length, n_sd, pattern):
    case = compact_case(length, n_sd, pattern)
    idx = kit.Index.from_ndarray(case.idx.copy())
    idx.length = int(length)
    mult = kit.IndexedStorage.from_ndarray(idx, case.mult.copy())
    new_length = kit.backend.remove_zero_n_or_flagged(mult.data, idx.data, length)
    got = idx.to_ndarray()
    tag = f"compaction {length} {pattern}"
    assert new_length == case.want_len, tag
    if pattern == "none":
        np.testing.assert_array_equal(got, case.idx, err_msg=tag)
    np.testing.assert_array_equal(got[length:], case.idx[length:], err_msg=tag + ": beyond length")
    assert (got[new_length:length] == n_sd).all(), tag + ": the removed tail"
    np.testing.assert_array_equal(got[:new_length], case.want_idx[:new_length], err_msg=tag)


# ---- sort_by_key / adaptive_sdm_end ---------------------------------------------------------
CELL_COUNTS = (1, 2, 255, 256, 257, 1025, 9216)
KEY_VALUES = (0.0, -0.0, 1.0, 2.5, 1e-300, np.inf)
KEY_ORDERS = ("ties", "equal", "ascending", "descending")
SORT_BY_KEY_CASES = tuple((n, order) for n in CELL_COUNTS for order in KEY_ORDERS)
LAST_POSITIVE = (0, 255, 256, "last", None)


def sort_by_key_keys(n, order):
    rng = np.random.default_rng([5, n, KEY_ORDERS.index(order)])
    if order == "ties":
        return rng.choice(KEY_VALUES, n)
    if order == "equal":
        return np.full(n, 2.5)
    keys = np.sort(rng.uniform(0, 100, n))
    return keys if order == "ascending" else keys[::-1].copy()


def check_sort_by_key(kit, n, order):
    keys = sort_by_key_keys(n, order)
    want = np.argsort(keys, kind="stable")[::-1]
    if order == "equal":  # ties keep their order under the stable sort, which is then reversed
        np.testing.assert_array_equal(want, np.arange(n)[::-1])
    cidx = kit.Index.from_ndarray(np.full(n, -7, dtype=np.int64))
    kit.backend.sort_by_key(cidx, kit.Storage.from_ndarray(keys.copy()))
    np.testing.assert_array_equal(cidx.to_ndarray(), want, err_msg=f"sort_by_key {n} {order}")


def check_adaptive_sdm_end(kit, n_cell):
    """cell_start[k + 1] for the last cell k with time left, 0 if there is none (the reference's
    loop, collisions_methods.py:313-328, starts from end = 0; k_adaptive_end counts from a zeroed
    word).  Cells may be empty; below k every second cell, at random, has time left as well"""
    rng = np.random.default_rng([6, n_cell])
    cell_start = np.concatenate([[3], 3 + np.cumsum(rng.integers(0, 4, n_cell))]).astype(np.int64)
    cell_start[-1] += 1  # (the end of the last cell differs from the end of the one before)
    d_cell_start = kit.Storage.from_ndarray(cell_start.copy())
    for place in LAST_POSITIVE:
        k = n_cell - 1 if place == "last" else place
        if k is not None and k >= n_cell:
            continue
        dt_left = np.zeros(n_cell)
        if k is not None:
            dt_left[:k] = rng.choice([0.0, 0.25, 1e-300], k)
            dt_left[k] = 1e-300 if k % 2 else 7.5
        end = kit.backend.adaptive_sdm_end(kit.Storage.from_ndarray(dt_left), d_cell_start)
        assert end == (0 if k is None else cell_start[k + 1]), (n_cell, place, end)

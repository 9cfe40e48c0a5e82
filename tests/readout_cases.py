"""The read-outs (moments, spectrum moments, Storage.amin / amax, the rainfall sum of
flag_precipitated) at the shapes where their fast paths run, written once and run with the oracle
backend (CPU) and the HIP backend (GPU).  The references are computed here with NumPy and
math.fsum; the oracle is a second system under test, not the reference.

Two tiers.  EXACT: multiplicities are integers in [1, 1000), the attribute takes the integer values
1..63, the weighting attribute 1..15, ranks come from {0, 1, 2, 3} and the weighting rank from
{0, 1}: every term and every partial sum is an integer below 1000 * 15 * 63^3 * 393217 ~ 1.5e15
< 2^53, so the sums are exact in float64 in ANY order and the comparison is assert_array_equal
(with skip_division_by_m0=False the expected value is the one quotient of two exact sums).
TOLERANCE: volumes log-uniform in [1e-16, 1e-10], mass = 1000 * volume as the weighting attribute,
ranks [1/3, 2/3, 1.5, -0.5, 3], math.fsum per cell, rtol = 1e-12 - the project's own figure for
"the order of the adds is free" (README, micro_cases.check_moments); all terms are positive.

Dead storage: n_sd = length + 101, idx is a random permutation of the ids, and every row beyond
`length` holds NaN in the attribute and weighting columns and the valid cell id 0, so a read past
`length` shows as a NaN or a wrong count, never as a fault.  The range filter compares false on
NaN and would hide such a read, so the FILTER column of every other dead row (the first one,
idx[length], included) holds a value inside the range; the others hold NaN.

Which case is there for which mistake (k_moments gives a wave one 64-position round up to
MOM_GRID * SDM_BLOCK = 131072 positions; `chunk` is 128 at 131073, 192 at 2^18 + 37 and 256 at
3 * 2^17 + 1 - two, three and four rounds):
  * the running sums a0 / acc[] are dropped in a mixed round: `sorted_ragged` at 131073 and above -
    its cell boundaries sit at offset 101 of a 256-position block, i.e. in the SECOND round of a
    wave, after a uniform one whose sums must survive;
  * the flush goes to the new cell instead of the old one: `striped` (every round uniform, every
    round another cell, cells revisited) from 131073 on, `sorted_aligned` and `sorted_ragged` at
    2^18 + 37 (a uniform round of the next cell follows the mixed one within a wave);
  * `hi < 0` (nothing in range) treated as a cell, or a skipped round losing the sums:
    `sorted_ragged_filtered` (whole rounds out of range, waves uniform only after the filter);
    131073: half the waves have no work at all;
  * with_m0 on every rank pass: any case with the five- or nine-entry rank list (two and three
    passes) - moment_0 doubles or triples;
  * `x < max_x` turned into `<=` (or `min_x <=` into `<`): the filter [2, 8) on a column of
    integers 0..9 - both bounds are attribute values;
  * a super-droplet lost or counted twice where chunks meet: 131072 / 131073 / 2^18 + 37 /
    3 * 2^17 + 1 (ragged tails, the last wave with work partly filled), 63 / 64 / 65 / 255 / 257;
  * per-lane fallback: `random`, `sorted_many` (length // 3 cells: every wave mixed);
  * the division: `one_of_five` - four cells hold nothing and must read exactly 0, all outputs
    are pre-filled with NaN;
  * spectrum scan stopping at the LAST match: the edges [4, 8, 8, 16, 12, 40, 2, 5] (overlapping
    bins, an empty one, a descending step) with x on integers 0..47; 7999 bins is the largest
    accepted number (x = 0 inside, x = 7999 outside), 8000 is refused by HIP with its outputs
    untouched;
  * k_reduce_f64 skipping elements in its grid-stride loop (a stride one too long): the extreme
    or the NaN planted at 262144, the first element only that loop sees.  (A stride one too SHORT
    still visits every element, some twice - min and max do not change, no test can see that.);
    k_reduce_final with all its 1024 threads holding a partial: n >= 262144;
  * k_fold_partials' strided loop: flag_precipitated at length 262145 = 1025 partials.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from pysdm_amd import diagnostics
from pysdm_amd.cases import make_box

from .micro_cases import MOMENTS, Kit  # noqa: F401  pylint: disable=unused-import

N_DEAD = 101
BIG = 2**18 + 37
# 131072: the last length with one round per wave; 131073: two rounds, half the waves idle;
# 3 * 2^17 + 1: `chunk` = 256, four rounds
LENGTHS = (1, 63, 64, 65, 255, 257, 1000, 131072, 131073, BIG, 3 * 2**17 + 1)
FILTER = (2.0, 8.0)  # on integers 0..9: 2 is inside, 8 is not
NO_FILTER = (-np.inf, np.inf)

RANKS_NINE = (3, 0, 2, 1, 1, 2, 0, 3, 2)
# (ranks, weighting rank, filtered, skip_division_by_m0): one pass, one full pass, two passes,
# three passes, and moment_0 alone (n_ranks = 0, moments = ranks = NULL)
EXACT_OPTIONS = (
    ((1,), 0, False, False),
    ((0, 1, 2, 3), 0, False, True),
    ((0, 1, 2, 3, 1), 1, True, True),
    (RANKS_NINE, 1, True, False),
    ((), 1, True, True),
)
TOLERANCE_RANKS = (1 / 3, 2 / 3, 1.5, -0.5, 3.0)
RTOL = 1e-12


# ---- layouts: cell of every position p of the permutation ---------------------------------------
def _boundaries(length, aligned):
    """six increasing cell boundaries in [0, length].  Ragged: where the length allows it, at
    offset 64 + 37 of a block of 256 positions - no multiple of 64, and the second 64-position
    round of a wave where its chunk is 128 or 256 (at 192 any of the three)"""
    base = np.arange(1, 7) * length // 7
    if aligned:
        return base // 64 * 64
    ragged = base // 256 * 256 + 101
    ragged = np.where(ragged < length, ragged, base)
    return np.maximum.accumulate(ragged)


def _sorted_cells(length, aligned):
    return np.searchsorted(_boundaries(length, aligned), np.arange(length), side="right"), 7


def _layout(name, length, rng):
    if name == "one":
        return np.zeros(length, dtype=np.int64), 1
    if name == "one_of_five":
        return np.full(length, 3, dtype=np.int64), 5
    if name == "sorted_aligned":
        return _sorted_cells(length, True)
    if name in ("sorted_ragged", "sorted_ragged_filtered"):
        return _sorted_cells(length, False)
    if name == "striped":
        return (np.arange(length) // 64) % 3, 3
    if name == "sorted_many":
        n_cell = max(length // 3, 1)
        return np.sort(rng.integers(0, n_cell, length)), n_cell
    if name == "random":
        return rng.integers(0, 7, length), 7
    raise ValueError(name)


LAYOUTS = ("one", "one_of_five", "sorted_aligned", "sorted_ragged", "striped", "sorted_many",
           "random", "sorted_ragged_filtered")
# every layout at 2^18 + 37; `one`, `sorted_ragged` and `striped` at every length
MOMENTS_EXACT_CASES = tuple((layout, BIG) for layout in LAYOUTS) + tuple(
    (layout, length) for layout in ("one", "sorted_ragged", "striped") for length in LENGTHS
    if length != BIG)


class State:  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """host columns of one case (read-only: shared between the checks that use them)"""

    def __init__(self, **columns):
        for name, value in columns.items():
            if isinstance(value, np.ndarray):
                value.setflags(write=False)
            setattr(self, name, value)


def _columns(rng, length, n_sd, cells):
    """idx, the ids of the dead rows, cell id by id, multiplicity"""
    ids = rng.permutation(n_sd).astype(np.int64)
    cell = np.zeros(n_sd, dtype=np.int64)
    cell[ids[:length]] = cells
    mult = rng.integers(1, 1000, n_sd).astype(np.int64)
    return ids, ids[length:], cell, mult


@functools.lru_cache(maxsize=4)
def exact_state(layout, length):
    rng = np.random.default_rng([length, LAYOUTS.index(layout)])
    n_sd = length + N_DEAD
    cells, n_cell = _layout(layout, length, rng)
    idx, dead, cell, mult = _columns(rng, length, n_sd, cells)
    attr = rng.integers(1, 64, n_sd).astype(float)
    weight = rng.integers(1, 16, n_sd).astype(float)
    x = rng.integers(0, 10, n_sd).astype(float)
    if layout == "sorted_ragged_filtered":  # odd cells: all outside [2, 8)
        odd = cell % 2 == 1
        x[odd] = rng.choice([0.0, 1.0, 8.0, 9.0], n_sd)[odd]
        x[~odd] = rng.integers(2, 8, n_sd).astype(float)[~odd]
    attr[dead], weight[dead] = np.nan, np.nan
    x[dead[0::2]], x[dead[1::2]] = 5.0, np.nan
    return State(layout=layout, length=length, n_sd=n_sd, n_cell=n_cell, idx=idx, cell=cell,
                 mult=mult, attr=attr, weight=weight, x=x)


@functools.lru_cache(maxsize=2)
def tolerance_state(layout):
    length = BIG
    rng = np.random.default_rng([77, LAYOUTS.index(layout)])
    n_sd = length + N_DEAD
    cells, n_cell = _layout(layout, length, rng)
    idx, dead, cell, mult = _columns(rng, length, n_sd, cells)
    vol = np.exp(rng.uniform(np.log(1e-16), np.log(1e-10), n_sd))
    mass = 1000 * vol
    x = vol.copy()
    vol[dead], mass[dead] = np.nan, np.nan
    x[dead[1::2]] = np.nan
    return State(layout=layout, length=length, n_sd=n_sd, n_cell=n_cell, idx=idx, cell=cell,
                 mult=mult, attr=vol, weight=mass, x=x)


# ---- references -----------------------------------------------------------------------------
def _selected(state, lo, hi):
    live = state.idx[:state.length]
    x = state.x[live]
    return live[(lo <= x) & (x < hi)]


def _divided(mom, m0):
    return np.where(m0 != 0, mom / np.where(m0 != 0, m0, 1), 0.0)


def moments_exact(state, ranks, wrank, lo, hi, skip):
    """integer arithmetic throughout (int64), converted once: exact below 2^53"""
    sel = _selected(state, lo, hi)
    cell = state.cell[sel]
    attr = state.attr[sel].astype(np.int64)
    w = state.mult[sel] * (state.weight[sel].astype(np.int64) ** int(wrank))
    m0 = np.bincount(cell, weights=w.astype(float), minlength=state.n_cell)
    mom = np.empty((len(ranks), state.n_cell))
    for k, rank in enumerate(ranks):
        mom[k] = np.bincount(cell, weights=(w * attr ** int(rank)).astype(float),
                             minlength=state.n_cell)
    assert m0.max(initial=0) < 2.0**53 and mom.max(initial=0) < 2.0**53
    return m0, mom if skip else _divided(mom, m0)


def moments_fsum(state, ranks, wrank):
    sel = _selected(state, *NO_FILTER)
    order = np.argsort(state.cell[sel], kind="stable")
    sel = sel[order]
    ends = np.cumsum(np.bincount(state.cell[sel], minlength=state.n_cell))
    w = state.mult[sel] * state.weight[sel] ** wrank
    columns = [w] + [w * state.attr[sel] ** rank for rank in ranks]
    out = np.zeros((len(columns), state.n_cell))
    for k, column in enumerate(columns):
        values = column.tolist()
        for c in range(state.n_cell):
            out[k, c] = math.fsum(values[ends[c - 1] if c else 0:ends[c]])
    return out[0], out[1:]


# ---- sdm_moments ------------------------------------------------------------------------------
def _uploaded(engine, state):
    up = engine.upload
    return {name: up(getattr(state, name)) for name in ("mult", "attr", "cell", "idx", "x",
                                                        "weight")}


def _call_moments(engine, dev, state, ranks, wrank, lo, hi, skip):
    """through the C ABI, outputs pre-filled with NaN; n_ranks = 0 passes moments = ranks = NULL"""
    m0 = engine.upload(np.full(state.n_cell, np.nan))
    mom = engine.upload(np.full((len(ranks), state.n_cell), np.nan)) if ranks else None
    d_ranks = engine.upload(np.asarray(ranks, dtype=float)) if ranks else None
    engine.call("sdm_moments", m0, mom, dev["mult"], dev["attr"], dev["cell"], dev["idx"],
                state.length, d_ranks, len(ranks), state.n_cell, float(lo), float(hi), dev["x"],
                dev["weight"], float(wrank), int(skip))
    return engine.download(m0), engine.download(mom) if ranks else np.empty((0, state.n_cell))


def check_moments_exact(kit, layout, length):
    state = exact_state(layout, length)
    engine = kit.engine
    dev = _uploaded(engine, state)
    for ranks, wrank, filtered, skip in EXACT_OPTIONS:
        lo, hi = FILTER if filtered or layout == "sorted_ragged_filtered" else NO_FILTER
        tag = f"{layout} {length} ranks={ranks} wrank={wrank} [{lo}, {hi}) skip={skip}"
        want0, want = moments_exact(state, ranks, wrank, lo, hi, skip)
        got0, got = _call_moments(engine, dev, state, ranks, wrank, lo, hi, skip)
        np.testing.assert_array_equal(got0, want0, err_msg="moment_0 " + tag)
        np.testing.assert_array_equal(got, want, err_msg=tag)


def check_moments_tolerance(kit, layout):
    state = tolerance_state(layout)
    want0, want = moments_fsum(state, TOLERANCE_RANKS, 1)
    got0, got = _call_moments(kit.engine, _uploaded(kit.engine, state), state, TOLERANCE_RANKS, 1,
                              *NO_FILTER, True)
    np.testing.assert_allclose(got0, want0, rtol=RTOL, atol=0, err_msg=layout)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, err_msg=layout)


def check_moments_backend(kit):
    """the same numbers through backend.moments (the storages of the PySDM-shaped backend)"""
    state = exact_state("sorted_ragged", BIG)
    idx = kit.Index.from_ndarray(state.idx.copy())
    idx.length = int(state.length)
    indexed = {name: kit.IndexedStorage.from_ndarray(idx, getattr(state, name).copy())
               for name in ("mult", "attr", "cell", "x", "weight")}
    for ranks, wrank, filtered, skip in EXACT_OPTIONS[:4]:
        lo, hi = FILTER if filtered else NO_FILTER
        m0 = kit.Storage.from_ndarray(np.full(state.n_cell, np.nan))
        mom = kit.Storage.from_ndarray(np.full((len(ranks), state.n_cell), np.nan))
        kit.backend.moments(
            moment_0=m0, moments=mom, multiplicity=indexed["mult"], attr_data=indexed["attr"],
            cell_id=indexed["cell"], idx=idx, length=state.length,
            ranks=kit.Storage.from_ndarray(np.asarray(ranks, dtype=float)), min_x=lo, max_x=hi,
            x_attr=indexed["x"], weighting_attribute=indexed["weight"], weighting_rank=wrank,
            skip_division_by_m0=skip)
        want0, want = moments_exact(state, ranks, wrank, lo, hi, skip)
        np.testing.assert_array_equal(m0.to_ndarray(), want0, err_msg=str(ranks))
        np.testing.assert_array_equal(mom.to_ndarray(), want, err_msg=str(ranks))


def check_moments_in_use(engine):
    """diagnostics.moments on a state the collision step left behind (20 steps of the Shima box at
    2^18 super-droplets: one cell, every wave uniform, two rounds per wave, real volumes) against
    the sums of the downloaded snapshot as tests/digests.py forms them, here with math.fsum"""
    import warnings  # pylint: disable=import-outside-toplevel

    runner = make_box(engine, "shima", n_sd=2**18, dv=1e6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        runner.run(20)
    pop = runner.population
    got0, got = diagnostics.moments(pop, [0, 1, 2, 3])
    snap = runner.snapshot()
    length = int(snap["length"])
    assert 0 < length <= 2**18
    idx = snap["idx"][:length]
    live_n = snap["multiplicity"][idx].astype(np.float64)
    vol = snap["attributes"][0][idx] / pop.rho_w
    sums = np.asarray([math.fsum((live_n * vol**k).tolist()) for k in range(4)])
    assert got0.shape == (1,) and got.shape == (4, 1)
    np.testing.assert_allclose(got0[0], sums[0], rtol=RTOL, atol=0)
    np.testing.assert_allclose(got[:, 0], sums / sums[0], rtol=RTOL, atol=0)


# ---- sdm_spectrum_moments ---------------------------------------------------------------------
SPECTRUM_LENGTHS = ((1, None), (255, None), (256, None), (257, None), (69999, 70001), (BIG, None))
IRREGULAR_EDGES = (4, 8, 8, 16, 12, 40, 2, 5)  # an empty bin, overlapping bins, a descending step
MAX_BINS = 7999  # the largest number sdm_spectrum_moments of the HIP library accepts
SPECTRUM_EDGES = ("one_bin", "golden", "irregular", "max_bins")
SPECTRUM_CASES = tuple((edges, length, n_sd) for edges in SPECTRUM_EDGES
                       for length, n_sd in SPECTRUM_LENGTHS)
SPECTRUM_OPTIONS = ((3, 1), (2, 0))  # (rank, weighting rank)


def _edges(name):
    return {"one_bin": np.asarray([8.0, 24.0]),
            "golden": np.asarray(MOMENTS["spectrum/bins"], dtype=float),
            "irregular": np.asarray(IRREGULAR_EDGES, dtype=float),
            "max_bins": np.arange(MAX_BINS + 1, dtype=float)}[name]


@functools.lru_cache(maxsize=2)
def spectrum_state(name, length, n_sd=None):
    """exact tier; x as the edges call for it: integers that sit on the edges (one in 97 live
    rows NaN), or log-uniform over more than the golden's range with every fifth value exactly an
    edge"""
    rng = np.random.default_rng([length, SPECTRUM_EDGES.index(name)])
    n_sd = n_sd or length + N_DEAD
    edges = _edges(name)
    idx, dead, cell, mult = _columns(rng, length, n_sd, rng.integers(0, 3, length))
    attr = rng.integers(1, 64, n_sd).astype(float)
    weight = rng.integers(1, 16, n_sd).astype(float)
    if name == "golden":
        x = np.exp(rng.uniform(np.log(edges[0] / 2), np.log(edges[-1] * 2), n_sd))
        x[::5] = rng.choice(edges, n_sd)[::5]
        inside = edges[7]
    else:
        x = rng.integers(0, 8101 if name == "max_bins" else 48, n_sd).astype(float)
        x[::97] = np.nan
        inside = 12.0
    attr[dead], weight[dead] = np.nan, np.nan
    x[dead[0::2]], x[dead[1::2]] = inside, np.nan
    return State(name=name, length=length, n_sd=n_sd, n_cell=3, idx=idx, cell=cell, mult=mult,
                 attr=attr, weight=weight, x=x, edges=edges)


def first_matching_bin(x, edges):
    """-1, or the first k with edges[k] <= x < edges[k + 1]: assigned in reverse order so that
    the first match is what remains"""
    found = np.full(x.shape, -1, dtype=np.int64)
    for k in range(len(edges) - 2, -1, -1):
        found[(edges[k] <= x) & (x < edges[k + 1])] = k
    return found


def spectrum_exact(state, rank, wrank):
    live = state.idx[:state.length]
    x, edges, n_bins = state.x[live], state.edges, len(state.edges) - 1
    if state.name == "max_bins":  # monotonic edges: np.searchsorted
        found = np.searchsorted(edges, x, side="right") - 1
        found[~((found >= 0) & (found < n_bins) & (x == x))] = -1
    else:
        found = first_matching_bin(x, edges)
    sel, found = live[found >= 0], found[found >= 0]
    w = state.mult[sel] * (state.weight[sel].astype(np.int64) ** int(wrank))
    term = w * state.attr[sel].astype(np.int64) ** int(rank)
    at = found * state.n_cell + state.cell[sel]
    shape = (n_bins, state.n_cell)
    m0 = np.bincount(at, weights=w.astype(float), minlength=n_bins * state.n_cell).reshape(shape)
    mom = np.bincount(at, weights=term.astype(float), minlength=n_bins * state.n_cell)
    return m0, _divided(mom.reshape(shape), m0)


def _call_spectrum(engine, dev, state, edges, rank, wrank, prefill=np.nan):
    shape = (len(edges) - 1, state.n_cell)
    m0, mom = engine.upload(np.full(shape, prefill)), engine.upload(np.full(shape, prefill))
    engine.call("sdm_spectrum_moments", m0, mom, dev["mult"], dev["attr"], dev["cell"],
                dev["idx"], state.length, float(rank), engine.upload(edges), len(edges) - 1,
                state.n_cell, dev["x"], dev["weight"], float(wrank))
    return engine.download(m0), engine.download(mom)


def check_spectrum_exact(kit, name, length, n_sd=None):
    state = spectrum_state(name, length, n_sd)
    dev = _uploaded(kit.engine, state)
    for rank, wrank in SPECTRUM_OPTIONS:
        tag = f"{name} {length} rank={rank} wrank={wrank}"
        want0, want = spectrum_exact(state, rank, wrank)
        got0, got = _call_spectrum(kit.engine, dev, state, state.edges, rank, wrank)
        np.testing.assert_array_equal(got0, want0, err_msg="moment_0 " + tag)
        np.testing.assert_array_equal(got, want, err_msg=tag)
        assert (got[got0 == 0] == 0).all(), tag  # (and not NaN: the pre-fill)
    if name == "irregular":
        assert (got0[1] == 0).all() and (got0[3] == 0).all()  # [8, 8) and [16, 12)
        if length >= 69999:  # (enough in every cell for [2, 5), the bin least likely hit)
            assert (got0[[0, 2, 4, 6]] > 0).all()


def check_spectrum_one_bin_too_many(kit):
    """8000 bins: more edges than the HIP library holds in LDS - an error, and nothing written;
    the oracle has no such limit and must simply be right"""
    state = spectrum_state("max_bins", 257)
    edges = np.arange(MAX_BINS + 2, dtype=float)
    dev = _uploaded(kit.engine, state)
    marker = -12345.5
    if kit.engine.name == "hip":
        m0 = kit.engine.upload(np.full((MAX_BINS + 1, 3), marker))
        mom = kit.engine.upload(np.full((MAX_BINS + 1, 3), marker))
        with pytest.raises(RuntimeError):
            kit.engine.call("sdm_spectrum_moments", m0, mom, dev["mult"], dev["attr"],
                            dev["cell"], dev["idx"], state.length, 1.0, kit.engine.upload(edges),
                            MAX_BINS + 1, 3, dev["x"], dev["weight"], 0.0)
        assert (kit.engine.download(m0) == marker).all()
        assert (kit.engine.download(mom) == marker).all()
    else:
        wider = State(**{**vars(state), "edges": edges, "name": "max_bins"})
        want0, want = spectrum_exact(wider, 1, 0)
        got0, got = _call_spectrum(kit.engine, dev, state, edges, 1, 0, prefill=marker)
        np.testing.assert_array_equal(got0, want0)
        np.testing.assert_array_equal(got, want)


# ---- Storage.amin / amax (sdm_reduce_f64) ---------------------------------------------------
GRID_STRIDE_FROM = 262144  # 1024 blocks of SDM_BLOCK: the first element only the loop sees
EXTREME_SIZES = (1, 63, 64, 65, 255, 256, 257, 1001, 262144, 262145, 262144 + 773, 2**20 + 1)


@functools.lru_cache(maxsize=1)
def _normal(n):
    data = np.random.default_rng(n).standard_normal(n)
    data.setflags(write=False)
    return data


def check_extremes(kit, n):
    """np.min / np.max for equality: the extreme, then one NaN, planted in turn at 0, n - 1 and
    262144; infinities of both signs; all elements equal"""
    def both(data, tag):
        sto = kit.Storage.from_ndarray(data)
        for got, want in ((sto.amin(), np.min(data)), (sto.amax(), np.max(data))):
            assert (np.isnan(want) and np.isnan(got)) or got == want, (n, tag, got, want)

    places = sorted({0, n - 1} | ({GRID_STRIDE_FROM} if n > GRID_STRIDE_FROM else set()))
    for place in places:
        for planted in (-10.0, 10.0, np.nan):
            data = _normal(n).copy()
            data[place] = planted
            both(data, (place, planted))
            if planted == planted:
                assert planted in (np.min(data), np.max(data))
    data = _normal(n).copy()
    data[n // 2], data[n // 3] = np.inf, -np.inf  # (the same element if n == 1: -inf)
    both(data, "inf")
    for value in (np.inf, -np.inf, 1.25):
        both(np.full(n, value), ("all", value))


def check_extremes_refuse_empty(kit):
    out = ctypes.c_double(-1.0)
    with pytest.raises(RuntimeError):
        kit.engine.call("sdm_reduce_f64", 0, kit.engine.upload(np.zeros(1)), 0, out)
    with pytest.raises(RuntimeError):
        kit.engine.call("sdm_reduce_f64", 1, kit.engine.upload(np.zeros(1)), 0, out)


# ---- sdm_flag_precipitated --------------------------------------------------------------------
PRECIPITATION_CASES = tuple((n_dims, length) for n_dims in (1, 2)
                            for length in (1, 255, 256, 257, 262145))  # 262145: 1025 partials
LEVEL = 1.5


def flag_precipitated_expected(state, displacement):
    """flag_precipitated of the reference's displacement_methods.py restated with NumPy: a live
    super-droplet that moves down (displacement < 0 in the last dimension) and lies below the
    counting level leaves - its slot of idx is set to n_sd, healthy drops to 0 and its
    |water mass| * multiplicity joins the sum (integers: exact in any order)"""
    live = state.idx[:state.length]
    z = state.cell_origin[-1, live] + state.position_in_cell[-1, live]
    gone = (displacement[-1, live] < 0) & (z < LEVEL)
    idx = state.idx.copy()
    idx[:state.length][gone] = state.n_sd
    rain = np.sum(np.abs(state.mass[live][gone]).astype(np.int64) * state.mult[live][gone])
    return idx, int(not gone.any()), float(rain), gone


@functools.lru_cache(maxsize=1)
def precipitation_state(n_dims, length):
    """z = origin + position takes the values 0, 0.25 .. 3.75 exactly, the level is one of them
    and the displacement is -0.5, 0 or 0.5; the rows of the first dimension (n_dims = 2) would
    flag everyone.  Position 0 holds z == level with a negative displacement, position 1
    displacement == 0 below the level; the ids beyond `length` all qualify"""
    rng = np.random.default_rng([n_dims, length])
    n_sd = length + N_DEAD
    idx, dead, _, mult = _columns(rng, length, n_sd, 0)
    origin = np.zeros((n_dims, n_sd), dtype=np.int64)
    within = np.zeros((n_dims, n_sd))
    displacement = np.full((n_dims, n_sd), -1.0)
    origin[-1] = rng.integers(0, 4, n_sd)
    within[-1] = rng.integers(0, 4, n_sd) / 4
    displacement[-1] = rng.integers(-1, 2, n_sd) / 2
    first = idx[0]
    origin[-1, first], within[-1, first], displacement[-1, first] = 1, 0.5, -0.5
    if length > 1:
        origin[-1, idx[1]], within[-1, idx[1]], displacement[-1, idx[1]] = 0, 0.25, 0.0
    origin[-1, dead], within[-1, dead], displacement[-1, dead] = 0, 0.0, -0.5
    mass = rng.integers(-50, 51, n_sd).astype(float)
    return State(length=length, n_sd=n_sd, idx=idx, mult=mult, mass=mass, cell_origin=origin,
                 position_in_cell=within, displacement=displacement)


def check_flag_precipitated(kit, n_dims, length):
    state = precipitation_state(n_dims, length)
    engine = kit.engine
    rising = np.abs(state.displacement)
    for tag, displacement in (("falling", state.displacement), ("none falls", rising)):
        want_idx, want_healthy, want_rain, gone = flag_precipitated_expected(state, displacement)
        if tag == "falling":
            assert not gone[0] and not gone[1:2].any()
            assert gone.any() == (length > 1)
        else:
            assert not gone.any()
        idx, healthy = engine.upload(state.idx), engine.upload(np.ones(1, dtype=np.int64))
        rain = engine.scalar_out(
            "sdm_flag_precipitated", ctypes.c_double, engine.upload(state.cell_origin),
            engine.upload(state.position_in_cell), engine.upload(state.mass),
            engine.upload(state.mult), idx, length, state.n_sd, n_dims, healthy, LEVEL,
            engine.upload(displacement))
        np.testing.assert_array_equal(engine.download(idx), want_idx, err_msg=tag)
        assert int(engine.download(healthy)[0]) == want_healthy, tag
        assert rain == want_rain, (tag, rain, want_rain)

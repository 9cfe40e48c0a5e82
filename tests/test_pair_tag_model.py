"""pysdm_amd/csrc/pair_tag.h compiled for the host (tests/pair_tag_model): the bounds a tag stands
for are never below the true values, class order is multiplicity order, `ex` is equality - and on
states the oracle produced, every pair the decision skips has gamma == 0 and the decided order in
the full computation.  No GPU."""
import functools
import warnings

import numpy as np
import pytest

from tests.pair_tag_model import model, skip_share

N_REFS = [1, 2, 3, 7, 8, 9_000_001, 2**23, 2**40 + 12345, 2**62 - 1]


def ulps(values, steps):
    out = np.asarray(values, dtype=np.float64)
    for _ in range(abs(steps)):
        out = np.nextafter(out, np.inf if steps > 0 else -np.inf)
    return out


def multiplicities(n_ref, rng):
    edges = np.asarray([n_ref >> k for k in range(0, 18)], dtype=np.int64)
    near = np.concatenate([edges - 1, edges, edges + 1])
    random = rng.integers(1, max(n_ref, 2), 4000, dtype=np.int64)
    small = np.asarray([0, -1, -2**40, 1, 2, 3], dtype=np.int64)
    return np.concatenate([near, random, small, np.asarray([n_ref + 1, 2 * n_ref], dtype=np.int64)])


def masses(m_base, rng):
    edges = m_base * 4.0 ** np.arange(-2, 17)
    near = np.concatenate([ulps(edges, -1), edges, ulps(edges, 1)])
    random = m_base * 4.0 ** rng.uniform(-3, 16, 4000)
    odd = np.asarray([0.0, -0.0, -1.0, -m_base, np.inf, -np.inf, np.nan, 5e-324, 1e308])
    return np.concatenate([near, random, odd])


@pytest.mark.parametrize("n_ref", N_REFS)
def test_multiplicity_classes(n_ref):
    mdl, rng = model(), np.random.default_rng(n_ref % 1000)
    n = multiplicities(n_ref, rng)
    tag = mdl.encode(n, np.ones(n.shape), n_ref, 1.0)
    n_class, exact = tag & 15, (tag >> 4) & 1
    n_ub, _ = mdl.bounds(tag, n_ref, 1.0)
    known = n_class != 0
    assert known.any()
    # unknown exactly where the issue says so
    outside = (n <= 0) | (n > n_ref) | (n <= (n_ref >> 15))
    np.testing.assert_array_equal(~known, outside)
    # the class's interval holds the value; its upper bound is never below it
    c = n_class[known].astype(np.int64)
    assert np.all(n[known] <= n_ub[known])
    assert np.all(n[known] > (n_ref >> c))
    assert np.all(n_ub[known] == (n_ref >> (c - 1)))
    # `ex` is equality with n_ref >> (c - 1), the shift having lost nothing
    is_exact = (n[known] << (c - 1)) == n_ref
    np.testing.assert_array_equal(exact[known].astype(bool), is_exact)
    assert np.all(n[known][is_exact] == n_ub[known][is_exact])
    assert not exact[~known].any()
    # class order is multiplicity order, for every pair of known values
    a, b = rng.integers(0, known.sum(), (2, 20000))
    na, nb, ca, cb = n[known][a], n[known][b], c[a], c[b]
    assert np.all(na[ca > cb] < nb[ca > cb])
    order = mdl.order(tag[known][a], tag[known][b])
    np.testing.assert_array_equal(order[ca != cb], (ca > cb)[ca != cb].astype(np.int8))
    both = (ca == cb) & is_exact[a] & is_exact[b]
    assert np.all(order[both] == 0) and np.all(na[both] == nb[both])
    assert np.all(order[(ca == cb) & ~both] == -1)
    assert np.all(mdl.order(tag[~known][:1].repeat(known.sum()), tag[known]) == -1)


@pytest.mark.parametrize("m_max", [1.0, 3.0e-10, 4.7e-13, 2.0**-1000, 1.7e300, 0.75])
def test_mass_classes(m_max):
    mdl, rng = model(), np.random.default_rng(3)
    m_base = mdl.m_base(m_max)
    mantissa, _ = np.frexp(m_base)
    assert mantissa == 0.5  # a power of two
    assert m_max * 2.0**-16 <= m_base < m_max * 2.0**-15
    m = masses(m_base, rng)
    tag = mdl.encode(np.ones(m.shape, dtype=np.int64), m, 1, m_base)
    m_class = (tag >> 5) & 15
    _, m_ub = mdl.bounds(tag, 1, m_base)
    known = m_class != 0
    with np.errstate(invalid="ignore"):
        outside = ~np.isfinite(m) | ~(m > 0) | (m > m_base * 4.0**14)
    np.testing.assert_array_equal(~known, outside)
    c = m_class[known].astype(np.float64)
    np.testing.assert_array_equal(m_ub[known], m_base * 4.0 ** (c - 1))  # exact edges
    assert np.all(m[known] <= m_ub[known])
    above_first = c > 1
    assert np.all(m[known][above_first] > m_base * 4.0 ** (c[above_first] - 2))


def test_no_reference_no_class():
    mdl = model()
    for bad in (0.0, -1.0, np.inf, np.nan, 5e-324, 2.0**-1020):
        assert mdl.m_base(bad) == 0.0
    tag = mdl.encode([5, 0, -3], [1.0, 1.0, 1.0], 0, 0.0)
    assert not tag.any()


def states(kind, n_sd, checkpoints):
    """(runner description, multiplicity, mass, live ids) of the oracle's box after every
    checkpoint, starting with the initial state"""
    from oracle.engine import OracleEngine  # pylint: disable=import-outside-toplevel
    from tests.test_hip_pair_tags import box  # pylint: disable=import-outside-toplevel

    runner = box(OracleEngine.get(), kind, n_sd)
    cfg = runner.step_cfg()
    numbers = dict(b=float(cfg.kernel_param[0]), rho_w=float(cfg.rho_w), dt=float(cfg.dt),
                   dv=float(cfg.dv), substeps=int(cfg.substeps))
    out, done = [], 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for upto in checkpoints:
            if upto > done:
                runner.run(upto - done)
                done = upto
            snap = runner.snapshot()
            length = int(snap["length"])
            out.append((snap["multiplicity"].copy(), snap["attributes"][0].copy(),
                        snap["idx"][:length].copy()))
    return numbers, out


@functools.lru_cache(maxsize=None)
def shares(kind, n_sd, checkpoints, pairings=8):
    """per checkpoint after the first: (pairs, skipped, colliding, sound) summed over a few random
    pairings, with the references of the state the call began with (the first checkpoint)"""
    mdl, rng = model(), np.random.default_rng(11)
    numbers, snaps = states(kind, n_sd, checkpoints)
    n0, m0, ids0 = snaps[0]
    n_ref = int(n0[ids0].max())
    m_base = mdl.m_base(float(m0[ids0].max()))
    rows = []
    for multiplicity, mass, ids in snaps[1:]:
        total = np.zeros(3, dtype=np.int64)
        sound = True
        for _ in range(pairings):
            pairs, skipped, colliding, ok = skip_share(mdl, multiplicity, mass, ids, rng,
                                                       n_ref=n_ref, m_base=m_base, **numbers)
            total += (pairs, skipped, colliding)
            sound = sound and ok
        rows.append((*total, sound))
    return rows


@pytest.mark.parametrize("kind,n_sd,checkpoints", [
    ("shima", 4097, (0, 1, 5, 12, 60)),
    ("thin", 4099, (0, 1, 3, 6, 12)),
    ("spread", 8193, (0, 1, 2, 5, 12)),
    ("spread", 4099, (3, 4, 8, 9, 12)),
])
def test_skipped_pairs_are_no_collisions_on_oracle_states(kind, n_sd, checkpoints):
    rows = shares(kind, n_sd, checkpoints)
    print(kind, n_sd, rows)
    assert all(sound for *_, sound in rows)
    assert sum(skipped for _, skipped, _, _ in rows) > 0
    if kind != "shima":
        assert sum(colliding for _, _, colliding, _ in rows) > 0


@pytest.mark.parametrize("n_sd", [4097, 4099, 8190, 8193, 12290, 2**16 + 5])
def test_default_box_share_is_above_the_bound_the_gpu_test_asserts(n_sd):
    """tests/test_hip_pair_tags.py asserts 0.8 per call of CHUNKS = (1, 2, 6, 3); the calls begin
    after steps 0, 1, 3 and 9, and the model's share - references from the call's start, the
    states of its interior steps - is far above that"""
    for start, interior in ((3, (4, 5, 6, 7)), (9, (10,))):
        rows = shares("shima", n_sd, (start, *interior), pairings=4)
        pairs = sum(r[0] for r in rows)
        skipped = sum(r[1] for r in rows)
        print(n_sd, start, skipped / pairs)
        assert all(r[3] for r in rows)
        assert skipped >= 0.9 * pairs

"""The seeding path on the device (pysdm_amd/csrc/seeding.hip) against the goldens recorded from
the reference and against the CPU checker of include/sdm_seeding.h, for both symbols.

Everything is compared for equality: integers with ==, doubles as uint64 (they are copies).
Sizes: around a wave (63, 64, 65), around the tile of the kernels (T - 1, T, T + 1), several
tiles, and one tile more than a round of the tile-count scan holds plus one slot - the largest
state here, 1 049 601 slots.  A refusal (fewer free slots than asked for) is part of every sweep:
small states with large K are refused by both sides, and then everything is compared with the
state before the call."""
import numpy as np
import pytest

from pysdm_amd import seeding as sd
from tests import seeding_cases as sc

pytestmark = pytest.mark.gpu

T, ROUND = sc.TILE, sc.ROUND
SIZES = [1, 63, 64, 65, 1000, 4097, 70001, T - 1, T, T + 1, (ROUND + 1) * T + 1]
RESERVOIRS = [(1, 1), (2, 1), (2, 2), (10, 1), (10, 5), (10, 10), (1000, 1), (1000, 500),
              (1000, 1000)]  # (seeds, K): K = 1, half of the reservoir, all of it
INDICES = ("identity", "reversed", "equal")
OFFSETS = (0, 2 ** 33 + 5)


@pytest.fixture(scope="module", name="checker")
def checker_engine():
    from tests.seeding_checker import SeedingCheckerEngine  # pylint: disable=import-outside-toplevel

    return SeedingCheckerEngine.get()


def both_symbols_agree(hip_engine, checker, state, offset, what):
    """sdm_seeding and sdm_seeding_step on the device against the checker; returns True if the
    injection went ahead"""
    got, want = sc.call_stage(hip_engine, state), sc.call_stage(checker, state)
    for key in ("status", "idx", "multiplicity", "attributes"):
        sc.assert_same_bits(got[key], want[key], f"{what}: sdm_seeding: {key}")
    free = int((state["multiplicity"] == 0).sum())
    assert int(got["status"][0]) == free, what
    went = free >= state["k"]
    assert int(got["status"][1]) == (state["k"] if went else 0), what
    got = sc.call_step(hip_engine, state, shuffle=True, offset=offset)
    want = sc.call_step(checker, state, shuffle=True, offset=offset)
    sc.assert_same_step(got, want, f"{what}: sdm_seeding_step")
    assert (got["error"] is None) == went, what
    if not went:  # against the state before the call: nothing was stored
        assert f"{free} free slots" in got["error"], got["error"]
        for key in ("idx", "multiplicity", "attributes"):
            sc.assert_same_bits(got[key], state[key], f"{what}: refused: {key}")
    return went


# ---- the goldens -------------------------------------------------------------------------------------
def test_hip_replays_recorded_method_calls(hip_backend_class):
    data = sc.gold("seed_methods")
    for number in range(int(data["n_calls"])):
        got, expected = sc.replay_method_call(hip_backend_class, data, number)
        for key, value in expected.items():
            sc.assert_same_bits(got[key], value, f"{data['kind'][number]}: {key}")


@pytest.mark.parametrize("route", sd.ROUTES)
@pytest.mark.parametrize("name", ["seed_box", "seed_box_coal"])
def test_hip_runner_reproduces_recorded_box_run(hip_engine, name, route):
    data = sc.gold(name)
    for step, got in enumerate(sc.run_box(hip_engine, data, route)):
        sc.assert_box_step(got, data, step, f"{name} ({route})")


def test_hip_under_the_pysdm_front_end_reproduces_the_box(hip_backend_class):
    """(where PySDM can be imported: skipped otherwise)"""
    from tests.test_seeding_checker import import_reference, run_pysdm_box  # pylint: disable=import-outside-toplevel

    ref = import_reference()
    data = sc.gold("seed_box")
    for fused in (False, True):
        for step, got in enumerate(run_pysdm_box(ref, hip_backend_class, data, fused)):
            sc.assert_box_step(got, data, step, f"PySDM front-end on HIP (fuse: {fused})")


# ---- against the checker -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_sd", SIZES)
def test_hip_equals_checker_on_seeded_states(hip_engine, checker, n_sd):
    """every (reservoir, K) at every size, with rows x seed-index order x stream offset in full
    combination while the state is small; at 70001 slots two of the twelve combinations per
    reservoir (all twelve over the nine reservoirs), at a million slots one (nine of them)"""
    combos = [(n_attr, index, offset) for n_attr in (1, 5) for index in INDICES
              for offset in OFFSETS]
    picks = 2 if n_sd < 100000 else 1
    went = refused = 0
    for at, (n_seeds, k) in enumerate(RESERVOIRS):
        chosen = combos if n_sd <= 4097 else [combos[(picks * at + j) % len(combos)]
                                              for j in range(picks)]
        if n_sd > 4097:
            assert len({combos[(picks * a + j) % len(combos)] for a in range(len(RESERVOIRS))
                        for j in range(picks)}) == (len(combos) if picks == 2 else 9)
        for n_attr, index, offset in chosen:
            state = sc.seeded_state(n_sd, n_seeds=n_seeds, k=k, n_attr=n_attr, index=index,
                                    seed=at)
            what = f"n_sd {n_sd}, {n_seeds} seeds, K {k}, {n_attr} rows, {index}, +{offset}"
            if both_symbols_agree(hip_engine, checker, state, offset, what):
                went += 1
            else:
                refused += 1
    assert went > 0
    assert refused == 0 or n_sd < 1000  # (only states smaller than K are refused)


def _slots(n_sd, slots):
    mask = np.zeros(n_sd, dtype=bool)
    mask[np.asarray(slots, dtype=np.int64)] = True
    return mask


def planted(pattern, n_free, k):
    """the mask of free slots of a planted pattern with `n_free` free slots (K = k)"""
    if pattern == "all free":
        return np.ones(n_free, dtype=bool)
    if pattern == "last tile only":
        n_sd = 3 * T + 17
        return _slots(n_sd, np.arange(n_sd - n_free, n_sd))
    if pattern.startswith("K-th free slot"):
        # the k-th free slot (rank k - 1) at `target`; those before it spread below, one after it
        target = {"K-th free slot on the last lane of a wave": 2 * T + 5 * 64 + 63,
                  "K-th free slot on the last slot of a tile": 2 * T - 1,
                  "K-th free slot on the first slot of the next tile": 2 * T}[pattern]
        before = np.linspace(0, target - 1, min(n_free, k - 1)).astype(np.int64)
        assert len(set(before)) == len(before)
        after = [target] + [target + 1 + 3 * j for j in range(n_free - k)]
        return _slots(4 * T + 3, list(before) + (after if n_free >= k else []))
    if pattern == "first and last lane only":
        lanes = np.sort(np.concatenate([np.arange(0, 4 * T, 64), np.arange(63, 4 * T, 64)]))
        return _slots(4 * T, lanes[:n_free])
    raise ValueError(pattern)


PATTERNS = ["all free", "last tile only", "K-th free slot on the last lane of a wave",
            "K-th free slot on the last slot of a tile",
            "K-th free slot on the first slot of the next tile", "first and last lane only"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_planted_patterns_of_free_slots(hip_engine, checker, pattern):
    k = 100
    for n_free in (k - 1, k, k + 1):
        free = planted(pattern, n_free, k)
        assert int(free.sum()) == n_free, pattern
        for n_attr, index in ((1, "reversed"), (5, "identity")):
            state = sc.state_with_free(free, k=k, n_seeds=k, n_attr=n_attr, index=index)
            went = both_symbols_agree(hip_engine, checker, state, 0,
                                      f"{pattern}, {n_free} free, K {k}, {n_attr} rows")
            assert went == (n_free >= k)
            if went and pattern.startswith("K-th"):
                out = sc.call_stage(hip_engine, state)
                filled = np.flatnonzero(out["idx"] == -1)
                assert len(filled) == k and filled[-1] == np.flatnonzero(free)[k - 1]
                assert filled[-1] % 64 == {"K-th free slot on the last lane of a wave": 63,
                                           "K-th free slot on the last slot of a tile": 63,
                                           "K-th free slot on the first slot of the next tile": 0
                                           }[pattern]


def test_free_slots_behind_the_live_length_in_another_order(hip_engine, checker):
    """a state as a coalescence run leaves it: the dead are named behind the live length of idx in
    the order in which they died, not in slot order; the injection goes by slot all the same"""
    rng = np.random.default_rng(7)
    n_sd, k = 3 * T + 5, 40
    for n_free in (k - 1, k, k + 1):
        dead = rng.permutation(n_sd)[:n_free]
        live = np.setdiff1d(np.arange(n_sd), dead)
        idx = np.concatenate([rng.permutation(live), dead]).astype(np.int64)
        state = sc.state_with_free(_slots(n_sd, dead), k=k, n_seeds=k, n_attr=2,
                                   index="reversed", idx=idx)
        went = both_symbols_agree(hip_engine, checker, state, 0, f"dead tail, {n_free} free")
        assert went == (n_free >= k)
    out = sc.call_stage(hip_engine, state)
    np.testing.assert_array_equal(np.flatnonzero(out["idx"] == -1), np.sort(dead)[:k])


def test_a_seed_of_multiplicity_zero_is_injected_and_compacted_away(hip_engine, checker):
    """at K - 1, K and K + 1 free slots; a refusal is compared with the state before the call
    (in `both_symbols_agree`)"""
    k, n_sd = 4, T + 9
    slots = [3, 64, T - 1, T, T + 8]
    for n_free in (k - 1, k, k + 1):
        state = sc.state_with_free(_slots(n_sd, slots[:n_free]), k=k, n_seeds=k, n_attr=2)
        state["seed_multiplicity"][[1, 2]] = 0
        went = both_symbols_agree(hip_engine, checker, state, 0,
                                  f"seeds of multiplicity 0, {n_free} free")
        assert went == (n_free >= k)
        fused = sc.call_step(hip_engine, state, shuffle=False)
        if not went:
            assert fused["lengths"] == [] and f"{n_free} free slots" in fused["error"]
            for key in ("idx", "multiplicity", "attributes"):
                sc.assert_same_bits(fused[key], state[key], f"refused: {key}")
            continue
        # seeds 1 and 2 land in slots 64 and T - 1 and leave again; a fifth free slot stays free
        assert fused["lengths"] == [n_sd - n_free + 2]
        np.testing.assert_array_equal(fused["multiplicity"][[64, T - 1]], [0, 0])
        np.testing.assert_array_equal(fused["multiplicity"][[3, T]],
                                      state["seed_multiplicity"][[0, 3]])
        sc.assert_same_bits(fused["attributes"][:, slots[:k]], state["seed_attributes"],
                            "the rows arrive all the same")
        gone = slots[1:3] + slots[k:n_free]
        assert not np.isin(gone, fused["idx"][:fused["lengths"][0]]).any()
        assert np.isin([3, T], fused["idx"][:fused["lengths"][0]]).all()


def test_nan_payloads_and_negative_zero_survive(hip_engine, checker):
    """at K - 1, K and K + 1 free slots; a refusal is compared with the state before the call"""
    k, n_sd = 4, 131
    slots = [0, 63, 64, 129, 130]
    words = np.array([0x7FF8000000000000, 0xFFF0DEADBEEF0001, 0x8000000000000000,
                      0x7FF0000000000001], dtype=np.uint64)  # NaNs with payloads, -0.0, an sNaN
    for n_free in (k - 1, k, k + 1):
        state = sc.state_with_free(_slots(n_sd, slots[:n_free]), k=k, n_seeds=k, n_attr=2)
        state["seed_attributes"][0] = words.view(np.float64)
        state["seed_attributes"][1] = -0.0
        went = both_symbols_agree(hip_engine, checker, state, 0, f"NaN and -0.0, {n_free} free")
        assert went == (n_free >= k)
        out = sc.call_stage(hip_engine, state)
        if not went:
            np.testing.assert_array_equal(out["status"][:3], [n_free, 0, 0])
            for key in ("idx", "multiplicity", "attributes"):
                sc.assert_same_bits(out[key], state[key], f"refused: {key}")
            continue
        np.testing.assert_array_equal(out["attributes"][0, slots[:k]].view(np.uint64), words)
        assert np.signbit(out["attributes"][1, slots[:k]]).all()
        sc.assert_same_bits(out["attributes"][:, slots[k:n_free]],
                            state["attributes"][:, slots[k:n_free]], "the fifth slot is left alone")


def test_ranks_decided_in_the_second_round_of_the_scan(hip_engine, checker):
    """(ROUND + 1) * T + 1 slots: ROUND + 2 tiles, of which the last two get their offsets in the
    second round of k_seed_scan.  Free slots: 30 in tile 5 and 30 in the last tile of round one
    (they make the carry between the rounds), the others in the first tile of round two, and the
    very last slot, alone in its tile - the K-th free slot at K free slots, the (K + 1)-th, which
    must stay free, at K + 1.  Then the same with free slots in those last two tiles only."""
    k, n_sd = 100, (ROUND + 1) * T + 1
    last = n_sd - 1
    for carried in (60, 0):
        for n_free in (k - 1, k, k + 1):
            early = np.concatenate([5 * T + 7 * np.arange(carried // 2),
                                    (ROUND - 1) * T + 64 * np.arange(carried // 2) + 63])
            rest = n_free - carried - 1
            late = ROUND * T + 10 * np.arange(rest)
            free = _slots(n_sd, np.concatenate([early, late, [last]]).astype(np.int64))
            assert int(free.sum()) == n_free and late.max() < (ROUND + 1) * T
            for n_attr, index in ((1, "reversed"), (2, "identity")):
                state = sc.state_with_free(free, k=k, n_seeds=k, n_attr=n_attr, index=index)
                went = both_symbols_agree(hip_engine, checker, state, 0,
                                          f"round two, carry {carried}, {n_free} free")
                assert went == (n_free >= k)
                if went:
                    out = sc.call_stage(hip_engine, state)
                    filled = np.flatnonzero(out["idx"] == -1)
                    assert len(filled) == k and (filled >= ROUND * T).sum() >= k - carried - 1
                    assert (out["idx"][last] == -1) == (n_free == k)
                    assert (out["multiplicity"][last] == 0) == (n_free == k + 1)


def test_shortfall_stores_nothing_and_is_reported(hip_engine):
    """against the state before the call (the reference has no expected value for this case)"""
    for n_sd, n_free, k in ((10, 2, 3), (2 * T + 1, 2 * T, 2 * T + 1), (5 * T, 0, 1)):
        rng = np.random.default_rng(n_sd)
        free = _slots(n_sd, rng.permutation(n_sd)[:n_free])
        state = sc.state_with_free(free, k=k, n_seeds=k, n_attr=3, index="reversed",
                                   idx=rng.permutation(n_sd).astype(np.int64))
        out = sc.call_stage(hip_engine, state)
        np.testing.assert_array_equal(out["status"][:3], [n_free, 0, 0])
        fused = sc.call_step(hip_engine, state, shuffle=False)
        assert fused["error"] is not None and f"{n_free} free slots" in fused["error"]
        assert fused["lengths"] == []
        for result in (out, fused):
            for key in ("idx", "multiplicity", "attributes"):
                sc.assert_same_bits(result[key], state[key], f"n_sd {n_sd}: {key}")


@pytest.mark.parametrize("n_sd, n_seeds, k", [(65, 2, 1), (1000, 10, 5), (T + 1, 1, 1),
                                             (70001, 1000, 1000), (4 * T, 1000, 500)])
def test_hip_fused_equals_stage_sequence_over_three_injections(hip_engine, n_sd, n_seeds, k):
    for offset in OFFSETS:
        state = sc.seeded_state(n_sd, n_seeds=n_seeds, k=k, n_attr=3, index="reversed",
                                free_fraction=0.8)
        assert int((state["multiplicity"] == 0).sum()) >= 3 * k
        got = sc.call_step(hip_engine, state, shuffle=True, offset=offset, n_calls=3)
        want = sc.stage_sequence(hip_engine, state, shuffle=True, offset=offset, n_calls=3)
        assert got["error"] is None and len(got["lengths"]) == 3
        sc.assert_same_step(got, want, f"n_sd {n_sd}, +{offset}")
        if n_seeds > 2:  # the index persists and is shuffled again
            assert (got["seed_index"] != state["seed_index"]).any()

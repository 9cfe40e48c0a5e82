"""time line of one launch of k_pair_all_sort from a -DPAIR_PROFILE build: which workgroup (sort /
pair) ran when and on which CU, and how many workgroups of the kernel the runtime keeps on a CU:
SDM_HIP_LIB=build_variants/libsdm_pairprof.so PYTHONPATH=. python profiles/tools/pair_profile.py
Also, per event tile, the XCDs its two pair workgroups ran on (SDM_WALK_LOCAL=0: grid order)."""
import ctypes
import os
import sys
from collections import defaultdict

import numpy as np

from pysdm_amd import abi
from pysdm_amd.cases import make_box
from pysdm_amd.engine import HipEngine

CAP = 8192  # PAIR_PROF_CAP (fused.hip)
TICK_US = 0.01  # wall_clock64: 100 MHz

engine = HipEngine.get()
runner = make_box(engine, "shima", adaptive=False, read_back=False)
runner.run(20)
engine.synchronize()
lib = abi.hip_library().cdll
launch = (ctypes.c_longlong * 3)()
out = (ctypes.c_longlong * (4 * CAP))()
runs = []
for _ in range(5):
    runner.run(3)  # the launch read back is the second step's: the last step has no sort riding
    engine.synchronize()
    assert lib.sdm_debug_pair_launch(launch) == 0
    n_wg = int(launch[0])
    assert 0 < n_wg <= CAP, n_wg
    assert lib.sdm_debug_pair_profile(out, n_wg) == 0
    runs.append(np.array(out[: 4 * n_wg], dtype=np.int64).reshape(n_wg, 4))
grid, lds_bytes, n_tiles = (int(v) for v in launch)
print(f"grid {grid} workgroups of 1024 threads: {n_tiles} sort + {grid - n_tiles} pair, "
      f"dynamic LDS {lds_bytes} B")
print("hipOccupancyMaxActiveBlocksPerMultiprocessor(k_pair_all_sort<Golovin>, 1024, "
      f"{lds_bytes}) = {lib.sdm_debug_pair_occupancy()}")


def describe(rows, verbose):
    t0, t1 = rows[:, 0], rows[:, 1]
    sorts = (rows[:, 2] & 1) == 0  # role: 0 sort, 1 pair
    hw = rows[:, 3]
    xcc = (hw >> 32) & 0xF
    cu = ((hw & 0xFFFFFFFF) >> 8) & 0xFF  # CU, shader array and shader engine of HW_ID, as one key
    place = xcc * 256 + cu
    origin = t0.min()
    us = lambda t: (t - origin) * TICK_US  # noqa: E731
    res = {
        "kernel": us(t1.max()),
        "sort_first_start": us(t0[sorts].min()), "sort_last_start": us(t0[sorts].max()),
        "sort_last_end": us(t1[sorts].max()),
        "sort_mean": ((t1 - t0)[sorts]).mean() * TICK_US,
        "pair_first_start": us(t0[~sorts].min()), "pair_last_start": us(t0[~sorts].max()),
        "pair_mean": ((t1 - t0)[~sorts]).mean() * TICK_US,
    }
    res["sort_span"] = res["sort_last_end"] - res["sort_first_start"]
    if not verbose:
        return res
    print(f"CUs seen: {len(set(place.tolist()))} on {len(set(xcc.tolist()))} XCDs")
    for k, v in res.items():
        print(f"  {k:18s} {v:7.2f} us")
    # residency per CU over time
    print("   t[us]  sort  pair | CUs with: sort+pair sort+sort pair+pair sort only pair only idle")
    places = sorted(set(place.tolist()))
    end = int(t1.max() - origin)
    for t in range(0, end + 100, 100 if end < 4000 else 200):
        here = (t0 - origin <= t) & (t < t1 - origin)
        per = defaultdict(lambda: [0, 0])
        for p, s in zip(place[here].tolist(), sorts[here].tolist()):
            per[p][0 if s else 1] += 1
        kinds = [0] * 6
        for p in places:
            s, q = per[p]
            kinds[0 if s and q else 1 if s > 1 else 2 if q > 1 else 3 if s else 4 if q else 5] += 1
        print(f"  {t * TICK_US:6.1f} {int((here & sorts).sum()):5d} {int((here & ~sorts).sum()):5d} |"
              f" {kinds[0]:18d} {kinds[1]:9d} {kinds[2]:9d} {kinds[3]:9d} {kinds[4]:9d} {kinds[5]:4d}")
    # exact: the largest number of this kernel's workgroups on one CU at any time
    most = 0
    for p in places:
        m = place == p
        ev = sorted([(a, 1) for a in t0[m].tolist()] + [(b, -1) for b in t1[m].tolist()],
                    key=lambda e: (e[0], e[1]))  # (an end before a start at the same tick)
        n = 0
        for _, d in ev:
            n += d
            most = max(most, n)
    print(f"most workgroups resident on one CU at a time: {most}")
    first = defaultdict(list)  # what each CU ran, in order of entry
    for i in np.argsort(t0):
        first[int(place[i])].append("S" if sorts[i] else "P")
    orders = defaultdict(int)
    for seq in first.values():
        orders["".join(seq)] += 1
    print("order of roles per CU (S sort, P pair) : number of CUs")
    for k, v in sorted(orders.items(), key=lambda kv: -kv[1])[:12]:
        print(f"  {k:12s} {v}")
    return res


def tile_xcds(rows):
    """the XCDs of the pair workgroups of every event tile (two workgroups of 2048 positions per
    4096-event tile), through the kernel's own block order where the library has one"""
    n_pair = grid - n_tiles
    logical = np.arange(n_pair)
    if hasattr(lib, "sdm_debug_walk_block_map") and os.environ.get("SDM_WALK_LOCAL", "1") != "0":
        buf = (ctypes.c_int * n_pair)()
        assert lib.sdm_debug_walk_block_map(n_pair, 2, buf) == 0
        logical = np.array(buf[:], dtype=np.int64)
    xcc = (rows[:, 3] >> 32) & 0xF
    block = np.arange(grid)
    share = float(np.mean(xcc[8:] == xcc[:-8]))
    print(f"workgroups b and b + 8 on the same XCD: {100 * share:.1f} % of {grid - 8}; "
          f"b and b + 1: {100 * float(np.mean(xcc[1:] == xcc[:-1])):.1f} %")
    print("XCD of workgroups 0..15:", xcc[:16].tolist(), " (b % 8 == XCD for "
          f"{100 * float(np.mean(xcc == block % 8)):.1f} %, (b % 8 - XCD) % 8 constant: "
          f"{len(set(((block - xcc) % 8).tolist())) == 1})")
    per_tile = defaultdict(set)
    for b in range(n_pair):
        per_tile[int(logical[b]) // 2].add(int(xcc[n_tiles + b]))
    counts = defaultdict(int)
    for xs in per_tile.values():
        counts[len(xs)] += 1
    print("XCDs per tile's pair workgroups: number of tiles",
          {k: counts[k] for k in sorted(counts)})
    for t in sorted(per_tile)[:8]:
        print(f"  tile {t}: XCDs {sorted(per_tile[t])}")


print("--- launch 0 ---")
describe(runs[0], True)
tile_xcds(runs[0])
print("--- medians over", len(runs), "launches ---")
all_res = [describe(r, False) for r in runs]
for k in all_res[0]:
    print(f"  {k:18s} {np.median([r[k] for r in all_res]):7.2f} us")
sys.stdout.flush()

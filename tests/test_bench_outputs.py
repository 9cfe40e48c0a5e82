"""bench.py --dump-outputs on the CPU checker: what the timed path left, as float64 .npy files,
the same from run to run, within the size budget (a seeded sample of the per-droplet columns
above it)"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_of_a_box_is_its_whole_state(oracle_engine, tmp_path):
    bench = _bench()
    runner = bench.build_workload("shima", oracle_engine, 0, 1, n_sd=2**12, adaptive=True)
    runner.run(3)
    snap = bench.timed_path_outputs(runner)
    bench.dump_outputs(snap, str(tmp_path))
    names = {p.name for p in tmp_path.iterdir()}
    assert {"idx.npy", "length.npy", "multiplicity.npy", "attributes.npy",
            "collision_rate.npy"} <= names
    for name in names:
        assert np.load(tmp_path / name).dtype == np.float64
        assert np.isfinite(np.load(tmp_path / name)).all(), name
    # (NaN from the start and NaN-sticky, as the reference's: no value the step computed)
    assert np.isnan(snap["stats_dt_min"]).all() and "stats_dt_min.npy" not in names
    length = int(np.load(tmp_path / "length.npy"))
    np.testing.assert_array_equal(np.load(tmp_path / "idx.npy"), snap["idx"][:length])
    np.testing.assert_array_equal(np.load(tmp_path / "multiplicity.npy"), snap["multiplicity"])
    np.testing.assert_array_equal(np.load(tmp_path / "attributes.npy"), snap["attributes"])


def test_dump_above_the_budget_is_a_fixed_sample(oracle_engine, tmp_path, monkeypatch):
    bench = _bench()
    budget = 200_000
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_MIN", 4096)
    for out in ("a", "b"):
        flow = bench.build_workload("kinematic2d_flow", oracle_engine, 0, 1, n_sd=2**13,
                                    grid=(4, 4))
        flow.run(3)
        bench.dump_outputs(bench.timed_path_outputs(flow), str(tmp_path / out))
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert {"idx.npy", "multiplicity.npy", "attributes.npy", "cell_id.npy", "cell_origin.npy",
            "position_in_cell.npy", "cell_start.npy"} <= set(names)
    data = sum(np.load(tmp_path / "a" / name).nbytes for name in names)
    assert data <= budget
    kept = np.load(tmp_path / "a" / "multiplicity.npy").shape[-1]
    assert 0 < kept < 2**13
    assert np.load(tmp_path / "a" / "position_in_cell.npy").shape == (2, kept)
    assert "stats_dt_min.npy" not in names
    for name in names:
        assert np.isfinite(np.load(tmp_path / "a" / name)).all(), name
        np.testing.assert_array_equal(np.load(tmp_path / "a" / name),
                                      np.load(tmp_path / "b" / name), err_msg=name)

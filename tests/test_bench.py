"""bench.py's own contract: --steps, --dump-outputs and the plain (not --full) result line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("ref_id", "query_id", "ab", "ae", "bb", "be", "score", "comp", "emitted", "first_tile_score", "n_tiles", "cells")


def _records(n, seed=3):
    from gact_amd import engine
    rec = np.zeros(n, dtype=engine.OVERLAP_DTYPE)
    rng = np.random.default_rng(seed)
    for f in FIELDS:
        rec[f] = rng.integers(0, 1 << 30, n)
    rec["cells"] += 1 << 40
    return rec


def test_dump_outputs_writes_every_field_as_float64(tmp_path):
    import bench
    rec = _records(1000)
    bench.dump_outputs(str(tmp_path / "out"), rec)
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f + ".npy" for f in FIELDS)
    for f in FIELDS:
        a = np.load(tmp_path / "out" / (f + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, rec[f].astype(np.float64))


def test_dump_outputs_samples_the_same_rows_above_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 13 * 100)
    rec = _records(5000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rec)
    rows = np.load(tmp_path / "a" / "sample_rows.npy")
    assert len(rows) == 100 and np.array_equal(rows, np.load(tmp_path / "b" / "sample_rows.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / p) for p in os.listdir(tmp_path / "a")) < 8 * 13 * 100 + 13 * 256
    for f in FIELDS:
        assert np.array_equal(np.load(tmp_path / "a" / (f + ".npy")), rec[f][rows.astype(np.int64)].astype(np.float64))


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, cwd=ROOT,
                         timeout=120)
    assert out.returncode != 0 and "--steps" in out.stderr


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """a plain run: the line's contract fields, nothing of --full, and the records of the last timed step in the dump"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "ecoli10x_small", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0
    assert res["unit"] == "GCUPS" and res["higher_is_better"] is True and res["dtype"].startswith("int")
    assert res["config"]["passes_in_this_process"] == 4
    assert not {"roofline", "single_slot", "cpu_baseline", "parity", "config4_strong"} & set(res)
    n = res["config"]["candidates"]
    for f in FIELDS:
        a = np.load(tmp_path / "dump" / (f + ".npy"))
        assert a.dtype == np.float64 and a.shape == (n,)
    assert int(np.load(tmp_path / "dump" / "cells.npy").sum()) == res["config"]["cells_per_step"]
    assert np.load(tmp_path / "dump" / "emitted.npy").sum() > 0

"""bench.py's command line: the float forms and the row sample of
--dump-outputs (CPU), and one small plain run end to end (GPU): --steps is
the number of timed steps, the line carries ms_per_step and none of --full's
legs, and the dumped fold equals the oracle's fold of the same population."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u64(f):
    """Rejoin the (high, low) float64 halves of a dumped 8-byte integer array."""
    return (f[..., 0].astype(np.uint64) << np.uint64(32)) | f[..., 1].astype(np.uint64)


def test_dump_outputs_forms_and_sample(tmp_path, monkeypatch):
    import torch

    import bench
    edge = np.array([0, 1, 2**53 + 1, 2**63 - 1, -1, -2**63], np.int64)
    arrays = {"i64": torch.from_numpy(edge), "u64": edge.view(np.uint64).reshape(3, 2),
              "u32": np.array([0, 2**24 + 1, 2**32 - 1], np.uint32), "u8": torch.arange(256, dtype=torch.uint8)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    assert got["i64"].dtype == np.float64 and got["i64"].shape == (6, 2)
    np.testing.assert_array_equal(_u64(got["i64"]).view(np.int64), edge)
    assert got["u64"].shape == (3, 2, 2)
    np.testing.assert_array_equal(_u64(got["u64"]), edge.view(np.uint64).reshape(3, 2))
    assert got["u32"].dtype == np.float64
    np.testing.assert_array_equal(got["u32"].astype(np.uint32), arrays["u32"])
    assert got["u8"].dtype == np.float32
    np.testing.assert_array_equal(got["u8"], np.arange(256))

    # above the bound: the same sorted rows of equal-length arrays, the same in every run, within the bound
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100_000)
    big = {"k": np.arange(50_000, dtype=np.int64), "v": np.arange(50_000, dtype=np.uint32) * 3,
           "m": np.arange(7000, dtype=np.int64).reshape(1000, 7)}
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big)
    b = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in big}
    for k in big:
        np.testing.assert_array_equal(b[k], np.load(tmp_path / "c" / f"{k}.npy"))
    assert sum(os.path.getsize(tmp_path / "b" / f"{k}.npy") for k in big) <= 100_000
    rows = _u64(b["k"]).astype(np.int64)
    assert 0 < len(rows) < 50_000 and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(b["v"], rows * 3)
    m = _u64(b["m"]).astype(np.int64)
    assert m.shape[1] == 7 and 0 < m.shape[0] < 1000
    np.testing.assert_array_equal(m, m[:, :1] + np.arange(7))


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    from crdt_amd import synth
    from oracle import oracle
    rows, nodes = 100_003, 64
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--total-rows", str(rows), "--dump-outputs", str(tmp_path / "out")],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "replica-merges/s" and d["dtype"] == "u64" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0
    # value = rows per step / seconds per step (ms_per_step is rounded to 1e-4 ms, a step takes > 0.01 ms)
    assert d["value"] == pytest.approx(rows / (d["ms_per_step"] / 1e3), rel=1e-2)
    # a plain run has none of --full's legs
    assert d["cpu_baseline"] is None and d["e2e_pcie"] is None
    assert "copy" not in d["roofline"]["measured_peak"]
    assert os.listdir(tmp_path / "out") == ["fold.npy"]
    f = np.load(tmp_path / "out" / "fold.npy")
    assert f.dtype == np.float64 and f.shape == (nodes, 2)
    a = synth.counters(2024, 1, rows * nodes).reshape(rows, nodes)
    np.testing.assert_array_equal(_u64(f), oracle.gcounter_fold(a))

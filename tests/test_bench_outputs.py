"""bench.py --dump-outputs and --full: the row sampler on the CPU, and on the
GPU one small run whose dumped composites are the bytes its digests name, with
none of the --full measurements in a plain line."""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_full_is_off_by_default():
    assert bench.parse(["--gpus", "1", "--steps", "2", "--warmup", "1"]).full is False
    assert bench.parse(["--full"]).full is True
    assert bench.parse([]).dump_outputs is None


def test_sample_rows_takes_every_row_that_fits():
    flat = torch.arange(200, dtype=torch.uint8)
    got = bench.sample_rows(flat, [10, 100, 50], [3, 2, 4], seed=0)
    assert got.dtype == np.float32
    assert got.tolist() == [10, 11, 12, 100, 101, 50, 51, 52, 53]
    assert bench.sample_rows(flat, [], [], seed=0).shape == (0,)
    with pytest.raises(ValueError):
        bench.sample_rows(flat, [10, 198], [3, 3], seed=0)


def test_sample_rows_is_a_fixed_sample_within_the_budget(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4 * 1000)
    buf = np.random.default_rng(1).integers(0, 256, 64 * 97, np.uint8)
    starts, lens = np.arange(64) * 97, np.full(64, 90)     # 64 rows of 90 of a 97-byte pitch
    a = bench.sample_rows(torch.from_numpy(buf), starts, lens, seed=3)
    b = bench.sample_rows(torch.from_numpy(buf), starts, lens, seed=3)
    assert a.size == 11 * 90 and np.array_equal(a, b)       # 11 whole rows fit 1000 values
    rows = buf.reshape(64, 97)[:, :90]
    picked = [int(np.flatnonzero((rows == r).all(axis=1))[0]) for r in a.reshape(11, 90).astype(np.uint8)]
    assert picked == sorted(set(picked))                    # distinct rows, in row order
    c = bench.sample_rows(torch.from_numpy(buf), starts, lens, seed=4)
    assert not np.array_equal(a, c)


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_and_skips_the_full_legs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--size", "256", "--batch", "6", "--backgrounds", "3", "--dump-outputs", str(tmp_path / "o"),
                        "--dump-digests", str(tmp_path / "d.json")],
                       capture_output=True, text=True, timeout=300, env=env, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "Mpix/s" and line["dtype"] == "u8"
    for k in ("stream", "cpu_baseline", "workloads"):
        assert k not in line
    assert "copy_ceiling" not in line["roofline"]
    assert [f.name for f in (tmp_path / "o").iterdir()] == ["composites.npy"]
    out = np.load(tmp_path / "o" / "composites.npy")
    assert out.dtype == np.float32 and out.size == 6 * 256 * 256 * 3
    digests = json.loads((tmp_path / "d.json").read_text())
    for i, item in enumerate(out.reshape(6, -1)):
        assert hashlib.sha1(item.astype(np.uint8).tobytes()).hexdigest() == digests[str(i)], i

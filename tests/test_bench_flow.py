"""bench.py's own multi-rank control flow on CPU: `python bench.py --gpus 2` with PIO_BENCH_STUB=1 spawns the ranks
through torch.distributed.run exactly as the driver's launch does (bench.spawn_ranks), every rank builds its own inputs,
steps, all-gathers through perceiverio_pytorch_amd.dist.all_gather_rows, the timed region is bracketed by barriers and
reduced with MAX, and rank 0 alone prints the JSON line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("gpus", [1, 2])
def test_bench_main_control_flow_stub(gpus):
    env = dict(os.environ, PIO_BENCH_STUB="1", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "3",
                          "--warmup", "1", "--batch", "4"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line (rank 0): {out.stdout[-500:]}"
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == gpus and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["config"]["global_batch"] == 4 * gpus and rec["data"] == "stub"
    assert rec["gather_ok"] is True
    assert rec["value"] > 0 and rec["scaling"] == "weak" and rec["higher_is_better"] is True


def test_bench_dump_outputs_stub(tmp_path):
    """--dump-outputs DIR writes the last timed step's outputs as float32 .npy files, the same from run to run."""
    import numpy as np
    env = dict(os.environ, PIO_BENCH_STUB="1", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                              "--warmup", "1", "--batch", "4", "--dump-outputs", str(d)],
                             env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        a = np.load(d / "output.npy")
        assert a.dtype == np.float32 and a.shape == (4, 10)
        dumps.append(a)
    assert np.array_equal(dumps[0], dumps[1])


def test_dump_outputs_samples_large_arrays(tmp_path):
    """An output above the per-array cap is written as the same fixed sample every time; a dict writes one file per key."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    big = torch.arange(bench.DUMP_MAX_ELEMS + 1000, dtype=torch.float32).reshape(-1, 8)
    small = torch.ones(3, 5, dtype=torch.float64)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"big": big, "small": small, "none": None}, "multimodal")
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and 0 < a.size <= bench.DUMP_MAX_ELEMS and np.array_equal(a, b)
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (3, 5)
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy"]

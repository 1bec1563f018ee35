"""CPU: bench.py's N>1 code path itself (2 ranks, gloo, --dry-run) so that the first real multi-GPU run is not the first execution of
the sharding / gather / max-over-ranks / JSON code.  Both launch forms: the documented `python -m torch.distributed.run ... bench.py
--gpus N` and the plain `python bench.py --gpus N` the driver's N=1 record shows (bench.py then starts its own N ranks)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_dry_run():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "3",
           "--max-boxes", "512", "--dry-run"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                         # rank 0 prints ONE JSON line
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["warmup"] == 1 and j["scaling"] == "weak" and j["dry_run"] is True
    assert j["gather_ok"] is True and j["config"]["global_batch"] == 6 and j["value"] > 0
    # counts first, then only the rows any rank filled: far below the 512-row capacity of the decode block
    assert 0 < j["gather_message_bytes_per_rank"] <= 3 * 400 * 112 * 4 + 3 * 4 + 8
    # the steady-state form: the whole capacity block in ONE collective (tests/test_dist.py asserts it contains no host synchronisation)
    assert j["static_gather_ok"] is True and j["static_gather_message_bytes_per_rank"] == 3 * 512 * 112 * 4


def test_bench_single_rank_dry_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "2", "--warmup", "1", "--batch", "2",
                        "--max-boxes", "512"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert j["n_gpus"] == 1 and j["gather_ok"] is True


def test_train_bench_two_ranks_dry_run():
    """bench.py --train --dry-run with 2 ranks under gloo: the bucketed gradient all-reduce (findtextcenternet_amd.dist.BucketedAllReduce),
    max-over-ranks timing and the JSON line of the train bench."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--train", "--dry-run", "--batch", "8"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["allreduce_ok"] is True and j["buckets"] == 3 and j["config"]["global_batch"] == 16


def test_plain_python_bench_gpus_2_launches_its_own_ranks():
    """`python bench.py --gpus 2 --dry-run` with no launcher and no WORLD_SIZE: bench.py re-executes itself under torch.distributed.run
    (one process per GPU); ONE JSON line, last on stdout, n_gpus 2."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "3",
                        "--max-boxes", "512", "--dry-run"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [ln for ln in r.stdout.splitlines() if ln.strip()]
    lines = [ln for ln in out if ln.startswith("{")]
    assert len(lines) == 1 and out[-1] == lines[0], r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["gather_ok"] is True and j["static_gather_ok"] is True and j["config"]["global_batch"] == 6


def test_plain_python_train_bench_gpus_2_launches_its_own_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--train", "--gpus", "2", "--dry-run", "--batch", "8"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [ln for ln in r.stdout.splitlines() if ln.strip()]
    lines = [ln for ln in out if ln.startswith("{")]
    assert len(lines) == 1 and out[-1] == lines[0], r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["allreduce_ok"] is True and j["config"]["global_batch"] == 16


def test_mismatched_world_size_is_refused():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], capture_output=True, text=True, timeout=120,
                       cwd=ROOT, env=env)
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_dump_outputs_writes_comparable_float_arrays(tmp_path):
    """The --dump-outputs helpers on CPU tensors: rows past a tile's count are zeroed and the rest put in map order, integers become
    float64, and an array above the size cap becomes the same seeded sample in every run."""
    import numpy as np
    import torch
    import bench
    rec = torch.full((2, 4, 112), 7.0)
    for b, rows in enumerate([[(3, 1), (1, 2), (2, 1)], [(5, 5)]]):
        for i, (ix, iy) in enumerate(rows):
            rec[b, i, 1], rec[b, i, 2], rec[b, i, 12] = ix, iy, 10 * ix + iy
    a = bench.decoded_arrays(torch.tensor([3, 1], dtype=torch.int32), rec)
    assert a["boxes"][0, :3, 1].tolist() == [2, 3, 1] and a["boxes"][0, :3, 2].tolist() == [1, 1, 2]
    assert a["box_features"][0, :3, 0].tolist() == [21, 31, 12] and a["box_features"].shape == (2, 4, 100)
    assert not a["boxes"][0, 3:].any() and not a["boxes"][1, 1:].any() and a["boxes"][1, 0, 1] == 5
    big = np.arange(bench.DUMP_ARRAY_BYTES // 4 + 1000, dtype=np.float32)
    for d in ("d1", "d2"):
        bench.dump_outputs(str(tmp_path / d), {**a, "big": big})
    for name in ("counts", "boxes", "box_features", "big"):
        x1, x2 = np.load(tmp_path / "d1" / f"{name}.npy"), np.load(tmp_path / "d2" / f"{name}.npy")
        assert x1.dtype in (np.float32, np.float64) and np.array_equal(x1, x2)
    s = np.load(tmp_path / "d1" / "big.npy")
    assert s.nbytes == bench.DUMP_ARRAY_BYTES and np.all(np.diff(s) > 0)
    assert np.load(tmp_path / "d1" / "counts.npy").dtype == np.float64
    # the NMS channel's -inf (non-peak) entries: written as 0 beside a 0/1 peak map; any other non-finite output is refused
    heat = torch.randn(2, 4, 4, 10)
    heat[..., 1][heat[..., 1] < 0.5] = float("-inf")
    h = bench.heatmap_arrays(heat)
    peak = torch.isfinite(heat[..., 1]).numpy()
    assert np.array_equal(h["nms_peak_mask"], peak.astype(np.float32)) and np.isfinite(h["heatmap"]).all()
    assert np.array_equal(h["heatmap"][..., 1][peak], heat[..., 1].numpy()[peak]) and not h["heatmap"][..., 1][~peak].any()
    assert np.array_equal(np.delete(h["heatmap"], 1, axis=3), np.delete(heat.numpy(), 1, axis=3))
    bench.dump_outputs(str(tmp_path / "d3"), h)
    with pytest.raises(ValueError, match="non-finite"):
        bench.dump_outputs(str(tmp_path / "d4"), {"heatmap": heat.numpy()})

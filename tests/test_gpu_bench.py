"""bench.py's multi-rank contract on the GPU box.

``bench.py --gpus 2`` run OUTSIDE torchrun must start the ranks itself (a
child torchrun, no exec) and print ``n_gpus: 2`` with a verified CRC of
every slice of the last fan-out.  The 1-GPU box cannot give RCCL two GPUs,
so the rehearsal uses gloo, whose collectives ShardedLoader stages through
host memory; the RCCL path is the same loader with device tensors.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(tmp_path, *extra, full=True):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1",
           "--window-mib", "64", "--file-gib", "0.25", "--lat-samples", "100",
           "--dir", str(tmp_path), *(["--full"] if full else []), *extra]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_two_ranks_self_launch_gloo(tmp_path):
    out = _run_bench(tmp_path, "--gpus", "2", "--backend", "gloo")
    assert out["n_gpus"] == 2
    assert out["rccl"]["world_size"] == 2
    assert out["rccl"]["allgather_verified"] is True
    assert out["verified_crc32c"] is True
    assert len(out["per_rank"]["load_GiBps_per_rank"]) == 2
    assert out["config"]["parallelism"] == "dp2+allgather"
    # every timed step's gathered shards delivered and slice-checked
    assert out["rccl"]["delivered_steps"] == 2 and out["rccl"]["per_step_slice_check"] is True
    assert out["per_rank"]["delivered_steps_per_rank"] == [2, 2]


@pytest.mark.gpu
def test_bench_single_rank_contract(tmp_path):
    out = _run_bench(tmp_path)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1
    assert out["verified_crc32c"] is True and out["value"] > 0
    assert out["full"] is True


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_window(tmp_path):
    """A plain run reports the headline only, and ``--dump-outputs`` writes
    the bytes the last timed step left in HBM: they equal the shard file's."""
    import numpy as np
    dump = tmp_path / "dump"
    out = _run_bench(tmp_path, "--keep", "--dump-outputs", str(dump), full=False)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "config"):
        assert k in out, k
    assert out["full"] is False and out["steps"] == 2 and out["value"] > 0
    W = 64 << 20
    assert abs(out["ms_per_step"] - W / (out["value"] * (1 << 30)) * 1e3) < 0.01 * out["ms_per_step"]
    # nothing of the other measurements ran
    for k in ("vs_baseline", "vfs_control_GiBps", "storage_seq_GiBps", "p50_4k_lat_us",
              "host_costs_ns", "verified_crc32c"):
        assert k not in out, k
    offs = np.load(dump / "window_offsets.npy")
    got = np.load(dump / "window_sample_r0.npy")
    crc = np.load(dump / "window_crc32c_r0.npy")
    assert got.dtype == np.float32 and offs.dtype == np.float64 and crc.dtype == np.float64
    assert sum(f.stat().st_size for f in dump.iterdir()) <= 64_000_000
    # steps 0..2 of a 4-window shard: the last timed step loaded window 2
    shard = np.fromfile(tmp_path / "shard_r0.bin", dtype=np.uint8)
    assert shard.size == 4 * W
    win = shard[2 * W:3 * W]
    idx = offs.astype(np.int64)
    assert len(idx) == len(got) > 1 << 20 and (np.diff(idx) > 0).all() and idx[-1] < W
    assert np.array_equal(got, win[idx].astype(np.float32))
    import nvme_strom_amd as S
    assert int(crc[0]) == S.crc32c_host(win.tobytes())

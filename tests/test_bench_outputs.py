"""bench.py's --dump-outputs and --full: the dump holds what the timed path left
in its output buffers (checked on the CPU with stand-in tensors, and on the
GPU through one small run of the benchmark itself), and a plain run carries no
CPU baseline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "reed-solomon-novelpoly_amd", "python")]


def _buffers(batch=3, n=8, wanted_n=6, sl=10, out_len=20):
    import torch

    g = torch.Generator().manual_seed(7)
    shards = torch.randint(0, 256, (batch, n, sl), dtype=torch.uint8, generator=g)
    out = torch.randint(0, 256, (batch, out_len), dtype=torch.uint8, generator=g)
    return shards, wanted_n, out


def test_dump_outputs_whole_arrays(tmp_path):
    """Arrays within the sample size are written whole, as float32, without the
    rows encode never produces; the row sums cover every byte."""
    import bench

    shards, wn, out = _buffers()
    bench.dump_outputs(str(tmp_path), 0, 1, shards, wn, out)
    assert sorted(os.listdir(tmp_path)) == ["reconstructed.npy", "reconstructed_rowsum.npy", "shards.npy",
                                            "shards_rowsum.npy"]
    got = np.load(tmp_path / "shards.npy")
    assert got.dtype == np.float32
    assert np.array_equal(got, shards[:, :wn].numpy().reshape(-1).astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "reconstructed.npy"), out.numpy().reshape(-1).astype(np.float32))
    rs = np.load(tmp_path / "shards_rowsum.npy")
    assert rs.dtype == np.float64 and rs.shape == (3, wn)
    assert np.array_equal(rs, shards[:, :wn].numpy().astype(np.float64).sum(-1))
    assert np.array_equal(np.load(tmp_path / "reconstructed_rowsum.npy"), out.numpy().astype(np.float64).sum(-1))


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    """Above the sample size the dump is a seeded sample: the same positions in
    every run, each value the byte at its position."""
    import bench

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 50)
    shards, wn, out = _buffers()
    bench.dump_outputs(str(tmp_path / "a"), 0, 1, shards, wn, out)
    changed = shards.clone()
    changed[:, wn:] ^= 0xFF  # rows that are never produced do not enter the dump
    bench.dump_outputs(str(tmp_path / "b"), 1, 2, changed, wn, out)
    a, b = np.load(tmp_path / "a" / "shards.npy"), np.load(tmp_path / "b" / "shards_rank1.npy")
    assert a.shape == (50,) and np.array_equal(a, b)
    flat = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, 3 * wn * 10, 50, dtype=np.int64))
    assert np.array_equal(a, shards[:, :wn].numpy().reshape(-1)[flat].astype(np.float32))
    assert np.load(tmp_path / "a" / "reconstructed.npy").shape == (50,)  # 60 elements: sampled too


def test_dump_outputs_many_shards_sum_per_payload(tmp_path, monkeypatch):
    """With more shards than half the sample size the shard sums are folded
    to one per payload, so the dump stays bounded at any shape."""
    import bench

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 20)
    shards, wn, out = _buffers()  # 18 shards > 10
    bench.dump_outputs(str(tmp_path), 0, 1, shards, wn, out)
    rs = np.load(tmp_path / "shards_rowsum.npy")
    assert np.array_equal(rs, shards[:, :wn].numpy().astype(np.float64).sum((1, 2)))
    assert np.load(tmp_path / "reconstructed_rowsum.npy").shape == (3,)


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_plain_run_dumps_its_outputs(tmp_path):
    """One small plain run of the benchmark: the line has ms_per_step for the
    steps asked for and no CPU baseline, and the dumped reconstruction is the
    synthetic payloads (whole arrays at this size: 16 payloads of 64 KiB)."""
    from novelpoly_amd import synth

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--config", "2", "--batch", "16", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["roundtrip_ok"]
    # both figures are rounded in the line (ms_per_step to 1e-4 ms of a step of some 0.1 ms)
    assert line["value"] == pytest.approx(16 * 65536 / (line["ms_per_step"] / 1e3) / 2**30, rel=0.02)
    assert "cpu_baseline" not in line
    plen = 64 * 1024
    want = np.stack([synth.payload_array(i, plen) for i in range(16)])
    rec = np.load(tmp_path / "reconstructed.npy")
    assert rec.dtype == np.float32 and np.array_equal(rec.reshape(16, -1)[:, :plen], want.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "reconstructed_rowsum.npy"),
                          rec.reshape(16, -1).astype(np.float64).sum(-1))
    sh = np.load(tmp_path / "shards.npy")
    assert sh.shape == (16 * 256 * (plen // 64),)
    assert np.array_equal(np.load(tmp_path / "shards_rowsum.npy"), sh.reshape(16, 256, -1).astype(np.float64).sum(-1))

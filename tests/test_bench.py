"""bench.py's command line: a plain run times the headline config only, --full adds the other measurements
and checks, --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("verified", "bit_exact_vs_reference", "lmkcdey", "config3", "small_batch", "ntt_roofline", "copy_bw",
             "cpu_baseline")


def test_bench_options(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 1, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


@pytest.mark.parametrize("B", [5, 20000])
def test_dump_outputs_sample_is_fixed_and_float64(tmp_path, B):
    """all of b, and the a rows of the same seeded sample of at most DUMP_ROWS gates on every call"""
    import bench
    import torch
    n = 7
    ao = torch.arange(B * n, dtype=torch.int64).reshape(B, n)
    bo = torch.arange(B, dtype=torch.int64) + (1 << 40)
    bench.dump_outputs(torch, ao, bo, str(tmp_path / "x"))
    bench.dump_outputs(torch, ao, bo, str(tmp_path / "y"), "_rank1")
    a, b = np.load(tmp_path / "x" / "out_a.npy"), np.load(tmp_path / "x" / "out_b.npy")
    assert a.dtype == b.dtype == np.float64
    assert a.shape == (min(B, bench.DUMP_ROWS), n) and b.shape == (B,)
    assert np.array_equal(b, bo.numpy())
    rows = (a[:, 0] / n).astype(np.int64)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, ao.numpy()[rows])
    assert np.array_equal(a, np.load(tmp_path / "y" / "out_a_rank1.npy"))
    assert a.nbytes + b.nbytes <= 64 << 20 and bench.DUMP_ROWS * 504 * 8 + 65536 * 8 <= 64 << 20


@pytest.mark.gpu
def test_gpu_plain_bench_line_and_dumped_outputs(tmp_path):
    """a plain run of a small batch: the headline fields and none of the --full objects; the dumped arrays
    are the engine's outputs for the same seeded inputs"""
    import bench
    from fhe_amd import binfhe as bf
    total, steps = 1536, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--total", str(total), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "bootstraps/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["value"] == pytest.approx(total / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in line]
    a, b = np.load(tmp_path / "out_a.npy"), np.load(tmp_path / "out_b.npy")
    assert a.dtype == b.dtype == np.float64 and a.shape == (total, 503) and b.shape == (total,)
    keys, x1, x2, a1, b1, a2, b2 = bench.make_inputs(bf, bf.STD128, bf.GINX, total)
    eng = bf.GateEngine(bf.STD128, bf.GINX, device=0)
    eng.load_keys(keys.bsk, keys.kskA, keys.kskB)
    ao, bo = eng.eval_gate(bf.AND, a1, b1, a2, b2)
    eng.close()
    assert np.array_equal(a, ao.astype(np.float64)) and np.array_equal(b, bo.astype(np.float64))
    assert np.array_equal(bf.decrypt(bf.STD128, bf.GINX, keys.sk, ao, bo), (x1 & x2).astype(np.int64))


@pytest.mark.gpu
def test_gpu_full_bench_line_has_every_object():
    """--full on a small batch (CPU baselines and one-gate latencies left out: they take a minute): the headline
    fields as in a plain run, the outputs checked, configs 5, 3 and 2 measured"""
    total = 1536
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--total", str(total), "--full", "--no-cpu-baseline", "--no-small-batch"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip())
    assert line["value"] == pytest.approx(total / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k != "small_batch" and k not in line]
    assert line["verified"] is True and line["lmkcdey"]["verified"] is True
    assert line["config3"]["verified"] is True and line["config3"]["bit_exact_vs_reference"] is True
    assert len(line["ntt_roofline"]) == 4 and line["cpu_baseline"] is None

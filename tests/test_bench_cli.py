"""bench.py's command line: a plain run times its steps and nothing else,
--full adds the parity check (and, unless switched off, the CPU baseline and
the copy ceiling), --dump-outputs writes what the last timed step returned.

CPU: the sampling behind --dump-outputs (fixed positions, float32, bounded).
GPU: one plain run and one --full run of config 2 (2^20 x 256 B frames, one
copy, three timed steps), the dumped digest checked against the reference's
(tests/golden/configs.json).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")


def test_dump_sample_is_fixed_bounded_float32():
    import bench
    small = torch.arange(200, dtype=torch.uint8)
    a = bench.dump_sample(torch, small, limit=256)
    assert a.dtype == np.float32 and a.tolist() == list(range(200))      # whole when it fits
    big = (torch.arange(100_000, dtype=torch.int64) * 7 % 251).to(torch.uint8)
    b = bench.dump_sample(torch, big, limit=1000)
    assert b.dtype == np.float32 and b.shape == (1000,)
    assert np.array_equal(b, bench.dump_sample(torch, big.clone(), limit=1000))   # same positions every time
    idx = np.sort(np.random.default_rng([bench.DUMP_SEED, big.numel()]).integers(0, big.numel(), size=1000))
    assert np.array_equal(b, big.numpy()[idx].astype(np.float32))
    assert 4 * (2 * bench.DUMP_SAMPLE + bench.DUMP_SAMPLE // 2) + 1024 <= 64 << 20   # all arrays of a dump


def run_bench(*extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--settle", "2", "--config", "c2", "--copies", "1", *extra],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_only_and_dumps_the_last_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = run_bench("--dump-outputs", str(tmp_path))
    assert out["steps"] == 3 and out["warmup"] == 2 and out["full"] is False
    assert out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "GiB/s" and out["dtype"] == "u8"
    assert out["higher_is_better"] is True
    assert out["parity"] is None and out["cpu_baseline"] is None and out["roofline"]["copy_ceiling"] is None
    arrays = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(arrays) == ["batch", "batch_digest", "batch_unmasked", "decode_count"]
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    # 2 warm-up + 3 timed decodes of the one copy: unmasked payloads
    assert arrays["decode_count"].tolist() == [5.0]
    digest = sum(int(x) << (16 * i) for i, x in enumerate(arrays["batch_digest"]))
    assert digest == load_golden("configs.json")["configs"]["c2_bin_256"]["out_digest"]
    assert arrays["batch"].shape == (4 << 20,) and np.array_equal(arrays["batch"], arrays["batch_unmasked"])
    assert arrays["batch"].min() >= 0 and arrays["batch"].max() <= 255


@pytest.mark.gpu
def test_full_run_checks_parity():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = run_bench("--full", "--no-cpu", "--no-ceiling")
    assert out["full"] is True and out["parity"] is True and out["steps"] == 3
    assert out["cpu_baseline"] is None and out["roofline"]["copy_ceiling"] is None

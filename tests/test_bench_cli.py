"""bench.py command line: --dump-outputs and --full on the toy-scale dry run."""
import json
import os
import subprocess
import sys

import numpy as np


def test_bench_dump_outputs_and_full(tmp_path):
    """One single-process FD_BENCH_TINY run: the result line keeps its keys,
    --steps sets the timed step count, and the dump holds float arrays."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    # the toy model is a CPU plumbing run: hide any GPU from the child
    env.update({"FD_BENCH_TINY": "1", "HIP_VISIBLE_DEVICES": "",
                "CUDA_VISIBLE_DEVICES": ""})
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1",
           "--steps", "2", "--warmup", "1", "--full",
           "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                         env=env, cwd=repo)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines()
                      if l.startswith("{")][-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                "ms_per_step"):
        assert key in rec
    assert rec["steps"] == 2
    assert rec["ms_per_step"] > 0
    assert rec["value"] > 0

    names = sorted(p.name for p in dump.iterdir())
    assert names == ["ema_params.npy", "loss.npy", "params.npy"]
    total = 0
    arrays = {}
    for n in names:
        a = np.load(dump / n)
        assert a.dtype in (np.float32, np.float64)
        assert np.isfinite(a).all()
        total += a.nbytes
        arrays[n] = a
    assert total <= 64 * 1024 * 1024
    assert float(arrays["loss.npy"][0]) == rec["config"]["final_loss"]
    assert arrays["params.npy"].shape == arrays["ema_params.npy"].shape
    # three optimizer steps moved the masters away from their EMA
    assert np.abs(arrays["params.npy"] - arrays["ema_params.npy"]).max() > 0

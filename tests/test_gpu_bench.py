"""`bench.py` on the GPU as a caller runs it: a plain run times exactly --steps steps in one window and nothing else, and
`--dump-outputs DIR` writes what the last timed step computed — the same arrays, bit for bit, from two runs with the same arguments
(what lets two builds of the project be compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "CTF_BENCH_DRYRUN")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(argv), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    E, K = 4096, 6
    argv = ["--envs-per-gpu", str(E), "--steps", str(K), "--warmup", "3"]
    lines, outs = [], []
    for i in range(2):
        d = tmp_path / f"run{i}"
        lines.append(_bench(*argv, "--dump-outputs", str(d)))
        outs.append(_load(d))
    for line in lines:
        assert line["steps"] == K and line["windows"] == 1 and line["full"] is False and line["device_status_bits"] == 0
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(E * 1e3 / line["ms_per_step"], rel=1e-9)
        assert "secondary" not in line and "cpu_baseline" not in line and "roofline" not in line
    a, b = outs
    assert sorted(a) == ["done", "meta", "obs", "rewards"]
    n = 8  # 8_arena: 4 v 4
    assert a["rewards"].shape == (E, n) and a["done"].shape == (E,)
    assert a["obs"].shape[:2] == (256, n) and a["meta"].shape == (256, n, 2 * n + 6)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
    assert set(np.unique(a["done"])) <= {0.0, 1.0} and set(np.unique(a["obs"])) <= {0.0, 1.0} and a["obs"].any()

"""What a scattered reset costs beside a plain one (profiles/r22_scatter_reset.md): ``reset()`` and ``reset_scattered(radius=2)`` on
65 536 arena envs, each for all envs and under the sparse mask of the staggered bench (envs whose phase e % GAME_STEPS hits this step:
about 131 of 65 536).  A sample is the device time of ``--inner`` back-to-back calls between two events, divided by their number (one
call is a few tens of microseconds: a window of one would measure the clock); the figure is the median of ``--calls`` samples after
``--warmup`` warm-up samples, the four cases taken in turn inside every round so that a drift of the machine meets them alike.

    python tools/scatter_bench.py --out profiles/r22_scatter_reset.json
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--log-metrics", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    pkg = importlib.import_module("marl-ctf-development_amd")
    if not torch.cuda.is_available():
        raise SystemExit("scatter_bench needs a GPU: a CPU run measures nothing")
    kw = dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii)
    E = args.envs
    vec = pkg.VecGridworldCtf(E, device=0, tune_placement=False, rng_mode="counter_direct", log_metrics=bool(args.log_metrics), py_seeds=np.arange(E),
                              np_seeds=np.arange(E), **kw)
    period = int(vec.cfg.game_steps)
    sparse = torch.from_numpy((np.arange(E) % period == 7).astype(np.uint8)).to(vec.device)
    episodes = torch.zeros((E,), dtype=torch.uint32, device=vec.device)
    cases = {
        "reset_all": lambda: vec.reset(),
        "scattered_all": lambda: vec.reset_scattered(radius=args.radius, seed=1, episodes=episodes),
        "reset_sparse": lambda: vec.reset(sparse),
        "scattered_sparse": lambda: vec.reset_scattered(mask=sparse, radius=args.radius, seed=1, episodes=episodes),
    }
    samples = {k: [] for k in cases}
    for rnd in range(args.warmup + args.calls):
        for name, fn in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            torch.cuda.synchronize(vec.device)
            if rnd >= args.warmup:
                samples[name].append(a.elapsed_time(b) * 1e3 / args.inner)  # microseconds per call
    assert vec.status() == 0
    med = {k: statistics.median(v) for k, v in samples.items()}
    result = dict(device=torch.cuda.get_device_name(0), envs=E, radius=args.radius, log_metrics=bool(args.log_metrics), masked_envs=int(sparse.sum()),
                  calls=args.calls, warmup=args.warmup, inner=args.inner, median_us=med,
                  min_us={k: min(v) for k, v in samples.items()}, max_us={k: max(v) for k, v in samples.items()},
                  ratio_all=med["scattered_all"] / med["reset_all"], ratio_sparse=med["scattered_sparse"] / med["reset_sparse"])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""A/B of ctf_step_observe's two paths IN ONE PROCESS on the SAME handle and buffers: the single launch (k_step_observe) and the
two launches (k_step, then k_observe_tiles), chosen per call by CTF_STEP_OBSERVE_ONE_LAUNCH.  Windows of --steps calls alternate
between the paths (A B A B ...); each window's time / steps is one sample.  Prints one JSON line: per-path medians (ms per
step), their ratio and every window.  Usage (GPU box):  python tools/one_launch_ab.py [--envs 65536] [--windows 7] [--steps 200]
"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
pkg = importlib.import_module("marl-ctf-development_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--workload", default="arena", choices=("arena", "arena20"))
args = ap.parse_args()
kw = (dict(pkg.configs.ARENA20_KWARGS, SCENARIO=pkg.configs.arena20_scenario()) if args.workload == "arena20"
      else dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii))
E = args.envs
vec = pkg.VecGridworldCtf(E, device=0, py_seeds=np.arange(E), np_seeds=np.arange(E), **kw)
ACTS = torch.empty((64, E, vec.N_AGENTS), dtype=torch.int8, device="cuda")
for t in range(64):
    vec.random_actions(ACTS[t], seed=0xC7F, step=t)
PATHS = {"one_launch": "1", "two_launches": "0"}
launches = {}
for name, v in PATHS.items():
    os.environ["CTF_STEP_OBSERVE_ONE_LAUNCH"] = v
    launches[name] = vec.step_observe_launches()
    for t in range(20):  # warm-up of either path
        vec.step_observe(ACTS[t % 64], auto_reset=True)
torch.cuda.synchronize()
res = {k: [] for k in PATHS}
step = 0
for w in range(args.windows):
    for name, v in (PATHS.items() if w % 2 == 0 else reversed(list(PATHS.items()))):
        os.environ["CTF_STEP_OBSERVE_ONE_LAUNCH"] = v
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            vec.step_observe(ACTS[step % 64], auto_reset=True)
            step += 1
        b.record()
        torch.cuda.synchronize()
        res[name].append(a.elapsed_time(b) / args.steps)
med = {k: float(np.median(x)) for k, x in res.items()}
print(json.dumps({"envs": E, "workload": args.workload, "steps_per_window": args.steps, "launches": launches,
                  "ms_per_step_median": med, "one_over_two": med["one_launch"] / med["two_launches"],
                  "env_steps_per_s": {k: E / (m * 1e-3) for k, m in med.items()},
                  "windows_ms": {k: [round(x, 5) for x in v] for k, v in res.items()}, "status": vec.status()}), flush=True)

"""What harvesting the visitation maps costs next to the step: ctf_harvest_visitation / ctf_export_visitation at 65 536 8_arena
envs, in ONE process on ONE observation buffer, the variants interleaved call by call (the A/B form of tools/harvest_bench.py).

  sparse  phases staggered as bench.py staggers them (~131 envs end per step), 64 groups in runs:
          (a) step_observe + harvest   (b) the same + harvest_visitation
  dense   a lockstep batch at its last step (all envs ended), 64 groups as runs and alternating: harvest_visitation against
          vec.visitation() + index_add_ on the same state, and vec.visitation() alone with its achieved bytes per second

HIP-event time per call, medians over --calls calls after warm-up, --reps repetitions; one JSON document on stdout (and --out).

    python tools/visitation_bench.py --out profiles/r08_visitation_bench.json
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--calls", type=int, default=120)
    ap.add_argument("--dense-calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench

    pkg = importlib.import_module("marl-ctf-development_amd")
    kw = dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii)
    E, G = args.envs, args.groups
    seeds = np.arange(E, dtype=np.uint64) + 1
    vec = pkg.VecGridworldCtf(E, device=0, py_seeds=seeds, np_seeds=seeds, **kw)
    dev, gs, N, g = vec.device, int(vec.cfg.game_steps), vec.N_AGENTS, vec.GRID_SIZE
    acts = torch.empty((E, N), dtype=torch.int8, device=dev)
    vec.observe()
    env = torch.arange(E, device=dev)
    layouts = {"runs": (env // max(E // G, 1)).clamp(max=G - 1).to(torch.int32), "alternating": (env % G).to(torch.int32)}
    acc = torch.zeros((G, vec.harvest_words), dtype=torch.int64, device=dev)
    table = torch.zeros((G, N, g, g), dtype=torch.int64, device=dev)
    step_no = [0]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    def next_actions():
        vec.random_actions(acts, seed=0xBE7C, step=step_no[0])
        step_no[0] += 1

    def medians(variants, calls, before=lambda: None):
        reps = []
        for _ in range(args.reps):
            events = {k: [] for k in variants}
            for i in range(args.warmup + calls):
                for k, fn in variants.items():
                    before()
                    ev = timed(fn)
                    if i >= args.warmup:
                        events[k].append(ev)
            torch.cuda.synchronize()
            reps.append({k: statistics.median(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in events.items()})
        return reps, {k: statistics.median(r[k] for r in reps) for k in variants}

    out = dict(envs=E, groups=G, calls=args.calls, dense_calls=args.dense_calls, reps=args.reps, device=torch.cuda.get_device_name(0),
               placement=vec.placement, unit="us per call", sparse={}, dense={})
    # sparse: every call is a real next step of the staggered batch; the variants take turns
    groups = layouts["runs"]
    bench.stagger_phases(vec, torch, 0, gs)
    reps, med = medians({
        "step_observe": lambda: vec.step_observe(acts, auto_reset=True),
        "step_observe+harvest": lambda: (vec.step_observe(acts, auto_reset=True), vec.harvest(acc, groups)),
        "step_observe+harvest+visitation": lambda: (vec.step_observe(acts, auto_reset=True), vec.harvest(acc, groups),
                                                    vec.harvest_visitation(table, groups)),
    }, args.calls, next_actions)
    out["sparse"] = dict(medians_per_rep=reps, **med, visitation_added=med["step_observe+harvest+visitation"] - med["step_observe+harvest"],
                         visitation_added_per_rep=[r["step_observe+harvest+visitation"] - r["step_observe+harvest"] for r in reps],
                         episodes_harvested=int(acc[:, 0].sum()), cells_harvested=int(table.sum()))
    # dense: a lockstep batch at its last step; the state stays, every collection runs on it again and again
    vec.reset()
    for t in range(gs):
        vec.random_actions(acts, seed=0xD157, step=t)
        vec.step(acts, auto_reset=True)
    per_env = torch.empty((E, N, g, g), dtype=torch.uint32, device=dev)
    log_bytes = gs * E * N * 2
    out_bytes = per_env.numel() * 4
    for name, groups in layouts.items():
        reps, med = medians({
            "harvest_visitation": lambda: vec.harvest_visitation(table, groups),
            "export+index_add": lambda: table.index_add_(0, groups.long(), vec.visitation(out=per_env).view(torch.int32).long()),
            "export": lambda: vec.visitation(out=per_env),
        }, args.dense_calls)
        out["dense"][name] = dict(medians_per_rep=reps, **med, speedup=med["export+index_add"] / med["harvest_visitation"],
                                  log_bytes_read=log_bytes, harvest_log_gb_per_s=log_bytes / med["harvest_visitation"] / 1e3,
                                  export_bytes_written=out_bytes, export_gb_per_s=(log_bytes + out_bytes) / med["export"] / 1e3)
    assert vec.status() == 0
    text = json.dumps(out, indent=1, default=str)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

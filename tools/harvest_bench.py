"""What collecting episode results costs next to the step: ctf_harvest_episodes against today's route (counters() of ALL envs +
a torch masked reduction to the same table), at 65 536 8_arena envs, in ONE process on ONE observation buffer, the variants
interleaved call by call (the A/B form of tools/ab_inproc.py).

  sparse  phases staggered as bench.py staggers them (~131 envs end per step):
          (a) step_observe   (b) step_observe + harvest   (c) step_observe + counters() + torch reduction
  dense   a lockstep batch at its last step (all envs ended): harvest against (c)'s collection alone, on the same state

HIP-event time per call, medians over --calls calls after warm-up, --reps repetitions; one JSON document on stdout (and --out).

    python tools/harvest_bench.py --out profiles/r07_harvest_bench.json
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


def torch_route(vec, torch, groups, acc):
    """counters() + masked reduction into acc: what a caller does today after every step"""
    met, caps, steps = vec.counters()
    idx = ((vec.done != 0) & (steps == int(vec.cfg.game_steps))).nonzero().squeeze(1)
    c = caps[idx].long()
    rows = torch.cat([torch.ones_like(c[:, :1]), (c[:, :1] > c[:, 1:]).long(), (c[:, :1] == c[:, 1:]).long(), (c[:, :1] < c[:, 1:]).long(), c,
                      steps[idx].long()[:, None], torch.zeros_like(c[:, :1]), met[idx].reshape(idx.numel(), -1).long()], dim=1)
    acc.index_add_(0, groups[idx].long(), rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench

    pkg = importlib.import_module("marl-ctf-development_amd")
    kw = dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii)
    E = args.envs
    seeds = np.arange(E, dtype=np.uint64) + 1
    vec = pkg.VecGridworldCtf(E, device=0, py_seeds=seeds, np_seeds=seeds, **kw)
    dev, gs, N = vec.device, int(vec.cfg.game_steps), vec.N_AGENTS
    acts = torch.empty((E, N), dtype=torch.int8, device=dev)
    vec.observe()
    env = torch.arange(E, device=dev)
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

    out = dict(envs=E, calls=args.calls, reps=args.reps, device=torch.cuda.get_device_name(0), placement=vec.placement, sparse={}, dense={})
    for G in (1, 64):
        groups = (env // (E // G)).to(torch.int32)
        acc = torch.zeros((G, vec.harvest_words), dtype=torch.int64, device=dev)
        variants = {
            "step_observe": lambda: vec.step_observe(acts, auto_reset=True),
            "step_observe+harvest": lambda: (vec.step_observe(acts, auto_reset=True), vec.harvest(acc, groups)),
            "step_observe+torch": lambda: (vec.step_observe(acts, auto_reset=True), torch_route(vec, torch, groups, acc)),
        }
        # sparse: every call is a real next step of the staggered batch; the three variants take turns
        bench.stagger_phases(vec, torch, 0, gs)
        reps = []
        for _ in range(args.reps):
            events = {k: [] for k in variants}
            for i in range(args.warmup + args.calls):
                for k, fn in variants.items():
                    next_actions()
                    ev = timed(fn)
                    if i >= args.warmup:
                        events[k].append(ev)
            torch.cuda.synchronize()
            reps.append({k: statistics.median(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in events.items()})
        med = lambda k: statistics.median(r[k] for r in reps)
        a_, b_, c_ = med("step_observe"), med("step_observe+harvest"), med("step_observe+torch")
        out["sparse"][f"groups_{G}"] = dict(
            unit="us per call", medians_per_rep=reps, step_observe=a_, with_harvest=b_, with_torch_route=c_,
            harvest_added=b_ - a_, torch_added=c_ - a_, harvest_share_of_step=(b_ - a_) / a_, torch_share_of_step=(c_ - a_) / a_,
            harvest_added_per_rep=[r["step_observe+harvest"] - r["step_observe"] for r in reps],
            torch_added_per_rep=[r["step_observe+torch"] - r["step_observe"] for r in reps])
        # dense: a lockstep batch at its last step; the state stays, both collections run on it again and again
        vec.reset()
        for t in range(gs):
            vec.random_actions(acts, seed=0xD157, step=t)
            vec.step(acts, auto_reset=True)
        collect = {"harvest": lambda: vec.harvest(acc, groups), "torch": lambda: torch_route(vec, torch, groups, acc)}
        reps = []
        for _ in range(args.reps):
            events = {k: [] for k in collect}
            for i in range(args.warmup + args.calls):
                for k, fn in collect.items():
                    ev = timed(fn)
                    if i >= args.warmup:
                        events[k].append(ev)
            torch.cuda.synchronize()
            reps.append({k: statistics.median(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in events.items()})
        h_, t_ = statistics.median(r["harvest"] for r in reps), statistics.median(r["torch"] for r in reps)
        read = E * 13 * N * 4 + E * 64  # the counters + one 64-byte line of every env's record
        out["dense"][f"groups_{G}"] = dict(unit="us per call", medians_per_rep=reps, harvest=h_, torch_route=t_, speedup=t_ / h_, bytes_read=read,
                                          harvest_gb_per_s=read / h_ / 1e3, fraction_of_8_tb_per_s=read / h_ / 1e3 / 8000)
    assert vec.status() == 0
    text = json.dumps(out, indent=1, default=str)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

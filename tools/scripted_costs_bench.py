"""What the cost-to-go launch costs next to the action launch that runs the same searches: ctf_scripted_costs against
ctf_scripted_abilities (epsilon 0) with the same masks, roles and ability bits, at 65 536 8_arena envs after some hundred random
steps, warm, in ONE process, the two alternating call by call behind a k_step that moves the state on (the A/B form of
tools/scripted_bench.py).  Ability bits all ones (the arena has a vaulter and a miner per team, so the action launch is
k_scripted_abilities, not one of the launches it hands walkers to); all agents and one team; an all-runner pack and the mix in which
the guardians guard and the rest run.

HIP-event time per call, medians over --calls calls after warm-up, --reps repetitions.  One JSON document on stdout (and --out).

    python tools/scripted_costs_bench.py --out profiles/r20_scripted_costs_bench.json
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
    ap.add_argument("--play", type=int, default=300, help="random steps before the first timed call")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    pkg = importlib.import_module("marl-ctf-development_amd")
    kw = dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii)
    E = args.envs
    seeds = np.arange(E, dtype=np.uint64) + 1
    vec = pkg.VecGridworldCtf(E, device=0, py_seeds=seeds, np_seeds=seeds, tune_placement=False, **kw)
    dev, N = vec.device, vec.N_AGENTS
    acts = torch.empty((E, N), dtype=torch.int8, device=dev)
    bot_acts = torch.zeros((E, N), dtype=torch.int8, device=dev)
    costs = torch.zeros((E, N), dtype=torch.int16, device=dev)
    step_no = [0]

    def play():
        vec.random_actions(acts, seed=0xBE7C, step=step_no[0])
        step_no[0] += 1
        vec.step(acts, auto_reset=True)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    all_mask, team1 = (1 << N) - 1, vec.team_mask(1)
    packs = {"runner": ["runner"] * N, "guardians_guard": pkg.scripted.guardians_guard(vec.cfg)}
    variants = {}
    for name, roles in packs.items():
        for who, mask in (("all", all_mask), ("team", team1)):
            variants[f"abilities_{who}_{name}"] = lambda roles=roles, mask=mask: vec.scripted_abilities(roles, all_mask, agent_mask=mask, out=bot_acts)
            variants[f"costs_{who}_{name}"] = lambda roles=roles, mask=mask: vec.scripted_costs(roles, all_mask, agent_mask=mask, out=costs)
    for _ in range(args.play):
        play()
    reps = []
    for _ in range(args.reps):
        events = {k: [] for k in variants}
        for i in range(args.warmup + args.calls):
            play()  # every timed launch of this round sees the state it left
            for k, fn in variants.items():
                ev = timed(fn)
                if i >= args.warmup:
                    events[k].append(ev)
        torch.cuda.synchronize()
        reps.append({k: statistics.median(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in events.items()})
    med = {k: statistics.median(r[k] for r in reps) for k in variants}
    finite = costs[costs >= 0]
    out = dict(envs=E, play=args.play, calls=args.calls, reps=args.reps, device=torch.cuda.get_device_name(0), unit="us per call",
               medians_per_rep=reps, **med,
               ratio_costs_to_abilities={k[len("costs_"):]: med[k] / med["abilities_" + k[len("costs_"):]] for k in variants if k.startswith("costs_")},
               last_costs=dict(none=int((costs < 0).sum()), zero=int((costs == 0).sum()), mean_finite=float(finite.float().mean()), max=int(costs.max())))
    assert vec.status() == 0
    text = json.dumps(out, indent=1, default=str)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

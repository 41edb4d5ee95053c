"""What the action-effect launches cost next to a launch that reads the same state: ctf_action_effects (mask only, flags only, both)
and ctf_random_effective_actions against the unchanged ctf_scripted_costs with all eight agents as runners (with the ability bits all
ones, the row of profiles/r20_scripted_costs.md, and with none), at 65 536 8_arena envs after some hundred random auto-reset steps,
warm, in ONE process, the launches alternating call by call behind a k_step that moves the state on (the A/B form of
tools/scripted_costs_bench.py).

HIP-event time per call, medians over --calls calls after warm-up, --reps repetitions with their spread.  Bytes per call are computed
from the shapes: read, the grid and the record fields the rule looks at (hp, pos, has_flag, inventory) of every env; written, what the
call stores.  One JSON document on stdout (and --out); --note writes the profile note from it.

    python tools/action_effects_bench.py --out profiles/r21_action_effects.json --note profiles/r21_action_effects.md
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
HBM_PEAK = 8e12  # bytes per second


def note(r):
    rows = []
    for k in r["variants"]:
        lo, hi = min(x[k] for x in r["medians_per_rep"]), max(x[k] for x in r["medians_per_rep"])
        b = r["bytes"].get(k)
        traffic = f"{b['read']:,} | {b['written']:,} | {100 * (b['read'] + b['written']) / (r[k] * 1e-6) / HBM_PEAK:.1f} %" if b else "— | — | —"
        rows.append(f"| `{k}` | {r[k]:.1f} | {lo:.1f}–{hi:.1f} | {r[k] / r['costs_abilities']:.3f} | {r[k] / r['costs_walkers']:.3f} | {traffic} |")
    verdict = "below" if r["both"] < min(r["costs_abilities"], r["costs_walkers"]) else "NOT below"
    return "\n".join([
        "# Round 21 — `ctf_action_effects` and `ctf_random_effective_actions` against `ctf_scripted_costs`",
        "",
        f"`python tools/action_effects_bench.py` on one {r['device']}: {r['envs']:,} `8_arena` envs after {r['play']} random auto-reset steps, one",
        "process, warm; behind every further `k_step` the launches below run one after the other on the state it left.  HIP-event time per",
        f"call, median of {r['calls']} calls after warm-up, median of {r['reps']} repetitions (their range beside it).  `ctf_scripted_costs` is the",
        "parent's unchanged kernel, all eight agents asked, all runners: the yardstick, with the ability bits all ones (the first row of",
        "`profiles/r20_scripted_costs.md`) and with none (every agent a walker).",
        "",
        "| launch | µs | range over reps | / costs (abilities) | / costs (walkers) | bytes read | bytes written | share of 8 TB/s |",
        "|---|---:|---:|---:|---:|---:|---:|---:|",
        *rows,
        "",
        f"`ctf_action_effects` with both outputs is {verdict} both forms of the `ctf_scripted_costs` call.  It reads the same state, searches",
        "nothing and writes 11 bytes per agent.  The byte counts come from the shapes (grid and the record's hp, pos, has_flag and inventory",
        "of every env; the stores of the call), not from counters; the share of the 8 TB/s peak is that kernel's figure for those bytes:",
        "how far the launch is from a plain copy of them.",
        "",
        "Shape (`make asm-effects`): one lane per (env, agent), 256 lanes per block over whole envs; per lane two 2-byte loads, one 8-byte",
        "load and eleven byte loads, the eight target cells in flight together; 44–56 VGPRs, no scratch, no LDS, 8 waves per SIMD.  The mask is one",
        "`global_store_short`, the nine flag bytes one `global_store_dwordx2` and one `global_store_byte`: a wave's rows are one run of",
        "576 bytes.  The vaulter's compare is `v_add_f64` (hp, -cost) and `v_cmp_lt_f64`: no fused multiply-add.",
        "",
        f"The masks of the last timed call: {r['last']['effective_pairs']:,} of {r['last']['pairs']:,} (agent, action) pairs do something",
        f"({100 * r['last']['effective_pairs'] / r['last']['pairs']:.1f} %); {r['last']['stuck_agents']:,} agents have no effective action.",
        "",
        "## `bench.py` against the parent",
        "",
        r.get("bench_note", "not measured"),
        "",
    ])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--play", type=int, default=300, help="random steps before the first timed call")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--note", default=None, help="write the profile note (markdown) here")
    ap.add_argument("--bench-note", default=None, help="a text file whose content becomes the note's bench.py section")
    args = ap.parse_args()
    import torch

    pkg = importlib.import_module("marl-ctf-development_amd")
    kw = dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii)
    E = args.envs
    seeds = np.arange(E, dtype=np.uint64) + 1
    vec = pkg.VecGridworldCtf(E, device=0, py_seeds=seeds, np_seeds=seeds, tune_placement=False, **kw)
    dev, N, G = vec.device, vec.N_AGENTS, vec.GRID_SIZE
    acts = torch.empty((E, N), dtype=torch.int8, device=dev)
    drawn = torch.zeros((E, N), dtype=torch.int8, device=dev)
    costs = torch.zeros((E, N), dtype=torch.int16, device=dev)
    mask = torch.zeros((E, N), dtype=torch.int16, device=dev)
    flags = torch.zeros((E, N, 9), dtype=torch.uint8, device=dev)
    abi = importlib.import_module("marl-ctf-development_amd._abi")
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

    full = (1 << N) - 1
    variants = {
        "costs_abilities": lambda: vec.scripted_costs(None, True, agent_mask=full, out=costs),
        "mask": lambda: vec.effective_actions(out=mask),
        "costs_walkers": lambda: vec.scripted_costs(None, False, agent_mask=full, out=costs),
        "flags": lambda: vec.action_effects(out=flags),
        "both": lambda: vec._call("ctf_action_effects", abi.ptr(mask), abi.ptr(flags), full, vec._stream()),
        "sampler": lambda: vec.random_effective_actions(drawn, 0x5EED, step_no[0]),
    }
    state = E * (G * G + N * (8 + 2 + 1 + 2))  # the grid; hp, pos, has_flag, inventory
    nbytes = {"mask": dict(read=state, written=E * N * 2), "flags": dict(read=state, written=E * N * 9), "both": dict(read=state, written=E * N * 11),
              "sampler": dict(read=state, written=E * N)}
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
    table = pkg.effects_table(mask)
    out = dict(envs=E, play=args.play, calls=args.calls, reps=args.reps, device=torch.cuda.get_device_name(0), unit="us per call", variants=list(variants),
               medians_per_rep=reps, **med, bytes=nbytes,
               ratio_to_costs_abilities={k: med[k] / med["costs_abilities"] for k in nbytes}, ratio_to_costs_walkers={k: med[k] / med["costs_walkers"] for k in nbytes},
               share_of_hbm_peak={k: (b["read"] + b["written"]) / (med[k] * 1e-6) / HBM_PEAK for k, b in nbytes.items()},
               last=dict(pairs=E * N * 9, effective_pairs=int(table.sum()), stuck_agents=int((mask == 0).sum())))
    assert vec.status() == 0
    assert bool(((flags != 0) == table).all())  # the two outputs of the last calls agree
    if args.bench_note and os.path.exists(args.bench_note):
        out["bench_note"] = open(args.bench_note).read().strip()
    text = json.dumps(out, indent=1, default=str)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.note:
        with open(args.note, "w") as f:
            f.write(note(out))


if __name__ == "__main__":
    main()

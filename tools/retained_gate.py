"""Gate of the retained observation render: is step + delta render clearly faster than step + full render, in ONE process on ONE
placement-tuned buffer, at the bench's state (65 536 arena envs, episode phases staggered as bench.py does), the variants
interleaved round by round as tools/ab_inproc.py does?

Variants, all on the same handle and the same buffer (switched with ctf_obs_retain, so nothing else differs):
  full        the buffer released: k_observe_tiles rewrites all of it (what every render was before retention)
  delta       the buffer retained, the round-11 kernel (k_observe_delta_bitmap, CTF_OBS_DELTA_BITMAP=1) with plain stores
  delta-nt    the same with the nontemporal hint on its stores (CTF_OBS_DELTA_NT=1, read when the buffer is retained)
  rebuild     the buffer retained, k_observe_delta as round 12 had it: the slot images rebuilt from the grid at every render
              (CTF_OBS_DELTA_REBUILD=1), plain stores
  rebuild-nt  the same with the nontemporal hint
  direct      the buffer retained, k_observe_delta with the slot images kept in the shadow and carried forward, plain stores
  direct-nt   the same with the nontemporal hint
  step-meta   direct-nt with the metadata rows written by k_step (CTF_STEP_META=1, the default; read at every ctf_step_observe)
  render-meta direct-nt with the rows made by the render, as before round 15 (CTF_STEP_META=0)
(every other variant runs with CTF_STEP_META unset.  The switch only changes ctf_step_observe, so it shows in the window of
step_observe calls and not in the two kernels timed apart, which are ctf_step and ctf_observe.)
Per round and variant: k_step and the render timed apart with events (the step of a variant runs behind that variant's render,
so what the render leaves in the caches shows in it), then 100 back-to-back step_observe calls timed as one window.

Usage: python tools/retained_gate.py [envs] [arena|arena20|split] [rounds] [variant,variant,...]      (prints a markdown table)"""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pkg = importlib.import_module("marl-ctf-development_amd")
_abi = importlib.import_module("marl-ctf-development_amd._abi")

E = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
WORKLOAD = sys.argv[2] if len(sys.argv) > 2 else "arena"
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 4
kw = {"arena": lambda: dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii),
      "arena20": lambda: dict(pkg.configs.ARENA20_KWARGS, SCENARIO=pkg.configs.arena20_scenario()),
      "split": lambda: dict(pkg.configs.SPLIT_KWARGS, SCENARIO=pkg.CtfScenarios.arrow)}[WORKLOAD]()
seeds = np.arange(E, dtype=np.uint64) + 1_000_003
vec = pkg.VecGridworldCtf(E, device=0, py_seeds=seeds, np_seeds=seeds, log_metrics=True, **kw)
buf = vec.obs  # the placement search runs here (full renders), then the buffer is retained
dev = vec.device
print(f"{WORKLOAD}, {E} envs; placement {vec.placement}", flush=True)

acts = torch.empty((8, E, vec.N_AGENTS), dtype=torch.int8, device=dev)
period = kw["GAME_STEPS"]
phase = torch.arange(E, device=dev) % period
for s in range(period):  # bench.stagger_phases: env e ends its episodes at steps congruent to e mod GAME_STEPS
    vec.random_actions(acts[0], seed=0x5747, step=s)
    vec.step(acts[0], auto_reset=True)
    vec.reset((phase == s).to(torch.uint8))
for k in range(8):
    vec.random_actions(acts[k], seed=0xC7F, step=k)
torch.cuda.synchronize(dev)


def select(variant):
    if variant == "full":
        vec._call("ctf_obs_retain", None, vec._stream())
    else:
        os.environ.pop("CTF_STEP_META", None)
        if variant in ("step-meta", "render-meta"):
            os.environ["CTF_STEP_META"] = "1" if variant == "step-meta" else "0"
        os.environ["CTF_OBS_DELTA_NT"] = "1" if variant.endswith("-nt") or variant.endswith("-meta") else "0"
        os.environ["CTF_OBS_DELTA_BITMAP"] = "1" if variant.startswith("delta") else "0"
        os.environ["CTF_OBS_DELTA_REBUILD"] = "1" if variant.startswith("rebuild") else "0"
        vec._call("ctf_obs_retain", _abi.ptr(buf), vec._stream())
    assert vec.observe_retained() == (variant != "full")
    vec.observe()  # (after retaining: the one full pass that fills the shadow)


def window(reps=100):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps + 1)]
    ev[0].record()
    for k in range(reps):
        vec.step(acts[k % 8], auto_reset=True)
        ev[2 * k + 1].record()
        vec.observe()
        ev[2 * k + 2].record()
    torch.cuda.synchronize(dev)
    st = float(np.mean([ev[2 * k].elapsed_time(ev[2 * k + 1]) for k in range(reps)]))
    ob = float(np.mean([ev[2 * k + 1].elapsed_time(ev[2 * k + 2]) for k in range(reps)]))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(reps):
        vec.step_observe(acts[k % 8], auto_reset=True)
    b.record()
    torch.cuda.synchronize(dev)
    return st, ob, a.elapsed_time(b) / reps


VARIANTS = ("full", "delta", "delta-nt", "rebuild", "rebuild-nt", "direct", "direct-nt")
if len(sys.argv) > 4:
    assert set(sys.argv[4].split(",")) <= set(VARIANTS + ("step-meta", "render-meta")), sys.argv[4]
    VARIANTS = tuple(sys.argv[4].split(","))
for v in VARIANTS:
    select(v)
    window(30)
rows = {v: [] for v in VARIANTS}
print("\n| round | variant | k_step ms | render ms | step_observe ms | M env-steps/s |\n|---|---|---|---|---|---|")
for rnd in range(ROUNDS):
    for v in VARIANTS:
        select(v)
        window(10)
        st, ob, whole = window()
        rows[v].append((st, ob, whole))
        print(f"| {rnd} | {v} | {st:.4f} | {ob:.4f} | {whole:.4f} | {E / whole / 1e3:.1f} |", flush=True)
print("\n| variant | step_observe ms: mean | min | max | spread between rounds |\n|---|---|---|---|---|")
for v in VARIANTS:
    w = [r[2] for r in rows[v]]
    print(f"| {v} | {np.mean(w):.4f} | {min(w):.4f} | {max(w):.4f} | {(max(w) - min(w)) / np.mean(w) * 100:.1f} % |")

"""Bandwidth of the batched snapshot calls (ctf_save_states / ctf_load_states) at bench size: the full-batch save and load and a
random 10 % subset of each, every one against a torch copy of the same number of bytes (read + write counted, as for the
snapshot calls).  Device events around --reps calls after warm-up; the median of --windows windows.  Prints one JSON line
(bytes moved, ms, GB/s, fraction of the 8 TB/s peak).  Usage (GPU box):
    python tools/snapshot_bench.py [--envs 65536] [--reps 20] [--windows 5] [--out profiles/<name>.json]
"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
pkg = importlib.import_module("marl-ctf-development_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
PEAK = 8.0e12
E = args.envs
kw = dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii)
vec = pkg.VecGridworldCtf(E, device=0, py_seeds=np.arange(E), np_seeds=np.arange(E), tune_placement=False, **kw)
acts = torch.empty((E, vec.N_AGENTS), dtype=torch.int8, device="cuda")
for t in range(40):  # a state with moved generators and a filled visitation log
    vec.random_actions(acts, seed=0xC7F, step=t)
    vec.step(acts, auto_reset=True)
S = vec.snapshot_bytes
g = torch.Generator().manual_seed(1)
sub = torch.randperm(E, generator=g)[: E // 10].sort().values.to(torch.int32).cuda()
full = vec.save_states()
part = vec.save_states(sub)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / args.reps)
    return float(np.median(ms))


def row(name, fn, n):
    moved = 2 * n * S  # the record bytes are read once and written once
    ms = timed(fn)
    return name, dict(records=n, bytes_moved=moved, ms=round(ms, 4), GBps=round(moved / ms / 1e6, 1), of_peak=round(moved / ms * 1e3 / PEAK, 3))


src_full, dst_full = torch.empty_like(full), torch.empty_like(full)
src_part, dst_part = torch.empty_like(part), torch.empty_like(part)
rows = dict([
    row("save_full", lambda: vec.save_states(out=full), E),
    row("load_full", lambda: vec.load_states(full, check=False), E),
    row("save_subset10", lambda: vec.save_states(sub, out=part), sub.numel()),
    row("load_subset10", lambda: vec.load_states(part, sub, check=False), sub.numel()),
    row("torch_copy_full", lambda: dst_full.copy_(src_full), E),
    row("torch_copy_subset10", lambda: dst_part.copy_(src_part), sub.numel()),
])
assert vec.status() == 0
for k in ("save", "load"):
    rows[f"{k}_full"]["vs_copy"] = round(rows["torch_copy_full"]["ms"] / rows[f"{k}_full"]["ms"], 3)
    rows[f"{k}_subset10"]["vs_copy"] = round(rows["torch_copy_subset10"]["ms"] / rows[f"{k}_subset10"]["ms"], 3)
res = dict(envs=E, snapshot_bytes=S, device=torch.cuda.get_device_name(0), reps=args.reps, windows=args.windows, **rows)
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

"""The three RNG modes side by side IN ONE PROCESS (separate processes cannot be compared: the placement of a large allocation
alone moves the render by 20 %): one handle each of "mt19937", "counter" and "counter_direct" on bench.py's state (a discarded
first episode, staggered episode phases, fresh actions every step), interleaved and warm.  Per workload and mode:
  k_step alone, back to back     mean and p10 / p50 / p90 over all timed launches (>= 200)
  step + render (ctf_step_observe into one shared buffer)   the same
Usage (GPU box):  python tools/counter_direct_ab.py [arena_65536 split_4096 arena_32768]
AB_JSON=<path> also writes the figures as JSON."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
pkg = importlib.import_module("marl-ctf-development_amd")
MODES = ("mt19937", "counter", "counter_direct")
WORKLOADS = {"arena": lambda: dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii),
             "split": lambda: dict(pkg.configs.SPLIT_KWARGS, SCENARIO=pkg.CtfScenarios.arrow)}
ROUNDS, PER_ROUND = int(os.environ.get("AB_ROUNDS", 5)), int(os.environ.get("AB_LAUNCHES", 60))  # round 0 is the warm-up


def stagger(vec, acts, period):
    phase = torch.arange(vec.n_envs, device=vec.device) % period
    for s in range(period):
        vec.random_actions(acts, seed=0x5747, step=s)
        vec.step(acts, auto_reset=True)
        vec.reset((phase == s).to(torch.uint8))


def quantiles(ms):
    ms = np.asarray(ms)
    return dict(n=int(ms.size), mean=float(ms.mean()), p10=float(np.percentile(ms, 10)), p50=float(np.percentile(ms, 50)), p90=float(np.percentile(ms, 90)))


def run(spec):
    name, _, envs = spec.partition("_")
    E, kw = int(envs), WORKLOADS[name]()
    seeds = np.arange(E, dtype=np.uint64) + 1
    vecs = {m: pkg.VecGridworldCtf(E, device=0, py_seeds=seeds, np_seeds=seeds, rng_mode=m, tune_placement=False, **kw) for m in MODES}
    first = vecs[MODES[0]]
    N = first.N_AGENTS
    acts = torch.empty((E, N), dtype=torch.int8, device=first.device)
    for v in vecs.values():
        stagger(v, acts, kw["GAME_STEPS"])
    ACTS = torch.empty((64, E, N), dtype=torch.int8, device=first.device)
    for t in range(64):
        first.random_actions(ACTS[t], seed=0xC7F, step=t)
    shared_obs, shared_meta = first.obs, first.meta
    step_ms, both_ms = {m: [] for m in MODES}, {m: [] for m in MODES}
    for rnd in range(ROUNDS):
        for m, v in vecs.items():
            v.obs, v.meta = shared_obs, shared_meta  # a caller's buffer: rendered in full every time, the same for every mode
            for t in range(8):
                v.step_observe(ACTS[t], auto_reset=True)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(PER_ROUND)]
            for t, (a, b) in enumerate(ev):
                a.record(); v.step(ACTS[t % 64], auto_reset=True); b.record()
            ev2 = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(PER_ROUND)]
            for t, (a, b) in enumerate(ev2):
                a.record(); v.step_observe(ACTS[(t + 7) % 64], auto_reset=True); b.record()
            torch.cuda.synchronize()
            if rnd:
                step_ms[m] += [a.elapsed_time(b) for a, b in ev]
                both_ms[m] += [a.elapsed_time(b) for a, b in ev2]
    out = {}
    for m, v in vecs.items():
        assert v.status() == 0, (spec, m)
        s, b = quantiles(step_ms[m]), quantiles(both_ms[m])
        out[m] = dict(k_step=s, step_render=b, env_steps_per_s=E / (b["mean"] * 1e-3))
        print(f"[{spec} {m:14s}] k_step mean {s['mean']:.4f} p10 {s['p10']:.4f} p50 {s['p50']:.4f} p90 {s['p90']:.4f} ms (p90/p50 {s['p90'] / s['p50']:.3f}, n {s['n']})"
              f"  step+render mean {b['mean']:.4f} p10 {b['p10']:.4f} p50 {b['p50']:.4f} p90 {b['p90']:.4f} ms  {out[m]['env_steps_per_s'] / 1e6:.1f} M env-steps/s",
              flush=True)
        v.close()
    return out


if __name__ == "__main__":
    specs = sys.argv[1:] or ["arena_65536", "split_4096", "arena_32768"]
    results = {}
    for spec in specs:
        results[spec] = run(spec)
        torch.cuda.empty_cache()
    if os.environ.get("AB_JSON"):
        with open(os.environ["AB_JSON"], "w") as f:
            json.dump(results, f, indent=1)

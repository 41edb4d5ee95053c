#!/usr/bin/env python3
"""bench.py — env-steps/sec of the batched GridworldCtf hot path on MI355X.

    python bench.py --gpus 1 --steps 200 --warmup 20
    python bench.py --gpus 1 --steps 200 --warmup 20 --full     # + per-kernel figures, roofline, secondaries, CPU baseline
    python bench.py --gpus 1 --steps 200 --dump-outputs DIR     # + the last timed step's outputs as DIR/<name>.npy
    python bench.py --gpus N --steps K --warmup W          # starts the N ranks itself (see launch_ranks below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W              # the driver's form: WORLD_SIZE must equal --gpus

The N-worker launch this replaces is the reference's one Ray task per env (ppo.py:264-266, :349-376: ray_rollout.remote(env, agent,
opponent) x num_envs, ray.get): here one process per GPU, each owning a contiguous range of global env indices.

A plain run (no --full) does only what the headline needs: set up, warm up (W steps), time ONE window of exactly K steps, write
the outputs if --dump-outputs is given, print the line.  --full adds everything else this file measures, as described below:
the headline over `--windows` (5) windows, the per-kernel durations and roofline, the compact-observation rate, the `secondary`
blocks and the `cpu_baseline`.

--dump-outputs DIR writes what the last timed step computed, as float32 .npy files: `rewards` [E, N] and `done` [E] of every env
of rank 0's shard (sampled like the observations when they would exceed 16 MiB), and `obs` [S, N, C, G, G] / `meta` [S, N, 2N+6]
of a fixed sample of S = min(E, 256) envs (np.random.default_rng(DUMP_SEED).choice(E, S, replace=False), sorted).  Same arguments,
same inputs: seeds and action streams are functions of --run and the global env index, so two builds compare output for output.

One "step" = one pass of the hot path over one batch: GridworldCtf.step() for every env of the shard
plus the N observations + metadata rows a rollout consumes (reference ppo.py:59-98), with auto-reset at
episode end — the two launches of ctf_step_observe (k_step, whose tail blocks regenerate the MT19937 blocks the
envs have used up, then the render).  The timed region holds nothing else: `--windows` back-to-back windows (1 in a plain run, 5
with --full) of exactly K such steps, each bracketed by barrier + synchronize, MAX over ranks per window; `ms_per_step` / `value`
are those of the MEDIAN window (`windows_ms` lists them all).  With --full the per-kernel durations come from SAMPLE_STEPS (12) further
steps AFTER the windows, issued as ctf_step + ctf_observe with a HIP event around each launch, net of the cost of an
empty event pair measured in the same run (`event_pair_overhead_ms`).  Workload at N=1: BASELINE.json configs[2] — 8_arena
(arena_iii, 4v4, the reference's 15x15 map), 65 536 envs resident in HBM; N>1 keeps 65 536 envs per GPU
(weak scaling) in the headline and, with --full, adds, as `secondary.configs3_262144`, BASELINE.json configs[3] at its own size
(262 144 envs GLOBAL = 262 144 / N per GPU: the strong-scaling reading of the same path); the N=1 --full line carries that
configuration's per-GPU shard of an 8-GPU job as `secondary.arena_32768`.  Envs are sharded by global index with no data-path collective (--rollout-exchange adds an
asynchronous RCCL all-gather of the compact rollout tensors once per 16-step chunk, what a centralised
learner would need).  Inputs (Philox action streams for every timed step) are generated on the device
before the timed region.

Protocol: before the timed region every env plays a first, discarded episode and the envs
are put at STAGGERED episode phases (env e has env_step_count = 499 - e % 500), so that any timed window
holds the steady-state mix: ~E/500 envs reach GAME_STEPS and are reset inside the launch at every step,
agents are spread over the map, tags / respawns / flag events occur at their steady-state rates.  (The
511-step visitation-log fold cannot occur under this protocol: an episode ends at 500 steps.)

With --full, at N=1 the line also carries, as `secondary`, the other single-GPU BASELINE configurations run the same
way — the synthetic 20x20 arena at 65 536 envs (BASELINE.json's wording) and 0_the_split at 4 096 envs
(configs[1]) — each with its own roofline.

Rank 0 prints ONE JSON line (see DESIGN.md §Measurement for the roofline / cpu_baseline fields).
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def observe_algorithmic_bytes(n, c, g):
    """Bytes one env MUST move in the observe launch: obs u8 [N][C][G][G] + metadata f16 [N][2N+6] written,
    grid G*G + agent state (hp 8, pos 2, flag 1 per agent) + step/captures/done (13) read."""
    return n * c * g * g + n * (2 * n + 6) * 2 + g * g + 11 * n + 13


def step_algorithmic_bytes(n, g):
    """SURVEY §8d terms of the step launch: grid r+w, agent state r+w (14 B/agent), actions in, f32 rewards +
    done out, RNG words r+w (~N^2 + 2(N-1) words)."""
    return 2 * g * g + 2 * 14 * n + (n + 4 * n + 1) + 8 * (n * n + 2 * n - 2)


def env_step_algorithmic_bytes(n, c, g):
    """SURVEY §8d's per-env-step total (26 891 B on 8_arena, 4 535 B on 0_the_split): grid and agent state counted once
    (the render's re-read of them is overhead, not algorithm)."""
    return n * c * g * g + n * (2 * n + 6) * 2 + step_algorithmic_bytes(n, g)



# ---- starting the ranks (stdlib only: the launching parent must never initialise HIP, so nothing here imports torch) ---------------

def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def visible_gpus():
    """How many HIP devices this box shows — asked of a CHILD process, so that the parent stays free of any HIP state (a process that
    has touched the GPU must not start the ranks on this pool).  CTF_BENCH_DRYRUN ranks run on the CPU and need none;
    CTF_BENCH_ONE_DEVICE=1 puts every rank on device 0 (a rehearsal of the N-rank path on a one-GPU box, over gloo: RCCL refuses two
    ranks on one device)."""
    import subprocess

    if os.environ.get("CTF_BENCH_DRYRUN") or os.environ.get("CTF_BENCH_ONE_DEVICE"):
        return None
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], stdout=subprocess.PIPE, text=True, timeout=600)
    try:
        return int(r.stdout.strip().splitlines()[-1])
    except (ValueError, IndexError):
        return 0


def single_rank_rendezvous():
    """CTF_FORCE_DIST=1 without a launcher: the env:// rendezvous of a one-rank group (rehearsal of the N > 1 code path on one GPU)."""
    if "RANK" not in os.environ:
        os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))


def world_or_launch(gpus, script, argv):
    """The launch rule of `--gpus N`, shared by bench.py and bench_rollout.py.

    * WORLD_SIZE set (a rank under torchrun, however it was started): it must equal --gpus, else exit non-zero — a line labelled
      n_gpus = WORLD_SIZE while the caller asked for N is a mislabelled record;
    * WORLD_SIZE unset, N == 1: this process is the only rank -> returns None and the caller goes on;
    * WORLD_SIZE unset, N > 1: this process becomes the LAUNCHER: it checks that N devices are visible, starts
      `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> script argv` as a
      CHILD process (never an exec of itself), relays the ranks' stdout (rank 0's one JSON line) and stderr, and returns the worst
      child's exit code (torchrun's own: non-zero as soon as any rank failed)."""
    import subprocess

    if gpus < 1:
        raise SystemExit(f"--gpus {gpus}: need at least one")
    ws = os.environ.get("WORLD_SIZE")
    if ws is not None:
        if int(ws) != gpus:
            raise SystemExit(f"--gpus {gpus} but WORLD_SIZE={ws}: start this job with --nproc-per-node {gpus}, or pass --gpus {ws}")
        return None
    if gpus == 1:
        return None
    have = visible_gpus()
    if have is not None and have < gpus:
        raise SystemExit(f"--gpus {gpus}: only {have} HIP device(s) visible on this box")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), script] + list(argv)
    print(f"[{os.path.basename(script)}] starting {gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


WORKLOADS = {
    "arena": ("8_arena (arena_iii 15x15, 4v4 heterogeneous)", lambda pkg: dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii)),
    "arena20": ("8_arena agents and rules on a synthetic 20x20 map (4v4 heterogeneous)",
                lambda pkg: dict(pkg.configs.ARENA20_KWARGS, SCENARIO=pkg.configs.arena20_scenario())),
    "split": ("0_the_split (arrow 11x11, 2v2)", lambda pkg: dict(pkg.configs.SPLIT_KWARGS, SCENARIO=pkg.CtfScenarios.arrow)),
}


def _cpu_quota():
    """CPUs the container's cgroup lets this process use at once (cgroup v2 cpu.max or v1 cfs quota / period), None if unlimited or
    unreadable.  A 1-GPU box shows all 256 logical CPUs in the affinity mask and throttles the process to its own share of them."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else max(1, int(int(q) / int(per)))
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else max(1, q // per)
    except (OSError, ValueError):
        return None


def _host_cpu():
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"model": model, "logical_cpus": os.cpu_count(), "affinity": len(os.sched_getaffinity(0)), "cgroup_cpu_quota": _cpu_quota()}


def cpu_baseline(pkg, kwargs, budget_s=12.0):
    """The CPU oracle (kind "port": the C restatement pinned to the reference by tests/golden) timed on this
    box's host cores on a bounded sample of the same workload: batches of arena envs x 200 steps of
    step()+observe() with the same Philox action streams, OpenMP over envs, until ~budget_s has elapsed."""
    import oracle  # test infrastructure: used here only as the reported CPU baseline

    cfg, _ = pkg.config.build_config(kwargs, log_metrics=True)
    # a 1-GPU box's CPU share is 16 cores; never more threads than the affinity mask allows
    cores = int(os.environ.get("CTF_BENCH_CPU_THREADS", min(len(os.sched_getaffinity(0)), 16)))
    steps = 200
    t0 = time.perf_counter()
    oracle.run_batch(cfg, 16, steps, 1_000_003, 7, True, 1)
    one = 16 * steps / (time.perf_counter() - t0)  # single-thread rate from a pilot
    batch, done_envs = cores * 16, 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < budget_s:
        oracle.run_batch(cfg, batch, steps, 1_000_003 + done_envs, 7, True, cores)
        done_envs += batch
    dt = time.perf_counter() - t0
    # the same on ALL host cores this process may use: the affinity mask, capped by the cgroup's CPU quota (round 5's
    # first box: 256 CPUs in the mask, 256 threads = 1.4 M env-steps/s against 3.2 M with 16 — the box throttles to its 16-core share)
    all_cores = min(len(os.sched_getaffinity(0)), _cpu_quota() or 1 << 30)
    all_cores_value = all_cores_sample = None
    if all_cores > cores and not os.environ.get("CTF_BENCH_CPU_THREADS"):
        b2, d2 = all_cores * 16, 0
        t1 = time.perf_counter()
        while time.perf_counter() - t1 < budget_s / 2:
            oracle.run_batch(cfg, b2, steps, 2_000_003 + d2, 7, True, all_cores)
            d2 += b2
        dt2 = time.perf_counter() - t1
        all_cores_value, all_cores_sample = d2 * steps / dt2, f"{d2} envs x {steps} steps ({dt2:.1f} s)"
    elif all_cores == cores:
        all_cores_value, all_cores_sample = done_envs * steps / dt, "the same run: `cores` is all this process may use (min of affinity mask and cgroup CPU quota)"
    out = {
        "value": done_envs * steps / dt,
        "unit": "env-steps/s",
        "cores": cores,
        "kind": "port",
        "sample": f"{done_envs} envs x {steps} steps, 8_arena step()+observe(), C oracle, OpenMP over envs ({dt:.1f} s)",
        "single_core_value": one,
        "all_cores_value": all_cores_value,
        "all_cores": all_cores,
        "all_cores_sample": all_cores_sample,
        "host_cpu": _host_cpu(),
    }
    try:  # the per-env Python/NumPy restatement on one core: calibrates this box against BASELINE.md's 1.2 k env-steps/s
        from oracle import ctf_numpy

        out["python_numpy_1core"] = ctf_numpy.timed_sample(kwargs, budget_s=6.0)
    except ImportError:
        pass
    return out


def facade_1env(pkg, kwargs, device, budget_s=4.0):
    """The boundary's DROP-IN mode, measured: the reference's own class API (marl-ctf-development_amd.GridworldCtf, a batch of one
    env behind it) driven exactly as ppo.py:59-98 drives the reference's — per env step N x (standardise_state + get_env_metadata) then
    step(actions), the process-global `random` / `np.random` contract ON (both generators' states go to the device and come back at
    every step) — in env-steps/s, to read beside cpu_baseline.python_numpy_1core and BASELINE.md's 1.2 k for the reference itself."""
    import random

    import numpy as np

    random.seed(42)
    np.random.seed(42)
    env = pkg.GridworldCtf(device=device, **kwargs)
    n = env.N_AGENTS
    rng = np.random.default_rng(1234)  # an independent action stream: the env's own generators are not perturbed

    def episode_steps(count):
        for _ in range(count):
            for i in range(n):
                env.standardise_state(i, reverse_grid=env.AGENT_TEAMS[i] == 1)
                env.get_env_metadata(i)
            _, _, done = env.step([int(a) for a in rng.integers(0, 9, n)])
            if done:
                env.reset()

    episode_steps(20)  # warm-up
    steps, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < budget_s:
        episode_steps(50)
        steps += 50
    dt = time.perf_counter() - t0
    return {"value": steps / dt, "unit": "env-steps/s", "steps": steps, "us_per_env_step": dt / steps * 1e6,
            "workload": f"GridworldCtf (reference API, 1 env) on 8_arena: per step {n} x (standardise_state + get_env_metadata) + step(), "
                        "global-RNG contract on, reset at done — the call pattern of ppo.py:59-98",
            "reference_python_same_pattern": "1.2 k env-steps/s (BASELINE.md, build container, 1 core); cpu_baseline.python_numpy_1core is "
                                             "the per-env NumPy restatement on THIS box"}


def selfplay_at_reference_length(torch, device, wall_so_far_s, need_gb=90.0, wall_limit_s=120.0):
    """BASELINE configs[4] on one GPU at the reference's rollout length (num_steps = 500, 8_arena.py:73-74, ppo.py:288): one PPO
    iteration of 65 536 envs x 500 steps (44 GB of compact rollout, ~78 GB peak).  Guarded: it runs only with >= need_gb GB of free
    device memory and while the bench has used < wall_limit_s of wall time; otherwise a `skipped` record says why."""
    torch.cuda.empty_cache()
    free_gb = torch.cuda.mem_get_info(device)[0] / 1e9
    if free_gb < need_gb:
        return {"skipped": f"free device memory {free_gb:.1f} GB < {need_gb:.0f} GB"}
    if wall_so_far_s > wall_limit_s:
        return {"skipped": f"bench wall time so far {wall_so_far_s:.0f} s > {wall_limit_s:.0f} s"}
    try:
        import bench_rollout

        t0 = time.perf_counter()
        res = bench_rollout.run(envs=65536, steps=500, device=device, order="device")
        res["wall_s"] = time.perf_counter() - t0
        return res
    except Exception as exc:  # a secondary must never cost the headline line
        return {"error": repr(exc)}
    finally:
        torch.cuda.empty_cache()


def stagger_phases(vec, torch, lo, period=500):
    """A first (discarded) episode for every env, leaving env e at env_step_count = period - 1 - e % period."""
    E, N = vec.n_envs, vec.N_AGENTS
    acts = torch.empty((E, N), dtype=torch.int8, device=vec.device)
    phase = torch.arange(E, device=vec.device) % period
    for s in range(period):
        vec.random_actions(acts, seed=0x5747, step=s, env_offset=lo)
        vec.step(acts, auto_reset=True)
        vec.reset((phase == s).to(torch.uint8))
    torch.cuda.synchronize()


def two_shards_two_streams(pkg, torch, name, E, K, W, local_rank, run, windows=5, shards=2):
    """The same E envs as `shards` handles of E / shards envs each (global env indices and seeds as in the headline), every handle's
    own ctf_step_observe chain on its own HIP stream and NO synchronisation between the shards inside a window: one shard's k_step
    runs beside the other's render.  What a caller gets that double-buffers its envs (each shard's policy step between that shard's
    env steps) — not the headline's protocol, where one call steps all envs and the next call starts after it.  -> secondary block."""
    sh = pkg.sharding
    label, make_kwargs = WORKLOADS[name]
    kwargs = make_kwargs(pkg)
    device = torch.device("cuda", local_rank)
    per = E // shards
    vecs, acts, streams = [], [], []
    for s in range(shards):
        lo = s * per
        seeds = sh.env_seeds(run, lo, lo + per)
        v = pkg.VecGridworldCtf(per, device=local_rank, py_seeds=seeds, np_seeds=seeds, **kwargs)
        v.observe()
        stagger_phases(v, torch, lo, kwargs["GAME_STEPS"])
        vecs.append(v)
        acts.append(torch.empty((max(W, K), per, v.N_AGENTS), dtype=torch.int8, device=device))
        streams.append(torch.cuda.Stream(device=device))

    def fill(first, count):
        for s, v in enumerate(vecs):
            for i in range(count):
                v.random_actions(acts[s][i], seed=0xC7F, step=first + i, env_offset=s * per)

    def steps(count):
        for i in range(count):
            for v, a, st in zip(vecs, acts, streams):
                with torch.cuda.stream(st):
                    v.step_observe(a[i], auto_reset=True)

    fill(0, W)
    torch.cuda.synchronize()
    steps(W)
    t, win = W, []
    for _ in range(max(1, windows)):
        fill(t, K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(K)
        torch.cuda.synchronize()
        win.append(time.perf_counter() - t0)
        t += K
    status = 0
    for v in vecs:
        status |= v.status()
    med = sorted(win)[len(win) // 2]
    out = {"value": E * K / med, "unit": "env-steps/s", "steps": K, "windows": len(win), "ms_per_step": med / K * 1e3,
           "windows_ms_per_step": [w / K * 1e3 for w in win], "shards": shards, "envs_per_shard": per,
           "placement": [v.placement for v in vecs], "device_status_bits": status,
           "protocol": f"{shards} handles x {per} envs on {shards} HIP streams, each stream its own K ctf_step_observe calls, no "
                       "synchronisation between the shards inside a window (host wall clock around a window, synchronize on both sides)"}
    for v in vecs:
        v.close()
    return out


SAMPLE_STEPS = 12  # steps run AFTER the timed windows with an event around each launch (the per-kernel durations)
DUMP_SEED, DUMP_ENVS = 0xD0, 256  # --dump-outputs: the fixed sample of envs whose observations are written
DUMP_FULL_LIMIT = 16 << 20  # rewards + done of every env while they fit in this many bytes (float32), else the sample's


def snapshot_outputs(torch, vec):
    """What the caller of the timed path holds after its last step (ctf_step_observe's rewards, done, obs, meta), as float32 host
    arrays: rewards / done of every env, obs / meta of a fixed, seeded sample of envs (see the module docstring)."""
    import numpy as np

    E, N = vec.n_envs, vec.N_AGENTS
    pick = np.sort(np.random.default_rng(DUMP_SEED).choice(E, min(E, DUMP_ENVS), replace=False))
    idx = torch.from_numpy(pick).to(vec.device)
    host = lambda t: t.float().cpu().numpy()
    full = E * (N + 1) * 4 <= DUMP_FULL_LIMIT
    return {"rewards": host(vec.rewards if full else vec.rewards.index_select(0, idx)),
            "done": host(vec.done if full else vec.done.index_select(0, idx)),
            "obs": host(vec.obs.index_select(0, idx)), "meta": host(vec.meta.index_select(0, idx))}


def run_workload(pkg, torch, name, E, K, W, rank, local_rank, world, run, log_metrics=True, stagger=True, gather=None, dist=None,
                 extras=True, rng_mode="mt19937", windows=5, env_lo=None, kernel_sample=True, capture=False):
    """-> dict of this rank's measurements of one workload.

    Timed region: `windows` back-to-back windows, each EXACTLY K calls of ctf_step_observe and nothing else (no event records, no
    host reads), bracketed by barrier + synchronize on both sides.  With `capture`, the outputs of the last timed step are copied to
    the host right after it (snapshot_outputs -> "outputs").  With `kernel_sample` the per-kernel durations are taken afterwards, in
    SAMPLE_STEPS further steps of the same trajectory issued as ctf_step + ctf_observe with an event around each launch and one
    empty event pair per step (what a pair costs by itself in this stream state: subtracted from the raw figures)."""
    import numpy as np

    sh = pkg.sharding
    label, make_kwargs = WORKLOADS[name]
    kwargs = make_kwargs(pkg)
    device = torch.device("cuda", local_rank)
    lo = rank * E if env_lo is None else int(env_lo)
    seeds = sh.env_seeds(run, lo, lo + E)
    vec = pkg.VecGridworldCtf(E, device=local_rank, py_seeds=seeds, np_seeds=seeds, log_metrics=log_metrics, rng_mode=rng_mode, **kwargs)
    N, G, C = vec.N_AGENTS, vec.GRID_SIZE, vec.N_CHANNELS
    actions = torch.empty((max(W, K, SAMPLE_STEPS), E, N), dtype=torch.int8, device=device)

    def fill(first, count):  # the Philox action streams of steps [first, first + count), generated outside every timed region
        for i in range(count):
            vec.random_actions(actions[i], seed=0xC7F, step=first + i, env_offset=lo)

    vec.observe()  # allocates (and places) the observation buffer
    if stagger:
        stagger_phases(vec, torch, lo, kwargs["GAME_STEPS"])
    observe_kernel = vec.observe_kernel()  # the library's own answer for this buffer (ctf_observe_kernel)
    observe_stores = vec.observe_stores()  # "nontemporal" for batches whose observations exceed the caches (ctf_observe_stores_hinted)

    def one_step(i, t):
        if gather is not None:
            vec.rewards, vec.done = gather.views(t)
        vec.step_observe(actions[i], auto_reset=True)  # the two launches through one call of the C ABI (ctf_step_observe)
        if gather is not None:
            gather.step_done(t)  # closes a chunk every 16th step: issued after the render, it runs beside the next step kernel

    fill(0, W)
    for i in range(W):
        one_step(i, i)
    if gather is not None:
        gather.wait()
    t, win = W, []
    for _ in range(max(1, windows)):
        fill(t, K)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(K):
            one_step(i, t + i)
        if gather is not None:
            gather.flush(t + K)
            gather.wait()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        win.append(time.perf_counter() - t0)
        t += K
    status = vec.status()
    outputs = snapshot_outputs(torch, vec) if capture else None
    out = dict(name=name, label=label, E=E, N=N, G=G, C=C, K=K, W=W, windows=win, env_lo=lo, status=status, outputs=outputs,
               placement_probe_ms=vec.placement_probe_ms, placement_fill_ms=vec.placement_fill_ms, placement=vec.placement, kwargs=kwargs)
    if not kernel_sample:
        vec.close()
        del vec, actions
        torch.cuda.empty_cache()
        return out

    # ---- after the timed region: per-kernel durations
    fill(t, SAMPLE_STEPS)
    if gather is not None:
        vec.rewards, vec.done = gather.views(0)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(SAMPLE_STEPS)]
    for i, e in enumerate(ev):
        e[0].record()
        vec.step(actions[i], auto_reset=True)
        e[1].record()
        vec.observe()
        e[2].record()
        e[3].record()  # (e[2], e[3]): an empty pair
    torch.cuda.synchronize()
    pair = float(np.median([e[2].elapsed_time(e[3]) for e in ev]))
    step_raw = np.array([e[0].elapsed_time(e[1]) for e in ev])
    obs_raw = np.array([e[1].elapsed_time(e[2]) for e in ev])
    step_all, obs_all = np.maximum(step_raw - pair, 0.0), np.maximum(obs_raw - pair, 0.0)
    out.update(status=status | vec.status(), observe_kernel=observe_kernel, observe_stores=observe_stores,
               k_step_ms=float(step_all.mean()), k_observe_ms=float(obs_all.mean()),
               k_step_raw_ms=float(step_raw.mean()), k_observe_raw_ms=float(obs_raw.mean()), event_pair_ms=pair,
               k_step_p=[float(x) for x in np.percentile(step_all, [10, 50, 90])],
               k_observe_p=[float(x) for x in np.percentile(obs_all, [10, 50, 90])],
               kernel_timing_samples=len(ev))
    if extras:
        # outside the timed region: the same env-step with the observation in compact form (ctf_observe_codes: one byte per
        # cell instead of C one-hot bytes — what the GPU policy path consumes)
        fill(t + SAMPLE_STEPS, K)
        torch.cuda.synchronize()
        tc = time.perf_counter()
        for i in range(K):
            vec.step(actions[i], auto_reset=True)
            vec.observe_codes()
        torch.cuda.synchronize()
        out["compact_rate"] = E * K / (time.perf_counter() - tc)
        _, _, nsteps = vec.counters()
        out["episode_phase_spread"] = [int(nsteps.min()), int(nsteps.max())]
    vec.close()
    del vec, actions
    torch.cuda.empty_cache()
    return out


def dryrun_workload(pkg, name, E, K, W, rank, dist, windows=5, env_lo=None):
    """CTF_BENCH_DRYRUN: the shape of run_workload's result with no kernel behind it (each rank 'takes' 1 + rank ms per step, so the
    max-over-ranks rule is visible in the line)."""
    label, make_kwargs = WORKLOADS[name]
    kwargs = make_kwargs(pkg)
    cfg, derived = pkg.config.build_config(kwargs, log_metrics=True)
    win = []
    for w in range(max(1, windows)):
        if dist is not None:
            dist.barrier()
        win.append(K * 1e-3 * (1 + rank) * (1 + 0.01 * abs(w - 2)))  # window 2 is the fastest; the median of five is window 1 or 3
        if dist is not None:
            dist.barrier()
    return dict(name=name, label=label, E=E, N=cfg.n_agents, G=cfg.grid_size, C=cfg.n_channels, K=K, W=W, windows=win,
                env_lo=rank * E if env_lo is None else env_lo, status=0, outputs=None,
                observe_kernel="none (dry run)", observe_stores="none (dry run)", k_step_ms=0.25, k_observe_ms=0.75, k_step_raw_ms=0.25, k_observe_raw_ms=0.75,
                event_pair_ms=0.0, k_step_p=[0.25] * 3, k_observe_p=[0.75] * 3,
                kernel_timing_samples=0, placement_probe_ms=None, placement_fill_ms=None, placement=None, kwargs=kwargs)


def dump_outputs(path, outputs):
    """--dump-outputs: the arrays of snapshot_outputs as path/<name>.npy (a dry run has none to write)."""
    import numpy as np

    if outputs is None:
        print("[bench.py] --dump-outputs: a dry run computes no outputs; nothing written", file=sys.stderr, flush=True)
        return
    os.makedirs(path, exist_ok=True)
    for name, a in outputs.items():
        np.save(os.path.join(path, name + ".npy"), a)
    print(f"[bench.py] wrote {', '.join(f'{k}{list(a.shape)}' for k, a in outputs.items())} "
          f"({sum(a.nbytes for a in outputs.values()) / 2**20:.1f} MiB) to {path}", file=sys.stderr, flush=True)


def reduce_windows(sh, r, device, world, use_dist):
    """The timing rule: per window the MAX over ranks; the line reports the MEDIAN window.  Adds to r: `windows_max` (s),
    `elapsed` (s, the median window), `my_ms` (this rank's own median window, ms per step)."""
    import statistics

    r["windows_max"] = sh.max_over_ranks_list(r["windows"], device, world if not use_dist else max(world, 2))
    r["elapsed"] = statistics.median(r["windows_max"])
    r["my_ms"] = statistics.median(r["windows"]) / r["K"] * 1e3
    return r


def workload_block(r, value, traffic_table, n_gpus=1):
    """The fields every measured workload carries (headline and secondaries alike)."""
    N, G, C, K = r["N"], r["G"], r["C"], r["K"]
    return {
        "value": value, "unit": "env-steps/s", "steps": K, "windows": len(r["windows_max"]), "ms_per_step": r["elapsed"] / K * 1e3,
        "windows_ms_per_step": [w / K * 1e3 for w in r["windows_max"]],
        "roofline": roofline_of(r, traffic_table),
        "whole_step_hbm_frac": env_step_algorithmic_bytes(N, C, G) * value / n_gpus / 1e9 / HBM_PEAK_GBS,
        "kernels_ms": {"k_step": r["k_step_ms"], r["observe_kernel"]: r["k_observe_ms"]},
        "render_stores": r["observe_stores"],
        "kernels_ms_raw_events": {"k_step": r["k_step_raw_ms"], r["observe_kernel"]: r["k_observe_raw_ms"]},
        "event_pair_overhead_ms": r["event_pair_ms"],
        "kernels_ms_p10_p50_p90": {"k_step": r["k_step_p"], r["observe_kernel"]: r["k_observe_p"]},
        "kernel_timing_samples": r["kernel_timing_samples"],
        "kernel_timing": f"{r['kernel_timing_samples']} steps AFTER the timed windows, ctf_step + ctf_observe with a HIP event around each "
                         "launch, net of an empty event pair (event_pair_overhead_ms); the timed windows hold ctf_step_observe only",
        "placement": r["placement"], "placement_probe_ms": r["placement_probe_ms"], "device_status_bits": r["status"],
    }


def roofline_of(r, traffic_table):
    """roofline object of the dominant kernel of one workload's run."""
    N, G, C, E = r["N"], r["G"], r["C"], r["E"]
    kernel, per_env, ms = r["observe_kernel"], observe_algorithmic_bytes(N, C, G), r["k_observe_ms"]
    achieved = per_env * E / (ms * 1e-3) / 1e9
    entry = traffic_table.get(f"{r['name']}_{E}", {})
    hbm = entry.get("k_observe_hbm_bytes_per_launch") if entry.get("kernel", "k_observe") == kernel else None
    return {
        "bound": "hbm",
        "kernel": kernel,
        "achieved": achieved,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS,
        "traffic": hbm,
        "traffic_source": ("profiles/traffic.json (rocprofv3 --pmc WRITE_SIZE / FETCH_SIZE passes of " + entry.get("source", "?") +
                           ", not measured in this run)") if hbm else None,
        "algorithmic_bytes_per_env": per_env,
        "avg_launch_ms": ms,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--envs-per-gpu", type=int, default=65536)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="arena",
                    help="arena: 8_arena on the reference's 15x15 arena_iii (the headline); split: 0_the_split, use with "
                         "--envs-per-gpu 4096; arena20: the 8_arena agents and rules on a synthetic 20x20 map")
    ap.add_argument("--no-metrics", action="store_true", help="compile the reference's metric counters out of the step kernel")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the arena20 / split secondaries of the N=1 line")
    ap.add_argument("--no-stagger", action="store_true", help="start the timed region at episode step 0 with all envs in lock-step")
    ap.add_argument("--rollout-exchange", action="store_true",
                    help="also all-gather the compact rollout tensors (rewards, done) over RCCL, once per 16-step chunk, for a "
                         "centralised learner; off by default: env shards are independent and a data-parallel learner needs no exchange")
    ap.add_argument("--run", type=int, default=1, help="seed family: env seeds are 1_000_003*run + global env index")
    ap.add_argument("--env-offset", type=int, default=0,
                    help="global index of the job's first env (rank r owns [offset + r * E, offset + (r + 1) * E)): e.g. 98304 with "
                         "--envs-per-gpu 32768 is the shard of rank 3 of 8 of configs[3]")
    ap.add_argument("--windows", type=int, default=None,
                    help="back-to-back timed windows of --steps steps each; the line reports the median one (default: 1, with --full 5)")
    ap.add_argument("--configs3-envs", type=int, default=262144,
                    help="GLOBAL env count of the N>1 secondary (BASELINE.json configs[3]: 262 144 envs over the N GPUs)")
    ap.add_argument("--full", action="store_true",
                    help="measure everything, not only the headline: 5 timed windows, per-kernel durations and roofline, the compact "
                         "observation rate, the secondary workloads and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32; rank 0's shard; see the module docstring)")
    args = ap.parse_args()
    if args.windows is None:
        args.windows = 5 if args.full else 1

    rc = world_or_launch(args.gpus, os.path.abspath(__file__), sys.argv[1:])
    if rc is not None:  # this process was the launcher of the N ranks; their rank 0 has printed the line
        sys.exit(rc)

    # stdout carries exactly one JSON line: native libraries (the RCCL banner at communicator init, for one) write to fd 1
    # as well, so fd 1 is pointed at stderr for the run and the result goes out through the saved descriptor
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    import torch

    pkg = importlib.import_module("marl-ctf-development_amd")
    sh = pkg.sharding
    rank, local_rank, world = sh.world_from_env()
    # CTF_BENCH_DRYRUN=1: everything of this file but the kernels — rank bookkeeping, process group (gloo, CPU), barrier, max-over-ranks
    # timing, the self-check and the JSON line — so that the N-rank launch is testable without a GPU (tests/test_bench_launch.py)
    dryrun = bool(os.environ.get("CTF_BENCH_DRYRUN"))
    if dryrun:
        device = torch.device("cpu")
        if os.environ.get("CTF_BENCH_DRYRUN_FAIL_RANK") == str(rank):  # a rank that dies: the job must not exit 0
            raise SystemExit(f"rank {rank}: made to fail (CTF_BENCH_DRYRUN_FAIL_RANK)")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU: the hot path has no CPU fallback")
        if os.environ.get("CTF_BENCH_ONE_DEVICE"):  # rehearsal: N ranks on device 0 (gloo)
            local_rank = 0
        if local_rank >= torch.cuda.device_count():
            raise SystemExit(f"rank {rank}: local rank {local_rank} has no device ({torch.cuda.device_count()} visible)")
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
    # CTF_FORCE_DIST=1 runs the RCCL code path even with one rank (rehearsal of the N>1 path on a 1-GPU box)
    use_dist = world > 1 or bool(os.environ.get("CTF_FORCE_DIST"))
    dist = None
    if use_dist:
        import torch.distributed as dist

        single_rank_rendezvous()
        if dryrun or os.environ.get("CTF_BENCH_ONE_DEVICE"):
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)
    n_gpus = world
    E, K, W = args.envs_per_gpu, args.steps, args.warmup
    t_start = time.perf_counter()

    # The path shards with NO data-path collective: envs are independent, every rank steps and renders its own shard, and a
    # data-parallel learner consumes the observations where they are.  --rollout-exchange adds the hand-off a centralised
    # learner would need: the step kernel writes rewards / done straight into a chunk buffer that is all-gathered (RCCL,
    # async) once per 16 steps.
    exchange = use_dist and args.rollout_exchange
    n_agents = len(WORKLOADS[args.workload][1](pkg)["AGENT_CONFIG"])

    def measure(name, e_rank, k, env_lo=None, use_gather=False, extras=False, rng_mode="mt19937", capture=False):
        """One workload on EVERY rank of the job (a collective call: barriers inside) -> this rank's record with the job-wide
        window times (reduce_windows)."""
        g = sh.ChunkedRolloutGather(e_rank, n_agents, device, world, chunk=16, force_collective=exchange) if use_gather else None
        if dryrun:
            r = dryrun_workload(pkg, name, e_rank, k, W, rank, dist, windows=args.windows, env_lo=env_lo)
        else:
            r = run_workload(pkg, torch, name, e_rank, k, W, rank, local_rank, world, args.run, log_metrics=not args.no_metrics,
                             stagger=not args.no_stagger, gather=g, dist=dist, extras=extras, rng_mode=rng_mode, windows=args.windows,
                             env_lo=env_lo, kernel_sample=args.full, capture=capture)
        return reduce_windows(sh, r, device, world, use_dist)

    r = measure(args.workload, E, K, env_lo=args.env_offset + rank * E, use_gather=exchange, extras=(rank == 0 and args.full),
                capture=(rank == 0 and args.dump_outputs is not None))
    elapsed = r["elapsed"]
    ranks_seen, per_rank_ms = sh.gather_rank_times(rank, r["my_ms"], world if use_dist else 1)
    # a multi-GPU line must verify itself: every rank of the job reported a time, exactly once
    ranks_ok = sh.ranks_complete(ranks_seen, per_rank_ms, n_gpus)

    # BASELINE.json configs[3] at ITS OWN size: 262 144 envs GLOBAL, sharded by global env index over the N ranks of this job
    # (strong scaling: 262 144 / N per GPU; 32 768 at N = 8).  Every rank runs it (barriers inside), rank 0 reports it.
    r3 = None
    if args.full and world > 1 and args.workload == "arena" and not args.no_secondary:
        lo3, hi3 = sh.shard_range(args.configs3_envs, rank, world)
        r3 = measure("arena", hi3 - lo3, max(20, min(K, 100)), env_lo=lo3)
        r3["shards"] = [list(sh.shard_range(args.configs3_envs, q, world)) for q in range(world)]

    if rank == 0:
        N, G, C = r["N"], r["G"], r["C"]
        value = n_gpus * E * K / elapsed
        line = {
            "metric": "env-steps/sec",
            "value": value,
            "unit": "env-steps/s",
            "n_gpus": n_gpus,
            "steps": K,
            "warmup": W,
            "ms_per_step": elapsed / K * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic" if not dryrun else "DRY RUN: no kernel ran, the times are placeholders (CTF_BENCH_DRYRUN)",
            "config": {
                "workload": f"{r['label']}, {E} envs/GPU resident in HBM, step()+observe() per env-step "
                            f"(u8 obs [N={N}][C={C}][{G}][{G}], f16 metadata), Philox uniform actions, auto-reset at GAME_STEPS=500, "
                            + ("envs at staggered episode phases after a discarded first episode" if not args.no_stagger
                               else "all envs in lock-step from episode step 0"),
                "envs_per_gpu": E,
                "global_envs": n_gpus * E,
                "first_global_env": args.env_offset,
                "metrics_counters": not args.no_metrics,
                "ranks_share_one_device": bool(os.environ.get("CTF_BENCH_ONE_DEVICE")),
                "rollout_exchange": ("RCCL all-gather of rewards+done per 16-step chunk, async" if exchange else
                                     "none: env shards are independent (data-parallel learner)"),
                "timed_region": f"{len(r['windows_max'])} back-to-back windows of exactly {K} ctf_step_observe calls (nothing else inside), "
                                "barrier + synchronize on both sides of each, MAX over ranks per window; value / ms_per_step = the MEDIAN window",
            },
        }
        line.update({
            "windows": len(r["windows_max"]),
            "windows_ms_per_step": [w / K * 1e3 for w in r["windows_max"]],
            # where the observation buffer landed: a box whose allocations are all of the slow kind explains its
            # own lower number here — kind, the render's time over a plain fill of the same buffer, the slowest candidate seen
            "placement": r["placement"],
            "placement_probe_ms": r["placement_probe_ms"],
            "placement_fill_ms": r["placement_fill_ms"],
            "device_status_bits": r["status"],
            "ranks_ok": ranks_ok,
            "ranks_seen": sorted(ranks_seen),
            "per_rank_ms_per_step": [per_rank_ms[ranks_seen.index(k)] for k in sorted(ranks_seen)],
            "full": args.full,
        })
        if args.dump_outputs is not None:
            dump_outputs(args.dump_outputs, r["outputs"])
        tpath = os.path.join(ROOT, "profiles", "traffic.json")
        traffic_table = json.load(open(tpath)) if args.full and os.path.exists(tpath) else {}
        if args.full:
            blk = workload_block(r, value, traffic_table, n_gpus)
            for k in ("roofline", "whole_step_hbm_frac", "kernels_ms", "render_stores", "kernels_ms_raw_events",
                      "event_pair_overhead_ms", "kernels_ms_p10_p50_p90", "kernel_timing_samples", "kernel_timing"):
                line[k] = blk[k]
            line.update({
                "step_kernel_gbs": step_algorithmic_bytes(N, G) * E / (r["k_step_ms"] * 1e-3) / 1e9 if r["k_step_ms"] > 0 else None,
                "episode_phase_spread": r.get("episode_phase_spread"),
                "compact_observation": {"env_steps_per_s_per_gpu": r.get("compact_rate"), "obs_bytes_per_env": N * G * G + N * (2 * N + 6) * 2,
                                        "note": "step() + observe_codes(); not the headline metric (the reference's consumers take the one-hot planes)"},
            })
        sec = {}
        if r3 is not None:
            g3 = args.configs3_envs
            v3 = g3 * r3["K"] / r3["elapsed"]
            b3 = workload_block(r3, v3, traffic_table, n_gpus)
            b3.update({
                "workload": f"BASELINE.json configs[3]: {r3['label']}, {g3} envs GLOBAL sharded by global env index over {n_gpus} GPUs "
                            f"({r3['E']} on rank 0), no data-path collective",
                "global_envs": g3, "envs_per_gpu": [hi - lo for lo, hi in r3["shards"]], "shards": r3["shards"], "n_gpus": n_gpus,
                "scaling": "strong",
            })
            sec[f"configs3_{g3}"] = b3
        if args.full and n_gpus == 1 and not args.no_secondary and args.workload == "arena" and not dryrun:
            # (a) the per-GPU shard of configs[3] on an 8-GPU node — 32 768 envs, created here as "rank 3 of 8" (global envs
            # [98 304, 131 072)); (b) the synthetic 20x20 arena; (c) configs[1], 0_the_split at 4 096 envs
            for key, name, e2, lo2 in (("arena_32768", "arena", 32768, 3 * 32768), ("arena20_65536", "arena20", 65536, None),
                                       ("split_4096", "split", 4096, None)):
                r2 = measure(name, e2, max(20, min(K, 100)), env_lo=lo2)
                v2 = e2 * r2["K"] / r2["elapsed"]
                b2 = workload_block(r2, v2, traffic_table)
                b2["workload"] = f"{r2['label']}, {e2} envs" + (
                    f" = the shard of rank 3 of 8 of BASELINE.json configs[3] (262 144 envs global; global envs [{lo2}, {lo2 + e2}))"
                    if lo2 is not None else "")
                sec[key] = b2
            # SURVEY 8(a)'s opt-in counter-based RNG (ctf_env.h CTF_RNG_COUNTER): the same workload with Philox streams in place of
            # the reference's two MT19937 generators — a secondary, never the headline (its trajectories are not the reference's)
            rc = measure("arena", E, max(20, min(K, 100)), rng_mode="counter")
            bc = workload_block(rc, E * rc["K"] / rc["elapsed"], traffic_table)
            bc["workload"] = f"{rc['label']}, {E} envs, rng_mode=counter (Philox4x32-10 streams; parity: the oracle reading the same tape)"
            sec["arena_65536_counter_rng"] = bc
            try:  # the headline's envs as two free-running shards on two streams (what a double-buffering caller gets); never the headline
                b2s = two_shards_two_streams(pkg, torch, "arena", E, max(20, min(K, 100)), W, local_rank, args.run, args.windows)
                b2s["workload"] = f"{r['label']}, {E} envs as 2 shards of {E // 2} on 2 HIP streams of one GPU"
                sec["arena_65536_two_shards"] = b2s
            except Exception as exc:  # a secondary must never cost the headline line
                sec["arena_65536_two_shards"] = {"error": repr(exc)}
            try:  # the boundary's drop-in mode: the reference's own GridworldCtf API driven as ppo.py:59-98 drives it, one env
                sec["facade_1env"] = facade_1env(pkg, r["kwargs"], local_rank)
            except Exception as exc:
                sec["facade_1env"] = {"error": repr(exc)}
            try:  # BASELINE configs[4] on one GPU: self-play rollout (env + two policy networks) + the reference's PPO update
                import bench_rollout

                sec["ppo_selfplay_65536x16"] = bench_rollout.run(envs=65536, steps=16, device=local_rank, order="device")
            except Exception as exc:  # a secondary must never cost the headline line
                sec["ppo_selfplay_65536x16"] = {"error": repr(exc)}
            sec["ppo_selfplay_65536x500"] = selfplay_at_reference_length(torch, local_rank, time.perf_counter() - t_start)
        if sec:
            line["secondary"] = sec
        if args.full and n_gpus == 1 and not args.no_cpu_baseline and not dryrun:
            line["cpu_baseline"] = cpu_baseline(pkg, r["kwargs"])
        line["wall_s"] = time.perf_counter() - t_start
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(line) + "\n").encode())
    if use_dist:
        dist.destroy_process_group()
    if not ranks_ok:
        raise SystemExit(f"bench.py --gpus {n_gpus}: ranks seen {sorted(ranks_seen)} with times {per_rank_ms} — not every rank of the job reported")


if __name__ == "__main__":
    main()

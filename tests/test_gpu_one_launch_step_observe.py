"""ctf_step_observe as ONE launch (k_step_observe: step blocks, ring regeneration, then render tiles that wait for the step blocks
of their own envs) against the two launches of ctf_step + ctf_observe, bit for bit after every step: observations, metadata,
rewards (f32 and f64), done; and at intervals every counter, both generators' states (or the counter-mode stream positions),
sampled full state views and the status word.  The two paths run on twin handles seeded alike, in one process; the
environment switch CTF_STEP_OBSERVE_ONE_LAUNCH is read at every call."""
import numpy as np
import pytest

from _cases import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ONE, TWO = "1", "0"


def _kwargs(name):
    if name == "arena20":
        return dict(pkg.configs.ARENA20_KWARGS, SCENARIO=pkg.configs.arena20_scenario())
    if name == "split":
        return dict(pkg.configs.SPLIT_KWARGS, SCENARIO=pkg.CtfScenarios.arrow)
    return dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii)


def _twins(name, n_envs, **opts):
    seeds = np.arange(n_envs, dtype=np.uint64) * 7919 + 11
    make = lambda: pkg.VecGridworldCtf(n_envs, device=0, py_seeds=seeds, np_seeds=seeds, tune_placement=False, **opts, **_kwargs(name))
    return make(), make()


def _step(vec, path, acts, monkeypatch, auto_reset=True):
    monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", path)
    assert vec.step_observe_launches() == (1 if path == ONE else 2)
    vec.step_observe(acts, auto_reset=auto_reset, want_f64=True)


def _same_outputs(a, b, ctx):
    assert torch.equal(a.obs, b.obs), f"{ctx}: observations"
    assert torch.equal(a.meta.view(torch.int16), b.meta.view(torch.int16)), f"{ctx}: metadata"
    assert torch.equal(a.rewards.view(torch.int32), b.rewards.view(torch.int32)), f"{ctx}: rewards f32"
    assert torch.equal(a.rewards64.view(torch.int64), b.rewards64.view(torch.int64)), f"{ctx}: rewards f64"
    assert torch.equal(a.done, b.done), f"{ctx}: done"


def _same_state(a, b, ctx, sample=()):
    for x, y, what in zip(a.counters(), b.counters(), ("metrics", "captures", "step counts")):
        assert torch.equal(x, y), f"{ctx}: {what}"
    if a.rng_mode == "counter":
        assert torch.equal(a.get_rng_counters(), b.get_rng_counters()), f"{ctx}: RNG counters"
    else:
        for x, y in zip(a.get_rng_states(), b.get_rng_states()):
            assert torch.equal(x, y), f"{ctx}: MT19937 states"
    for e in sample:
        assert bytes(a.get_state(e)) == bytes(b.get_state(e)), f"{ctx}: state view of env {e}"


def _run(a, b, steps, monkeypatch, ctx, check_every=25, seed=0x51DE, auto_reset=True):
    acts = torch.empty((a.n_envs, a.N_AGENTS), dtype=torch.int8, device=a.device)
    sample = sorted({0, a.n_envs // 3, a.n_envs - 1})
    for t in range(steps):
        a.random_actions(acts, seed=seed, step=t)
        _step(a, ONE, acts, monkeypatch, auto_reset)
        _step(b, TWO, acts, monkeypatch, auto_reset)
        _same_outputs(a, b, f"{ctx} step {t}")
        if t % check_every == check_every - 1 or t == steps - 1:
            _same_state(a, b, f"{ctx} step {t}", sample)
    assert a.status() == 0 and b.status() == 0, ctx


def test_bench_size_over_an_episode_end_and_a_visitation_fold(monkeypatch):
    """8_arena at 65 536 envs (bench.py's variant: metrics and visitation log on) for 520 steps: every env ends its episode at
    step 500 and is reset inside the launch."""
    a, b = _twins("arena", 65536, log_metrics=True)
    assert a.observe_kernel() == "k_observe_tiles"
    _run(a, b, 520, monkeypatch, "arena 65536", check_every=65)
    a.close(), b.close()


def test_no_auto_reset_crosses_the_visitation_fold(monkeypatch):
    """Without auto-reset the envs run past GAME_STEPS and fold their visitation log in-kernel at step 511."""
    a, b = _twins("arena", 2048, log_metrics=True)
    _run(a, b, 520, monkeypatch, "arena 2048 no auto-reset", check_every=104, auto_reset=False)
    a.close(), b.close()


@pytest.mark.parametrize("name,n_envs,opts", [
    ("arena20", 4096, {}),
    ("arena", 1000, {}),                      # ragged: not a multiple of a step block's envs
    ("arena", 777, {"log_metrics": False}),
    ("arena", 1536, {"rng_mode": "counter"}),
])
def test_configurations(name, n_envs, opts, monkeypatch):
    a, b = _twins(name, n_envs, **opts)
    if a.observe_kernel() != "k_observe_tiles":
        pytest.fail(f"{name}: the tile render does not apply, so neither does the single launch")
    _run(a, b, 160, monkeypatch, f"{name} {n_envs} {opts}")
    a.close(), b.close()


def test_without_the_tile_render_it_stays_two_launches(monkeypatch):
    """0_the_split's observation block (3 872 bytes) is smaller than a tile: ctf_observe takes k_observe, ctf_step_observe the
    two launches whatever the switch says."""
    a, _ = _twins("split", 64)
    monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", ONE)
    assert a.observe_kernel() == "k_observe" and a.step_observe_launches() == 2
    a.close(), _.close()


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_every_step_lane_width(lanes, monkeypatch):
    monkeypatch.setenv("CTF_STEP_W", str(lanes))  # read when the handle is created
    a, b = _twins("arena", 1200)
    _run(a, b, 120, monkeypatch, f"W={lanes}")
    a.close(), b.close()


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
@pytest.mark.parametrize("log_metrics,nt", [(False, None), (True, "1"), (False, "1")])
def test_every_step_lane_width_of_the_other_variants(lanes, log_metrics, nt, monkeypatch):
    """The rest of the one launch's dispatch: k_step_observe<METRICS, W, STORE_NT> without metrics and with hinted stores at every
    W (the test above runs <true, W, 0>).  CTF_OBS_NT forces the hint at a size far below the rule's; 65 envs: at every width the
    last step block is a ragged one of a single env."""
    monkeypatch.setenv("CTF_STEP_W", str(lanes))  # both read when the handle is created
    if nt is not None:
        monkeypatch.setenv("CTF_OBS_NT", nt)
    a, b = _twins("arena", 65, log_metrics=log_metrics)
    assert a.observe_kernel() == "k_observe_tiles" and a.observe_stores() == ("nontemporal" if nt == "1" else "plain")
    _run(a, b, 40, monkeypatch, f"W={lanes} metrics={log_metrics} nt={nt}", check_every=20)
    a.close(), b.close()


def test_captured_launch_replays(monkeypatch):
    """The launch reads no argument that moves from call to call: a captured graph of K one-launch steps replayed several times
    (the generation number in device memory advances by itself) equals the two-launch path called eagerly."""
    K, REPLAYS = 4, 5
    a, b = _twins("arena", 3000)
    acts = torch.empty((K, a.n_envs, a.N_AGENTS), dtype=torch.int8, device=a.device)
    for k in range(K):
        a.random_actions(acts[k], seed=0xC0DE, step=k)
    obs = torch.empty((K,) + tuple(a.obs.shape), dtype=torch.uint8, device=a.device)
    monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", ONE)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=a.device)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        for k in range(K):
            a.step_observe(acts[k], auto_reset=True, want_f64=True)
            obs[k].copy_(a.obs)
    torch.cuda.synchronize()
    for r in range(REPLAYS):
        graph.replay()
        torch.cuda.synchronize()
        for k in range(K):
            _step(b, TWO, acts[k], monkeypatch)
            assert torch.equal(obs[k], b.obs), f"replay {r} step {k}: observations"
        _same_outputs(a, b, f"replay {r}")
        _same_state(a, b, f"replay {r}", (0, a.n_envs - 1))
    assert a.status() == 0 and b.status() == 0
    a.close(), b.close()


def test_two_handles_on_two_streams_at_once(monkeypatch):
    """Two handles (each its own sync words) whose single launches run concurrently on two streams, against their two-launch twins."""
    a1, b1 = _twins("arena", 4096)
    a2, b2 = _twins("arena20", 2048)
    s1, s2 = torch.cuda.Stream(device=a1.device), torch.cuda.Stream(device=a1.device)
    acts1 = torch.empty((a1.n_envs, a1.N_AGENTS), dtype=torch.int8, device=a1.device)
    acts2 = torch.empty((a2.n_envs, a2.N_AGENTS), dtype=torch.int8, device=a1.device)
    for t in range(100):
        a1.random_actions(acts1, seed=1, step=t)
        a2.random_actions(acts2, seed=2, step=t)
        torch.cuda.synchronize()
        monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", ONE)
        with torch.cuda.stream(s1):
            a1.step_observe(acts1, auto_reset=True, want_f64=True)
        with torch.cuda.stream(s2):
            a2.step_observe(acts2, auto_reset=True, want_f64=True)
        _step(b1, TWO, acts1, monkeypatch)
        _step(b2, TWO, acts2, monkeypatch)
        torch.cuda.synchronize()
        _same_outputs(a1, b1, f"handle 1 step {t}")
        _same_outputs(a2, b2, f"handle 2 step {t}")
    _same_state(a1, b1, "handle 1", (0,))
    _same_state(a2, b2, "handle 2", (0,))
    assert all(v.status() == 0 for v in (a1, b1, a2, b2))
    for v in (a1, b1, a2, b2):
        v.close()

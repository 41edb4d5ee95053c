"""k_reset_scattered (ctf_reset_scattered; VecGridworldCtf.reset_scattered, ScatteredStarts, collect(starts=...)) on the device:
positions and grids must equal tests/_scatter_ref.py for every config and argument combination of tests/_scatter_cases.py, in batches
of 1, 3 and 67 envs; everything else is a plain reset's; `perm`, both generators and the envs outside the mask stay; radius 0 and an
empty agent mask are ctf_reset bit for bit; a twin planted with the exported state continues identically, and so does the oracle;
visitation, the renders (a retained buffer included), a captured graph that draws afresh at every replay, refusals, the collector."""
import numpy as np
import pytest

import oracle
import _scatter_cases as scs
import _scatter_ref as sr
import _scripted_cases as sc
from _cases import pkg, view_arrays
from _stub_policy import StubPolicy
from test_gpu_agent_counts import _segments

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RECORD = ("hp", "has_flag", "inventory", "step_count", "team_captures", "done")


def _vec(kw, n_envs, **more):
    seeds = np.arange(n_envs, dtype=np.uint64) * 13 + 5
    return pkg.VecGridworldCtf(n_envs, device=0, tune_placement=False, py_seeds=seeds, np_seeds=seeds, **more, **kw)


def _arena(**over):
    return dict(sc.workloads()["arena"], **over)


def _u32(vec, values):
    return torch.from_numpy(np.asarray(values, np.uint32)).to(vec.device)


def _play(vec, steps, seed=0xACE):
    acts = torch.empty((vec.n_envs, vec.N_AGENTS), dtype=torch.int8, device=vec.device)
    for t in range(steps):
        vec.random_actions(acts, seed, t, 0)
        vec.step(acts)
    return acts


def _i64(t):
    return t.to(torch.int64)  # (torch compares no uint32)


def _host(states):
    return {k: v.cpu().numpy() for k, v in states.items()}


def _generators(vec):
    if vec.rng_mode == "mt19937":
        return [x.cpu().numpy() for x in vec.get_rng_states()]
    return [vec.get_rng_counters().cpu().numpy()]


def _want(rules, cells):
    """the restatement's grids and positions of a batch -> (uint8 [E, G, G], int8 [E, N, 2])"""
    both = [sr.state(rules, row) for row in cells]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


# ---- against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", scs.config_names())
def test_positions_and_grids_match_the_restatement(name):
    kw, cfg = scs.configs()[name]
    rules = sr.cfg_rules(cfg)
    vecs = {E: _vec(kw, E) for E in scs.BATCHES}
    plain = {E: _host(v.get_states()) for E, v in vecs.items()}  # a fresh handle is a reset one
    envs = np.arange(67, dtype=np.uint64) + scs.ENV_OFFSET
    moved = 0
    for k, (radius, own_side, mask, seed, rnd, ep) in enumerate(scs.combos(cfg)):
        cells = sr.place(rules, mask, radius, own_side, seed, envs, rnd + ep)
        grids, pos = _want(rules, cells)
        moved += int((pos != np.array(rules["starts"], np.int8)[None]).any())
        for E, vec in vecs.items():
            if k % 8 == 3 and name in ("arena", "split", "large32"):  # from a played state, not from the last combo's (nobody falls in two steps there)
                _play(vec, 2, seed=k)
            perm = vec.get_states(fields=("perm",))["perm"].clone()
            episodes = _u32(vec, [ep] * E)
            vec.reset_scattered(radius=radius, agent_mask=mask, own_side=own_side, seed=seed, round=rnd, episodes=episodes, env_offset=scs.ENV_OFFSET)
            got = _host(vec.get_states())
            ctx = f"{name} combo {k} (radius {radius}, own side {own_side}, agents 0x{mask:x}, round {rnd} + {ep}), {E} envs"
            assert np.array_equal(got["pos"], pos[:E]), ctx
            assert np.array_equal(got["grid"], grids[:E]), ctx
            for f in RECORD + ("metrics",):  # everything else is a plain reset's
                assert np.array_equal(got[f].view(np.uint8), plain[E][f].view(np.uint8)), (ctx, f)
            assert np.array_equal(got["perm"], perm.cpu().numpy()), ctx
            assert episodes.cpu().numpy().tolist() == [(ep + 1) & sr.U32] * E, ctx
            if E == 67 or k % 5 == 0:  # the maps at step 0: 1 at every agent's cell
                vis = vec.visitation().cpu().numpy()
                assert np.array_equal(vis, np.stack([sr.visitation(rules, row) for row in cells[:E]]).astype(np.uint32)), ctx
    assert moved > 20
    for vec in vecs.values():
        assert vec.status() == 0
        vec.close()


@pytest.mark.parametrize("rng_mode,log_metrics", [("mt19937", True), ("mt19937", False), ("counter", True), ("counter_direct", True), ("counter_direct", False)])
def test_record_is_a_resets_and_the_generators_stay(rng_mode, log_metrics):
    kw = _arena()
    A, B = (_vec(kw, 67, rng_mode=rng_mode, log_metrics=log_metrics) for _ in range(2))
    rules = sr.cfg_rules(A.cfg)
    for v in (A, B):
        _play(v, 5)
    perm, gens = A.get_states(fields=("perm",))["perm"].cpu().numpy(), _generators(A)
    A.reset_scattered(radius=2, seed=11, round=4)
    B.reset()
    a, b = _host(A.get_states()), _host(B.get_states())
    for f in RECORD + (("metrics",) if log_metrics else ()):
        assert np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)), f
    assert np.array_equal(a["perm"], perm) and np.array_equal(b["perm"], perm)
    for x, y in zip(_generators(A), gens):
        assert np.array_equal(x, y)
    grids, pos = _want(rules, sr.place(rules, 0xFF, 2, False, 11, np.arange(67), 4))
    assert np.array_equal(a["pos"], pos) and np.array_equal(a["grid"], grids)
    assert not np.array_equal(a["pos"], b["pos"])
    assert A.status() == 0
    A.close(), B.close()


# ---- masking ---------------------------------------------------------------------------------------------------------------------
def test_envs_outside_the_mask_are_untouched():
    kw = _arena()
    vec = _vec(kw, 67)
    rules = sr.cfg_rules(vec.cfg)
    _play(vec, 5)
    mask_host = (np.arange(67) % 3 == 1).astype(np.uint8) * np.where(np.arange(67) % 2, 1, 200).astype(np.uint8)  # mixed non-zero bytes
    mask_host[[0, 66]] = (7, 0)
    mask = torch.from_numpy(mask_host).to(vec.device)
    ep_host = (np.arange(67, dtype=np.uint32) * 7 + 1)
    ep_host[0] = 0xFFFFFFFF
    episodes = _u32(vec, ep_host)
    before, vis_before = vec.save_states().cpu().numpy(), vec.visitation().cpu().numpy()
    vec.reset_scattered(mask=mask, radius=2, own_side=True, seed=0x5EED, round=3, episodes=episodes)
    after, vis_after, ep_after = vec.save_states().cpu().numpy(), vec.visitation().cpu().numpy(), episodes.cpu().numpy()
    on = mask_host != 0
    assert 20 < on.sum() < 30
    assert np.array_equal(after[~on], before[~on]) and np.array_equal(vis_after[~on], vis_before[~on])  # snapshot records, byte for byte
    assert np.array_equal(ep_after[~on], ep_host[~on]) and np.array_equal(ep_after[on], ep_host[on] + np.uint32(1)) and ep_after[0] == 0
    cells = sr.place(rules, 0xFF, 2, True, 0x5EED, np.arange(67), 3 + ep_host.astype(np.uint64))
    grids, pos = _want(rules, cells)
    got = _host(vec.get_states(fields=("pos", "grid", "step_count")))
    assert np.array_equal(got["pos"][on], pos[on]) and np.array_equal(got["grid"][on], grids[on])
    assert (got["step_count"][on] == 0).all() and (got["step_count"][~on] == 5).all()
    assert vec.status() == 0
    vec.close()


# ---- equality with ctf_reset -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_metrics", [True, False])
@pytest.mark.parametrize("how", ["radius0", "radius0_episodes", "nobody", "nobody_episodes"])
def test_radius_zero_and_an_empty_agent_mask_are_ctf_reset(how, log_metrics):
    kw = _arena()
    for E in scs.BATCHES:
        A, B = (_vec(kw, E, log_metrics=log_metrics) for _ in range(2))
        for v in (A, B):
            _play(v, 5)
        episodes = _u32(A, np.arange(E) + 9) if how.endswith("episodes") else None
        if how.startswith("radius0"):
            A.reset_scattered(radius=0, seed=5, round=1, episodes=episodes)
        else:
            A.reset_scattered(radius=3, agent_mask=0, seed=5, round=1, episodes=episodes)
        B.reset()
        a, b = _host(A.get_states()), _host(B.get_states())
        assert sorted(a) == sorted(b) and all(np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)) for f in a)
        # snapshot records: every byte that means something — header, record (misc[3]'s flags among them), grid, both generators,
        # counters.  Under CTF_F_BASE_ZERO with an empty log the vis and vislog segments are memory nobody has written since
        # hipMalloc (ctf_create clears neither; tests/test_gpu_agent_counts.py reads them by meaning too): the maps are compared as
        # visitation() shows them
        ra, rb = A.save_states().cpu().numpy(), B.save_states().cpu().numpy()
        cut = _segments(A)[0]["vis"][0] if log_metrics else ra.shape[1]
        assert ra.shape == rb.shape and np.array_equal(ra[:, :cut], rb[:, :cut])
        if log_metrics:
            assert torch.equal(_i64(A.visitation()), _i64(B.visitation()))
        if episodes is not None:
            assert episodes.cpu().numpy().tolist() == (np.arange(E) + 10).tolist()  # still advanced
        assert A.status() == 0
        A.close(), B.close()


# ---- continuation, visitation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_metrics", [True, False])
def test_a_twin_planted_with_the_exported_state_continues_identically(log_metrics):
    kw = _arena()
    E = 67
    A, B = (_vec(kw, E, log_metrics=log_metrics) for _ in range(2))
    n, g = A.N_AGENTS, A.GRID_SIZE
    A.reset_scattered(radius=2, seed=21)
    st = A.get_states()
    st.pop("metrics", None)
    if log_metrics:
        vis0 = A.visitation()
        assert (vis0.cpu().numpy().reshape(E, n, -1).sum(axis=2) == 1).all()  # 1 at the drawn cell, nothing else
        pos = st["pos"].cpu().numpy().astype(np.int64)
        assert (vis0.cpu().numpy()[np.arange(E)[:, None], np.arange(n)[None, :], pos[..., 0], pos[..., 1]] == 1).all()
        st["visitation"] = (_i64(vis0) & 0xFF).to(torch.uint8)
    B.set_states(st)
    ref = oracle.OracleEnv(A.cfg)  # env 0 against the oracle, from the same planted state and generators
    ref.seed(5, 5)
    ref.set_state(A.get_state(0))
    acts = torch.empty((E, n), dtype=torch.int8, device=A.device)
    for t in range(8):
        A.random_actions(acts, 0xBEE, t, 0)
        ra, da = A.step(acts, want_f64=True)
        r64a = A.rewards64.clone()
        rb, db = B.step(acts, want_f64=True)
        assert torch.equal(r64a.view(torch.int64), B.rewards64.view(torch.int64)) and torch.equal(da, db), t
        a, b = A.get_states(), B.get_states()
        assert all(torch.equal(a[f].view(torch.uint8), b[f].view(torch.uint8)) for f in a), t
        if log_metrics:
            va = A.visitation()
            assert torch.equal(_i64(va), _i64(B.visitation())), t
            assert (va.cpu().numpy().reshape(E, n, -1).sum(axis=2) == t + 2).all(), t  # scatter plus k steps: k + 1 visits
        rw, dn, status = ref.step(acts[0].cpu().numpy())
        assert status == 0 and np.array_equal(r64a[0].cpu().numpy().view(np.uint64), np.asarray(rw, np.float64).view(np.uint64)) and int(da[0]) == int(dn), t
        got, want = view_arrays(A.get_state(0), n, g), view_arrays(ref.get_state(), n, g)
        for key in ("grid", "pos", "hp", "has_flag", "inv", "perm", "step_count", "done", "team_captures") + (("metrics", "visitation") if log_metrics else ()):
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), (t, key)
    py, npw = A.get_rng_state(0)
    rpy, rnp = ref.get_rng_state()
    assert np.array_equal(py, rpy) and np.array_equal(npw, rnp)
    assert A.status() == 0 and B.status() == 0
    A.close(), B.close()


# ---- renders ---------------------------------------------------------------------------------------------------------------------------
def test_renders_after_a_scatter_match_the_oracle():
    kw = _arena()
    E = 67
    vec = _vec(kw, E)
    n = vec.N_AGENTS
    assert vec.observe_retained() == 1
    _play(vec, 3)
    vec.observe()  # the retained buffer's shadow now holds the played state
    mask = torch.from_numpy((np.arange(E) % 4 != 2).astype(np.uint8)).to(vec.device)
    vec.reset_scattered(mask=mask, radius=3, seed=77)
    obs, meta = vec.observe()  # no invalidate_obs: a state change like reset
    obs, meta = obs.cpu().numpy(), meta.cpu().numpy().view(np.uint16)
    codes, _ = vec.observe_codes()
    assert torch.equal(pkg.expand_codes(codes, vec.N_CHANNELS).cpu(), torch.from_numpy(obs))
    fresh = torch.zeros_like(vec.obs)  # the same render into a buffer of the caller's: in full
    other = _vec(kw, E)
    other.set_states({k: v for k, v in vec.get_states().items() if k != "metrics"})
    other.obs = fresh
    assert other.observe_retained() == 0
    assert np.array_equal(other.observe()[0].cpu().numpy(), obs)
    ref = oracle.OracleEnv(vec.cfg)
    for e in (0, 1, 2, 3, 33, 66):
        ref.set_state(vec.get_state(e))
        ro, rm = ref.observe()
        assert np.array_equal(obs[e], ro) and np.array_equal(meta[e], rm.view(np.uint16)), e
    assert vec.status() == 0
    vec.close(), other.close()


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
def test_a_captured_graph_draws_afresh_at_every_replay():
    kw = _arena(GAME_STEPS=1)  # every step ends the episode: every env is done at every replay
    E = 67
    vec = _vec(kw, E)
    rules = sr.cfg_rules(vec.cfg)
    dev = vec.device
    acts = torch.full((E, vec.N_AGENTS), 4, dtype=torch.int8, device=dev)
    episodes = _u32(vec, [0] * E)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph, stream=side):  # capture only: nothing runs
        vec.step(acts)
        vec.reset_scattered(mask=vec.done, radius=2, seed=0x6A9, round=0, episodes=episodes)
    torch.cuda.synchronize(dev)
    seen = []
    for rep in range(3):
        graph.replay()
        torch.cuda.synchronize(dev)
        assert bool(vec.done.all()) and episodes.cpu().numpy().tolist() == [rep + 1] * E
        got = _host(vec.get_states(fields=("pos", "grid", "step_count")))
        grids, pos = _want(rules, sr.place(rules, 0xFF, 2, False, 0x6A9, np.arange(E), rep))
        assert np.array_equal(got["pos"], pos) and np.array_equal(got["grid"], grids) and (got["step_count"] == 0).all(), rep
        seen.append(got["pos"])
    assert all((seen[a] != seen[b]).any() for a, b in ((0, 1), (0, 2), (1, 2)))
    assert vec.status() == 0
    vec.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_state_alone():
    vec = _vec(_arena(), 3)
    _play(vec, 2)
    episodes = _u32(vec, [1, 2, 3])
    odd = torch.zeros(32, dtype=torch.uint8, device=vec.device)
    before = vec.save_states().cpu().numpy()
    call = lambda *a: vec._lib.ctf_reset_scattered(vec._h, None, *a, 0, vec._stream())  # noqa: E731
    ep = episodes.data_ptr()
    for args in ((0xFF, -1, 0, 5, 0, ep), (0x100, 1, 0, 5, 0, ep), (0xFF, 1, 2, 5, 0, ep), (0xFF, 1, 0x80000001, 5, 0, ep), (0xFF, 1, 0, 5, 0, odd.data_ptr() + 1),
                 (0xFF, 1, 0, 5, 0, odd.data_ptr() + 2)):
        assert call(*args) == -1, args
    assert vec._lib.ctf_reset_scattered(None, None, 0xFF, 1, 0, 5, 0, ep, 0, vec._stream()) == -1
    torch.cuda.synchronize(vec.device)
    assert np.array_equal(vec.save_states().cpu().numpy(), before) and episodes.cpu().numpy().tolist() == [1, 2, 3]
    with pytest.raises(ValueError):
        vec.reset_scattered(radius=-1)
    with pytest.raises(ValueError):
        vec.reset_scattered(agent_mask=1, team=0)
    with pytest.raises(ValueError):
        vec.reset_scattered(agent_mask=1 << 8)
    with pytest.raises(ValueError):
        vec.reset_scattered(episodes=torch.zeros(3, dtype=torch.int32, device=vec.device))
    assert vec.status() == 0
    vec.close()


# ---- the collector ---------------------------------------------------------------------------------------------------------------------
def test_the_collector_with_scattered_starts():
    kw = _arena()
    E, T = 8, 4
    vec, A, B = (_vec(kw, E) for _ in range(3))
    starts = pkg.ScatteredStarts(2)
    out = pkg.BatchedRolloutCollector(vec, T, 0).collect(StubPolicy(1), StubPolicy(2), starts=starts)
    first = out["grid_states"][0]  # slot 0: the first trained agent's view of every env at step 0
    assert first.shape[0] == E and any(not torch.equal(first[0], first[e]) for e in range(1, E))
    assert starts.episodes(vec).cpu().numpy().tolist() == [1] * E
    # starts=None is the parent's behaviour: the same tensors as a collect behind a reset of the caller's own
    a = pkg.BatchedRolloutCollector(A, T, 0).collect(StubPolicy(1), StubPolicy(2))
    B.reset()
    b = pkg.BatchedRolloutCollector(B, T, 0).collect(StubPolicy(1), StubPolicy(2), reset=False)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.equal(a["grid_states"][0][0], a["grid_states"][0][e]) for e in range(1, E))  # config starts: one start state
    for v in (vec, A, B):
        assert v.status() == 0
        v.close()

"""Visitation maps on the device (ctf_harvest_visitation / ctf_export_visitation, VecGridworldCtf.harvest_visitation / visitation,
harvest.EpisodeHarvest(visitation=True), duel.batched_duel / batched_tournament(visitation=True)).

Expected values come from the CPU oracle alone: per oracle env an int64 [N, G, G] array, set to 1 at the start cells after reset()
and incremented at ``view.pos`` after every step; before it is used ``counts & 0xFF`` is compared with the oracle's own (pinned)
uint8 visitation maps.  Integer sums: every comparison is exact.  Each shape is the smallest at which its path is exercised."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import oracle  # noqa: E402
from _cases import abi, pkg, view_arrays  # noqa: E402
from _stub_policy import StubDuelPolicy  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ACT_SEED = 0x4A57
STAGGER_SEED = 0x5747  # bench.stagger_phases' action stream
SHORT_SEED = 3         # test_gpu_harvest.py's short-episode config
DENSE_SEED = 13        # of the 5 x 5 map (chosen on the CPU with the oracle alone: a count passes 255 within 600 steps, status 0)


def _arena(**over):
    return dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii, **over)


def _fuzz_kwargs(seed, game_steps, n_agents=None, grid=None):
    """A capture-dense map in the style of the committed fuzz fixtures (make_golden_fuzz.random_scenario)."""
    import make_golden_fuzz as mgf

    rng = np.random.default_rng(seed)
    while True:
        scen, agents = mgf.random_scenario(rng, "Visitation")
        if (n_agents is None or len(agents) == n_agents) and (grid is None or scen["GRID_SIZE"] == grid):
            break
    return dict(GRID_SIZE=scen["GRID_SIZE"], AGENT_CONFIG=agents, GAME_STEPS=game_steps, MAP_SYMMETRY_CHECK=False, HOME_FLAG_CAPTURE=False,
                DROP_FLAG_WHEN_NO_HP=True, USE_ADJUSTED_REWARDS=True, TAG_PROBABILITY=0.5, AGENT_TYPE_HP={0: 10, 1: 8, 2: 8, 3: 7},
                AGENT_TYPE_DAMAGE={0: 1, 1: 0.5, 2: 0.5, 3: 1}, GUARDIAN_DAMAGE_MULTIPLIER=5.0, VAULT_HP_COST=1.25, SCENARIO=scen)


def _largest_kwargs():
    """N = 16, G = 32, the largest shape the ABI accepts: an open map, the teams' agents in two columns."""
    G, N = 32, 16
    starts = {i: (4 + 3 * (i // 2), 10 if i % 2 == 0 else 21) for i in range(N)}
    scen = dict(SCENARIO_NAME="Open32", GRID_SIZE=G, FLIP_AXIS=None, FLAG_POSITIONS={0: (15, 3), 1: (16, 28)},
                CAPTURE_POSITIONS={0: (15, 3), 1: (16, 28)}, SPAWN_POSITIONS={0: (8, 6), 1: (23, 25)},
                AGENT_STARTING_POSITIONS=starts, BLOCK_TILE_SLICES=[], DESTRUCTIBLE_TILE_SLICES=[])
    return dict(GRID_SIZE=G, AGENT_CONFIG={i: {"team": i % 2, "type": (i // 2) % 4} for i in range(N)}, GAME_STEPS=100,
                MAP_SYMMETRY_CHECK=False, TAG_PROBABILITY=0.5, SCENARIO=scen)


def _make(n_envs, kw, seed_base=11, log_metrics=True):
    seeds = np.arange(n_envs, dtype=np.uint64) * 7919 + seed_base
    return pkg.VecGridworldCtf(n_envs, device=0, py_seeds=seeds, np_seeds=seeds, log_metrics=log_metrics, tune_placement=False, **kw), seeds


class Tracked:
    """One oracle env and the test's own true visit counts."""

    def __init__(self, cfg, seed):
        self.env = oracle.OracleEnv(cfg)
        self.env.seed(int(seed), int(seed))
        self.n, self.g = cfg.n_agents, cfg.grid_size
        self.counts = np.zeros((self.n, self.g, self.g), np.int64)
        self._mark()

    def _mark(self):
        v = self.env.get_state()
        for i in range(self.n):
            self.counts[i, v.pos[i][0], v.pos[i][1]] += 1
        return v

    def reset(self):
        self.env.reset()
        self.counts[:] = 0
        self._mark()

    def step(self, actions):
        """-> the env's view after the step"""
        _, _, status = self.env.step(actions)
        assert status == 0
        return self._mark()

    def done(self):
        return bool(self.env.get_state().done)

    def checked(self):
        """the counts, tied to the pinned oracle: their u8 wrap is its visitation maps"""
        assert np.array_equal((self.counts & 0xFF).astype(np.uint8), view_arrays(self.env.get_state(), self.n, self.g)["visitation"])
        return self.counts


def _tracked(cfg, seeds, envs=None):
    return {int(e): Tracked(cfg, seeds[e]) for e in (range(len(seeds)) if envs is None else envs)}


def _i64(t):
    """uint32 counts (all below 2^31) as int64"""
    return t.view(torch.int32).long()


def _acts(vec):
    return torch.empty((vec.n_envs, vec.N_AGENTS), dtype=torch.int8, device=vec.device)


def _table(vec, n_groups):
    return torch.zeros((n_groups, vec.N_AGENTS, vec.GRID_SIZE, vec.GRID_SIZE), dtype=torch.int64, device=vec.device)


def test_staggered_auto_reset_run_equals_the_oracle():
    """96 envs of the short-episode config, staggered, 5 groups by a fixed permutation, 130 step(auto_reset) calls, both harvests
    after every step.  Expected: the oracle envs' counts read just before they reset."""
    import bench

    E, G, steps, kw = 96, 5, 130, _fuzz_kwargs(SHORT_SEED, 40, n_agents=8)
    vec, seeds = _make(E, kw)
    n, gs = vec.N_AGENTS, int(vec.cfg.game_steps)
    assert (n, gs) == (8, 40) and vec.visitation_words == n * vec.GRID_SIZE ** 2
    refs = _tracked(vec.cfg, seeds)
    groups_h = np.random.default_rng(1).permutation(E) % G
    groups = torch.from_numpy(groups_h.astype(np.int32)).to(vec.device)
    bench.stagger_phases(vec, torch, 0, gs)
    for s in range(gs):  # the same steps and resets on the CPU
        for e, r in refs.items():
            if r.done():
                r.reset()
            r.step(oracle.philox_actions(n, STAGGER_SEED, s, e))
            if e % gs == s:
                r.reset()
    acts = _acts(vec)
    acc = torch.zeros((G, vec.harvest_words), dtype=torch.int64, device=vec.device)
    table = _table(vec, G)
    want = np.zeros(tuple(table.shape), np.int64)
    episodes = np.zeros(G, np.int64)
    for t in range(steps):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        vec.step(acts, auto_reset=True)
        vec.harvest_visitation(table, groups)
        vec.harvest(acc, groups)
        for e, r in refs.items():
            if r.done():
                r.reset()
            v = r.step(oracle.philox_actions(n, ACT_SEED, t, e))
            if v.done:
                assert v.step_count == gs
                want[groups_h[e]] += r.checked()
                episodes[groups_h[e]] += 1
    assert (episodes >= 2).all(), f"a group finished fewer than 2 episodes: {episodes}"
    assert len({want[k].tobytes() for k in range(G)}) >= 2, "every group's table is the same"
    got = table.cpu()
    assert torch.equal(got, torch.from_numpy(want))
    a = acc.cpu()
    assert torch.equal(a[:, 0], torch.from_numpy(episodes))
    assert torch.equal(got.sum((1, 2, 3)), n * (a[:, 6] + a[:, 0]))  # steps + 1 cells per agent and episode: the same envs
    assert vec.status() == 0
    vec.close()


def test_counts_past_255_and_the_fold_into_the_base_maps():
    """24 envs of a 5 x 5 map, GAME_STEPS 600, no auto-reset, one group per env.  Steps 511-513 cross k_step's fold of the log into
    the base maps; at step 600 a true count is above 255, where the table and the u8 view differ."""
    E, kw = 24, _fuzz_kwargs(DENSE_SEED, 600, grid=5)
    vec, seeds = _make(E, kw)
    n, g = vec.N_AGENTS, vec.GRID_SIZE
    assert (n, g, int(vec.cfg.game_steps)) == (6, 5, 600)
    refs = _tracked(vec.cfg, seeds)
    groups = torch.arange(E, dtype=torch.int32, device=vec.device)
    acts = _acts(vec)
    t = 0
    for stop in (0, 1, 510, 511, 512, 513, 600):
        while t < stop:
            vec.random_actions(acts, seed=ACT_SEED, step=t)
            vec.step(acts)
            for e, r in refs.items():
                r.step(oracle.philox_actions(n, ACT_SEED, t, e))
            t += 1
        want = np.stack([refs[e].checked() for e in range(E)])
        table = vec.harvest_visitation(_table(vec, E), groups, all_envs=True).cpu()
        assert torch.equal(table, torch.from_numpy(want)), stop
        if stop == 0:
            assert bool((table.sum((2, 3)) == 1).all())  # straight after reset(): the start cells only
        wrapped = (table & 0xFF).to(torch.uint8).numpy()
        for e in range(E):
            assert np.array_equal(wrapped[e], view_arrays(vec.get_state(e), n, g)["visitation"]), (stop, e)
        assert torch.equal(_i64(vec.visitation()).cpu(), table), stop
    assert want.max() > 255, f"no count passed 255: {want.max()}"
    assert vec.status() == 0
    vec.close()


def test_base_maps_handed_in_with_set_state():
    E, k, kw = 4, 2, _fuzz_kwargs(SHORT_SEED, 40, n_agents=8)
    vec, seeds = _make(E, kw)
    n, g = vec.N_AGENTS, vec.GRID_SIZE
    refs = _tracked(vec.cfg, seeds)
    acts = _acts(vec)

    def step(t):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        vec.step(acts)
        for e, r in refs.items():
            r.step(oracle.philox_actions(n, ACT_SEED, t, e))

    for t in range(10):
        step(t)
    view = vec.get_state(k)
    handed = ((np.arange(n * g * g).reshape(n, g * g) * 37 + 5) % 256).astype(np.uint8)
    handed[:, ::3] = 0
    for i in range(n):
        for c in range(g * g):
            view.visitation[i][c] = int(handed[i, c])
    vec.set_state(k, view)
    refs[k].env.set_state(view)
    refs[k].counts[:] = handed.reshape(n, g, g)
    for t in range(10, 13):
        step(t)
    want = np.stack([refs[e].checked() for e in range(E)])
    assert (want[k] >= handed.reshape(n, g, g)).all() and int((want[k] - handed.reshape(n, g, g)).sum()) == 3 * n
    assert torch.equal(_i64(vec.visitation([k])).cpu()[0], torch.from_numpy(want[k]))
    table = vec.harvest_visitation(_table(vec, E), torch.arange(E, dtype=torch.int32, device=vec.device), all_envs=True).cpu()
    assert torch.equal(table, torch.from_numpy(want))  # (row k: the handed-in maps + three steps; the others as they were)
    assert torch.equal(_i64(vec.visitation()).cpu(), table)
    assert vec.status() == 0
    vec.close()


def test_ragged_batch_both_group_layouts_and_a_mask():
    """4 133 arena envs (no multiple of the 32 envs a wave scans), GAME_STEPS 30, 30 steps."""
    E, gs = 4133, 30
    vec, seeds = _make(E, _arena(GAME_STEPS=gs))
    n, g, dev = vec.N_AGENTS, vec.GRID_SIZE, vec.device
    edges = [e for m in range(64, E, 64) for e in (m - 1, m)]
    rest = np.random.default_rng(7).permutation(np.setdiff1d(np.arange(E), [0, E - 1] + edges))
    sample = sorted([0, E - 1] + edges + rest[:256 - 2 - len(edges)].tolist())
    assert len(set(sample)) == 256
    refs = _tracked(vec.cfg, seeds, sample)
    env = torch.arange(E, device=dev)
    acts = _acts(vec)
    for t in range(gs):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        vec.step(acts)
        for e, r in refs.items():
            r.step(oracle.philox_actions(n, ACT_SEED, t, e))
        if t == gs // 2:
            runs = vec.harvest_visitation(_table(vec, 65), (env // 64).to(torch.int32))
            assert not bool(runs.any()), "mid-episode: nothing has ended"
    per_env = vec.visitation()
    assert tuple(per_env.shape) == (E, n, g, g) and per_env.dtype == torch.uint32
    per_env = _i64(per_env)
    want = np.stack([refs[e].checked() for e in sample])
    assert torch.equal(per_env[torch.tensor(sample, device=dev)].cpu(), torch.from_numpy(want))
    assert bool((per_env.sum((2, 3)) == gs + 1).all())

    def reduced(groups, n_groups, take=None):
        idx = env if take is None else take.nonzero().squeeze(1)
        return _table(vec, n_groups).index_add_(0, groups[idx].long(), per_env[idx])

    gen = torch.Generator().manual_seed(5)
    mask = (torch.rand(E, generator=gen) < 0.3).to(torch.uint8).to(dev)
    for groups, n_groups in (((env // 64).to(torch.int32), 65), ((env % 7).to(torch.int32), 7)):
        assert torch.equal(vec.harvest_visitation(_table(vec, n_groups), groups), reduced(groups, n_groups))  # (every env has just ended)
        assert torch.equal(vec.harvest_visitation(_table(vec, n_groups), groups, all_envs=True), reduced(groups, n_groups))
        assert torch.equal(vec.harvest_visitation(_table(vec, n_groups), groups, mask=mask, all_envs=True), reduced(groups, n_groups, mask != 0))
    zeros = torch.zeros(E, dtype=torch.int32, device=dev)
    got = vec.harvest_visitation(_table(vec, 3), mask=mask, all_envs=True)  # no group list: row 0
    assert torch.equal(got[:1], reduced(zeros, 1, mask != 0)) and not bool(got[1:].any())
    assert torch.equal(vec.harvest_visitation(_table(vec, 1), all_envs=True), reduced(zeros, 1))
    assert vec.status() == 0
    vec.close()


def test_the_largest_accepted_shape():
    """N = 16, G = 32: the maps of one env are 64 KiB of u32, twice the LDS histogram — the kernel tiles over agents."""
    E, kw = 8, _largest_kwargs()
    vec, seeds = _make(E, kw)
    n, g = vec.N_AGENTS, vec.GRID_SIZE
    assert (n, g) == (abi.MAX_AGENTS, abi.MAX_GRID) and vec.visitation_words == 16 * 1024
    refs = _tracked(vec.cfg, seeds)
    acts = _acts(vec)
    for t in range(20):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        vec.step(acts)
        for e, r in refs.items():
            r.step(oracle.philox_actions(n, ACT_SEED, t, e))
    want = np.stack([refs[e].checked() for e in range(E)])
    assert torch.equal(_i64(vec.visitation()).cpu(), torch.from_numpy(want))
    groups_h = np.array([0, 0, 0, 1, 1, 0, 1, 1])
    table = vec.harvest_visitation(_table(vec, 2), torch.from_numpy(groups_h.astype(np.int32)).to(vec.device), all_envs=True).cpu()
    assert torch.equal(table, torch.from_numpy(np.stack([want[groups_h == k].sum(0) for k in range(2)])))
    assert bool((table.sum((2, 3)) == 4 * 21).all())
    assert vec.status() == 0
    vec.close()


def test_bad_ids_skip_their_records_and_write_nothing_outside():
    E, G, POISON, POISON32 = 256, 4, 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
    vec, _ = _make(E, _arena())
    n, g, dev = vec.N_AGENTS, vec.GRID_SIZE, vec.device
    acts = _acts(vec)
    for t in range(30):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        vec.step(acts)
    per_env = _i64(vec.visitation())
    groups = (torch.arange(E, device=dev) % G).to(torch.int32)
    groups[7], groups[100] = -1, G
    big = torch.full((G + 8, n, g, g), POISON, dtype=torch.int64, device=dev)
    acc = big[4:4 + G]
    acc.zero_()
    vec.harvest_visitation(acc, groups, all_envs=True)
    assert vec.status() == abi.ST_BAD_GROUP
    good = torch.ones(E, dtype=torch.bool, device=dev)
    good[7] = good[100] = False
    idx = good.nonzero().squeeze(1)
    assert torch.equal(acc, _table(vec, G).index_add_(0, groups[idx].long(), per_env[idx]))
    assert bool((big[:4] == POISON).all()) and bool((big[4 + G:] == POISON).all())
    assert vec.status() == 0
    # the export: records 1 and 3 name no env
    ids = torch.tensor([3, -1, 5, E, 3], dtype=torch.int32, device=dev)
    big32 = torch.full((len(ids) + 4, n, g, g), POISON32, dtype=torch.int32, device=dev)
    out = big32[2:2 + len(ids)].view(torch.uint32)
    assert vec.visitation(ids, out=out) is out
    assert vec.status() == abi.ST_BAD_GROUP
    got = big32[2:2 + len(ids)].long()
    assert torch.equal(got[0], per_env[3]) and torch.equal(got[2], per_env[5]) and torch.equal(got[4], per_env[3])
    assert bool((got[1] == POISON32).all()) and bool((got[3] == POISON32).all())
    assert bool((big32[:2] == POISON32).all()) and bool((big32[2 + len(ids):] == POISON32).all())
    assert vec.status() == 0
    vec.close()


def test_both_calls_leave_env_state_alone():
    E = 2048
    vec, _ = _make(E, _arena(GAME_STEPS=30))
    acts = _acts(vec)
    for t in range(30):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        vec.step(acts)
    before = vec.save_states()
    h = pkg.EpisodeHarvest(vec, 3, np.arange(E) % 3, visitation=True)
    h.update()
    per_env = vec.visitation()
    assert int(h.table()[:, 0].sum()) == E and int(h.visitation_table().sum()) == E * vec.N_AGENTS * 31 == int(_i64(per_env).sum())
    assert torch.equal(vec.save_states(), before)
    assert vec.status() == 0
    vec.close()


def test_step_observe_and_both_harvests_replayed_from_a_graph():
    """step_observe(auto_reset) + harvest + harvest_visitation captured once on a side stream, replayed 60 times, against 60
    direct calls on a twin."""
    import bench

    E, G, kw = 192, 3, _arena(GAME_STEPS=50)
    (a, _), (b, _) = _make(E, kw), _make(E, kw)
    dev = a.device
    groups = (torch.arange(E, device=dev) % G).to(torch.int32)
    for v in (a, b):
        v.observe()
        bench.stagger_phases(v, torch, 0, 50)
    acts = _acts(a)
    acc_a = torch.zeros((G, a.harvest_words), dtype=torch.int64, device=dev)
    acc_b = torch.zeros_like(acc_a)
    vis_a, vis_b = _table(a, G), _table(b, G)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph, stream=side):  # capture only: nothing runs
        a.step_observe(acts, auto_reset=True)
        a.harvest(acc_a, groups)
        a.harvest_visitation(vis_a, groups)
    torch.cuda.synchronize(dev)
    assert not bool(acc_a.any()) and not bool(vis_a.any())
    for t in range(60):
        a.random_actions(acts, seed=ACT_SEED, step=t)
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        b.step_observe(acts, auto_reset=True)
        b.harvest(acc_b, groups)
        b.harvest_visitation(vis_b, groups)
    torch.cuda.synchronize(dev)
    assert int(acc_b[:, 0].sum()) >= E and torch.equal(acc_a, acc_b)
    assert torch.equal(vis_a, vis_b) and torch.equal(vis_b.sum((1, 2, 3)), a.N_AGENTS * (acc_b[:, 6] + acc_b[:, 0]))
    assert a.status() == 0 and b.status() == 0
    a.close(), b.close()


def test_argument_errors_raise_before_any_launch():
    E = 64
    vec, _ = _make(E, _arena())
    dev, n, g = vec.device, vec.N_AGENTS, vec.GRID_SIZE
    acc = _table(vec, 2)
    groups = torch.zeros(E, dtype=torch.int32, device=dev)
    mask = torch.ones(E, dtype=torch.uint8, device=dev)
    bad_acc = [torch.zeros((0, n, g, g), dtype=torch.int64, device=dev), acc.to(torch.int32), acc.cpu(), acc.reshape(2, n, g * g),
               torch.zeros((2, n, g, g + 1), dtype=torch.int64, device=dev), torch.zeros((2, n + 1, g, g), dtype=torch.int64, device=dev),
               acc.reshape(-1), torch.zeros((2, n, g, 2 * g), dtype=torch.int64, device=dev)[..., ::2], acc.cpu().numpy()]
    for x in bad_acc:
        with pytest.raises(ValueError):
            vec.harvest_visitation(x, groups, mask)
    for x in (groups.long(), groups.cpu(), groups[:-1], torch.zeros(2 * E, dtype=torch.int32, device=dev)[::2]):
        with pytest.raises(ValueError):
            vec.harvest_visitation(acc, x, mask)
    for x in (mask.to(torch.bool), mask.cpu(), mask[:-1], mask.to(torch.int32)):
        with pytest.raises(ValueError):
            vec.harvest_visitation(acc, groups, x)
    out = torch.zeros((3, n, g, g), dtype=torch.int32, device=dev).view(torch.uint32)
    for x in (torch.zeros(3, device=dev), torch.zeros((3, 1), dtype=torch.int32, device=dev), [0, 1, E], [0, -1, 2], np.zeros(3, np.float32)):
        with pytest.raises(ValueError):
            vec.visitation(x, out=out)
    bad_out = [out.view(torch.int32), out.cpu(), out[:2], out.reshape(3, n, g * g), out.reshape(-1),
               torch.zeros((3, n, g, 2 * g), dtype=torch.int32, device=dev).view(torch.uint32)[..., ::2]]
    for x in bad_out:
        with pytest.raises(ValueError):
            vec.visitation([0, 1, 2], out=x)
    with pytest.raises(ValueError):
        vec.visitation(out=out)  # (every env: E records)
    lib, ptr = vec._lib, lambda t: t.data_ptr()
    for n_groups, table, flags in ((0, ptr(acc), 0), (2, None, 0), (2, ptr(acc) + 4, 0), (2, ptr(acc), 2)):  # the C ABI's own checks
        assert lib.ctf_harvest_visitation(vec._h, None, n_groups, None, flags, table, None) == -1 and b"ctf_harvest_visitation" in lib.ctf_last_error()
    assert lib.ctf_harvest_visitation(None, None, 2, None, 0, ptr(acc), None) == -1
    for cnt, ids in ((-1, None), (E + 1, None)):
        assert lib.ctf_export_visitation(vec._h, ids, cnt, ptr(out), None) == -1 and b"ctf_export_visitation" in lib.ctf_last_error()
    bare, _ = _make(E, _arena(), log_metrics=False)  # keeps no maps
    assert lib.ctf_harvest_visitation(bare._h, None, 2, None, 0, ptr(acc), None) == -1 and b"ctf_harvest_visitation" in lib.ctf_last_error()
    assert lib.ctf_export_visitation(bare._h, None, 3, ptr(out), None) == -1 and b"ctf_export_visitation" in lib.ctf_last_error()
    with pytest.raises(ValueError):
        bare.harvest_visitation(acc, groups, mask)
    with pytest.raises(ValueError):
        bare.visitation([0, 1, 2], out=out)
    torch.cuda.synchronize()
    assert not bool(acc.any()) and not bool(out.view(torch.int32).any()) and vec.status() == 0 and bare.status() == 0
    bare.close()
    vec.close()


def test_tournament_maps_equal_the_single_pairing_duels():
    A, B, per = 2, 3, 64
    kw = dict(pkg.configs.SPLIT_KWARGS, SCENARIO=pkg.CtfScenarios.arrow)
    seeds = np.arange(A * B * per, dtype=np.uint64) * 31 + 5
    agents, opponents = [StubDuelPolicy(3), StubDuelPolicy(8)], [StubDuelPolicy(5), StubDuelPolicy(13), StubDuelPolicy(21)]
    vec = pkg.VecGridworldCtf(A * B * per, device=0, py_seeds=seeds, np_seeds=seeds, tune_placement=False, **kw)
    n, g = vec.N_AGENTS, vec.GRID_SIZE
    out = pkg.batched_tournament(vec, agents, opponents, visitation=True)
    assert vec.status() == 0
    assert out["visitation"].shape == (A, B, n, g, g) and out["visitation"].dtype == np.int64
    assert (out["visitation"].sum((2, 3, 4)) == per * n * (out["steps"] + 1)).all()
    assert "visitation" not in pkg.batched_tournament(vec, agents, opponents, max_steps=2)
    vec.close()
    for a in range(A):
        for b in range(B):
            k = a * B + b
            s = seeds[k * per:(k + 1) * per]
            one = pkg.VecGridworldCtf(per, device=0, py_seeds=s, np_seeds=s, tune_placement=False, **kw)
            d = pkg.batched_duel(one, agents[a], opponents[b], visitation=True)
            assert tuple(d["visitation"].shape) == (per, n, g, g) and d["visitation"].dtype == torch.uint32
            assert np.array_equal(out["visitation"][a, b], _i64(d["visitation"]).sum(0).cpu().numpy()), (a, b)
            if k == 0:
                assert "visitation" not in pkg.batched_duel(one, agents[a], opponents[b], max_steps=2)
            one.close()
    assert len({out["visitation"][a, b].tobytes() for a in range(A) for b in range(B)}) > 1  # (the pairings do differ)

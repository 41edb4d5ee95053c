"""The episode harvest on the device (ctf_harvest_episodes, VecGridworldCtf.harvest, harvest.EpisodeHarvest,
duel.batched_tournament): the table it builds equals, word for word, the sums over the CPU oracle's envs read just before they reset
(small, staggered, auto-reset and not) and the torch reduction of ``counters()`` at full size in both regimes — a few envs ending
per step, and a lockstep batch ending at once — for group ids in runs and alternating.  Integer sums: every comparison is exact."""
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
SHORT_SEED = 3         # of the short-episode config (chosen on the CPU with the oracle alone: _check_inputs holds)


def _arena(**over):
    return dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii, **over)


def _short_kwargs():
    """A capture-dense 4 v 4 map in the style of the committed fuzz fixtures (make_golden_fuzz.random_scenario), GAME_STEPS 40."""
    import make_golden_fuzz as mgf

    rng = np.random.default_rng(SHORT_SEED)
    while True:
        scen, agents = mgf.random_scenario(rng, "Harvest")
        if len(agents) == 8:
            break
    return dict(GRID_SIZE=scen["GRID_SIZE"], AGENT_CONFIG=agents, GAME_STEPS=40, MAP_SYMMETRY_CHECK=False, HOME_FLAG_CAPTURE=False,
                DROP_FLAG_WHEN_NO_HP=True, USE_ADJUSTED_REWARDS=True, TAG_PROBABILITY=0.5, AGENT_TYPE_HP={0: 10, 1: 8, 2: 8, 3: 7},
                AGENT_TYPE_DAMAGE={0: 1, 1: 0.5, 2: 0.5, 3: 1}, GUARDIAN_DAMAGE_MULTIPLIER=5.0, VAULT_HP_COST=1.25, SCENARIO=scen)


def _make(n_envs, kw, seed_base=11, log_metrics=True):
    seeds = np.arange(n_envs, dtype=np.uint64) * 7919 + seed_base
    return pkg.VecGridworldCtf(n_envs, device=0, py_seeds=seeds, np_seeds=seeds, log_metrics=log_metrics, tune_placement=False, **kw), seeds


def _row(view, n, g):
    """one env's contribution to its group's row, from a state view"""
    s = view_arrays(view, n, g)
    c0, c1 = s["team_captures"]
    return np.concatenate([np.array([1, c0 > c1, c0 == c1, c0 < c1, c0, c1, s["step_count"], 0], np.int64), s["metrics"].reshape(-1).astype(np.int64)])


def _reduce(vec, groups, n_groups, take=None, all_envs=False):
    """today's route: counters() of ALL envs, reduced in torch to the harvest's table"""
    met, caps, steps = vec.counters()
    if not all_envs:
        ended = (vec.done != 0) & (steps == int(vec.cfg.game_steps))
        take = ended if take is None else take & ended
    elif take is None:
        take = torch.ones_like(steps, dtype=torch.bool)
    idx = take.nonzero().squeeze(1)
    c = caps[idx].long()
    rows = torch.cat([torch.ones_like(c[:, :1]), (c[:, :1] > c[:, 1:]).long(), (c[:, :1] == c[:, 1:]).long(), (c[:, :1] < c[:, 1:]).long(), c,
                      steps[idx].long()[:, None], torch.zeros_like(c[:, :1]), met[idx].reshape(idx.numel(), -1).long()], dim=1)
    out = torch.zeros((n_groups, vec.harvest_words), dtype=torch.int64, device=vec.device)
    out.index_add_(0, groups[idx].long(), rows)
    return out


def _oracles(cfg, seeds):
    refs = [oracle.OracleEnv(cfg) for _ in seeds]
    for r, s in zip(refs, seeds):
        r.seed(int(s), int(s))
    return refs


def _check_inputs(table):
    assert (table[:, 0] >= 2).all(), f"a group finished fewer than 2 episodes: {table[:, 0]}"
    assert table[:, 1].sum() > 0 and table[:, 2].sum() > 0 and table[:, 3].sum() > 0, f"wins / draws / losses: {table[:, 1:4].sum(0)}"


def test_staggered_auto_reset_run_equals_the_oracle():
    """96 envs of the short-episode config, phases staggered as bench.stagger_phases does it (period = GAME_STEPS), 5 groups by a
    fixed permutation, 130 step(auto_reset) + harvest calls.  Expected: the oracle envs' states read just before they reset."""
    import bench

    E, G, steps, kw = 96, 5, 130, _short_kwargs()
    vec, seeds = _make(E, kw)
    n, g, gs = vec.N_AGENTS, vec.GRID_SIZE, int(vec.cfg.game_steps)
    assert (n, gs) == (8, 40)
    refs = _oracles(vec.cfg, seeds)
    groups_h = np.random.default_rng(1).permutation(E) % G
    groups = torch.from_numpy(groups_h.astype(np.int32)).to(vec.device)
    bench.stagger_phases(vec, torch, 0, gs)
    for s in range(gs):  # the same steps and resets on the CPU
        for e, r in enumerate(refs):
            if r.get_state().done:
                r.reset()
            r.step(oracle.philox_actions(n, STAGGER_SEED, s, e))
            if e % gs == s:
                r.reset()
    acts = torch.empty((E, n), dtype=torch.int8, device=vec.device)
    acc = torch.zeros((G, vec.harvest_words), dtype=torch.int64, device=vec.device)
    want = np.zeros((G, vec.harvest_words), np.int64)
    for t in range(steps):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        vec.step(acts, auto_reset=True)
        vec.harvest(acc, groups)
        for e, r in enumerate(refs):
            if r.get_state().done:
                r.reset()
            _, done, status = r.step(oracle.philox_actions(n, ACT_SEED, t, e))
            assert status == 0
            if done:
                v = r.get_state()
                assert v.step_count == gs
                want[groups_h[e]] += _row(v, n, g)
    _check_inputs(want)
    assert want[:, 8:].any()
    assert torch.equal(acc.cpu(), torch.from_numpy(want))
    assert vec.status() == 0
    vec.close()


def test_without_auto_reset_every_env_is_counted_exactly_once():
    E, G, kw = 96, 5, _short_kwargs()
    vec, seeds = _make(E, kw)
    n, g, gs = vec.N_AGENTS, vec.GRID_SIZE, int(vec.cfg.game_steps)
    refs = _oracles(vec.cfg, seeds)
    groups_h = np.random.default_rng(1).permutation(E) % G
    h = pkg.EpisodeHarvest(vec, G, groups_h)
    acts = torch.empty((E, n), dtype=torch.int8, device=vec.device)
    for t in range(3 * gs):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        vec.step(acts)
        h.update()
    want = np.zeros((G, vec.harvest_words), np.int64)
    for e, r in enumerate(refs):
        for t in range(gs):
            r.step(oracle.philox_actions(n, ACT_SEED, t, e))
        assert r.get_state().done
        want[groups_h[e]] += _row(r.get_state(), n, g)
    got = h.table()
    assert got[:, 0].sum() == E and got[:, 6].sum() == E * gs
    assert np.array_equal(got, want)
    assert sum(h.results(k, got)["episodes"] for k in range(G)) == E
    assert h.metrics(0, got)["team_flag_captures"] == {0: int(want[0, 4]), 1: int(want[0, 5])}
    assert vec.status() == 0
    vec.close()


@pytest.mark.parametrize("assignment,one_launch", [("runs", "0"), ("alternating", "0"), ("runs", "1")])
def test_full_size_sparse_and_dense_equal_the_reduction_of_counters(assignment, one_launch, monkeypatch):
    """65 536 arena envs, 64 groups.  Sparse: staggered with bench.stagger_phases, 40 step_observe(auto_reset) + harvest, ~131
    envs ending per step.  Dense: a lockstep batch stepped through GAME_STEPS, all envs ending in the last step."""
    import bench

    E, G = 65536, 64
    vec, _ = _make(E, _arena())
    monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", one_launch)
    assert vec.step_observe_launches() == (1 if one_launch == "1" else 2)
    gs, dev = int(vec.cfg.game_steps), vec.device
    env = torch.arange(E, device=dev)
    groups = (env // (E // G) if assignment == "runs" else env % G).to(torch.int32)
    acts = torch.empty((E, vec.N_AGENTS), dtype=torch.int8, device=dev)
    acc = torch.zeros((G, vec.harvest_words), dtype=torch.int64, device=dev)
    want = torch.zeros_like(acc)
    vec.observe()
    bench.stagger_phases(vec, torch, 0, gs)
    for t in range(40):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        vec.step_observe(acts, auto_reset=True)
        vec.harvest(acc, groups)
        want += _reduce(vec, groups, G)
    assert int(want[:, 0].sum()) == sum(len(range(t, E, gs)) for t in range(40))  # env e ends at step e % GAME_STEPS
    assert torch.equal(acc, want), "sparse"
    vec.reset()
    acc.zero_()
    for t in range(gs):
        vec.random_actions(acts, seed=ACT_SEED + 1, step=t)
        if t < gs - 1:
            vec.step(acts, auto_reset=True)
        else:
            vec.step_observe(acts, auto_reset=True)
        vec.harvest(acc, groups)
        if t == gs - 2:
            assert not bool(acc.any()), "an episode was harvested before its last step"
    want = _reduce(vec, groups, G)
    assert int(want[:, 0].sum()) == E and bool((want[:, 0] == E // G).all())
    assert torch.equal(acc, want), "dense"
    assert vec.status() == 0
    vec.close()
    torch.cuda.empty_cache()


def test_harvest_all_with_and_without_a_mask_and_without_metrics():
    E, G = 4096, 7
    for log_metrics in (True, False):
        vec, _ = _make(E, _arena(), log_metrics=log_metrics)
        dev = vec.device
        gen = torch.Generator().manual_seed(5)
        groups = torch.randint(0, G, (E,), generator=gen).to(torch.int32).to(dev)
        mask = (torch.rand(E, generator=gen) < 0.3).to(torch.uint8).to(dev)
        acts = torch.empty((E, vec.N_AGENTS), dtype=torch.int8, device=dev)
        for t in range(37):
            vec.random_actions(acts, seed=ACT_SEED, step=t)
            vec.step(acts)
        acc = torch.zeros((G, vec.harvest_words), dtype=torch.int64, device=dev)
        vec.harvest(acc, groups)
        assert not bool(acc.any()), "mid-episode: nothing has ended"
        vec.harvest(acc, groups, all_envs=True)
        want = _reduce(vec, groups, G, all_envs=True)
        assert torch.equal(acc, want) and int(acc[:, 0].sum()) == E and int(acc[:, 6].sum()) == 37 * E
        assert bool(acc[:, 8:].any()) == log_metrics  # (log_metrics off: words 0-6 counted, the counter words untouched)
        acc.zero_()
        vec.harvest(acc, groups, mask=mask, all_envs=True)
        assert torch.equal(acc, _reduce(vec, groups, G, take=mask != 0, all_envs=True)) and int(acc[:, 0].sum()) == int(mask.sum())
        acc.zero_()
        vec.harvest(acc, mask=mask, all_envs=True)  # no group list: row 0
        assert torch.equal(acc[:1], _reduce(vec, torch.zeros_like(groups), 1, take=mask != 0, all_envs=True)) and not bool(acc[1:].any())
        assert vec.status() == 0
        vec.close()


def test_a_bad_group_id_skips_its_env_and_writes_nothing_outside_the_table():
    E, G, POISON = 256, 4, 0x5A5A5A5A5A5A5A5A
    vec, _ = _make(E, _arena())
    dev = vec.device
    acts = torch.empty((E, vec.N_AGENTS), dtype=torch.int8, device=dev)
    for t in range(30):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        vec.step(acts)
    groups = (torch.arange(E, device=dev) % G).to(torch.int32)
    groups[7], groups[100] = -1, G
    big = torch.full((G + 8, vec.harvest_words), POISON, dtype=torch.int64, device=dev)
    acc = big[4:4 + G]
    acc.zero_()
    vec.harvest(acc, groups, all_envs=True)
    assert vec.status() == abi.ST_BAD_GROUP
    good = torch.ones(E, dtype=torch.bool, device=dev)
    good[7] = good[100] = False
    assert torch.equal(acc, _reduce(vec, groups.clamp(0, G - 1), G, take=good, all_envs=True)) and int(acc[:, 0].sum()) == E - 2
    assert bool((big[:4] == POISON).all()) and bool((big[4 + G:] == POISON).all())
    assert vec.status() == 0
    vec.close()


def test_the_harvest_leaves_env_state_alone():
    E = 2048
    vec, _ = _make(E, _arena(GAME_STEPS=30))
    acts = torch.empty((E, vec.N_AGENTS), dtype=torch.int8, device=vec.device)
    for t in range(30):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        vec.step(acts)
    before = vec.save_states()
    h = pkg.EpisodeHarvest(vec, 3, np.arange(E) % 3)
    h.update()
    assert int(h.table()[:, 0].sum()) == E
    assert torch.equal(vec.save_states(), before)
    vec.close()


def test_step_observe_and_harvest_replayed_from_a_graph():
    """step_observe(auto_reset) + harvest captured once on a side stream, replayed 60 times, against 60 direct calls on a twin."""
    import bench

    E, G, kw = 192, 3, _arena(GAME_STEPS=50)
    (a, _), (b, _) = _make(E, kw), _make(E, kw)
    dev = a.device
    groups = (torch.arange(E, device=dev) % G).to(torch.int32)
    for v in (a, b):
        v.observe()
        bench.stagger_phases(v, torch, 0, 50)
    acts = torch.empty((E, a.N_AGENTS), dtype=torch.int8, device=dev)
    acc_a = torch.zeros((G, a.harvest_words), dtype=torch.int64, device=dev)
    acc_b = torch.zeros_like(acc_a)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph, stream=side):  # capture only: nothing runs
        a.step_observe(acts, auto_reset=True)
        a.harvest(acc_a, groups)
    torch.cuda.synchronize(dev)
    assert not bool(acc_a.any())
    for t in range(60):
        a.random_actions(acts, seed=ACT_SEED, step=t)
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        b.step_observe(acts, auto_reset=True)
        b.harvest(acc_b, groups)
    torch.cuda.synchronize(dev)
    assert int(acc_b[:, 0].sum()) >= E and torch.equal(acc_a, acc_b)
    assert torch.equal(a.obs, b.obs) and all(torch.equal(x, y) for x, y in zip(a.counters(), b.counters()))
    assert a.status() == 0 and b.status() == 0
    a.close(), b.close()


def test_argument_errors_raise_before_any_launch():
    E = 64
    vec, _ = _make(E, _arena())
    dev, H = vec.device, vec.harvest_words
    assert H == 8 + 13 * vec.N_AGENTS
    acc = torch.zeros((2, H), dtype=torch.int64, device=dev)
    groups = torch.zeros(E, dtype=torch.int32, device=dev)
    mask = torch.ones(E, dtype=torch.uint8, device=dev)
    bad_acc = [torch.zeros((0, H), dtype=torch.int64, device=dev), acc.to(torch.int32), acc.cpu(), torch.zeros((2, H + 1), dtype=torch.int64, device=dev),
               acc.reshape(-1), torch.zeros((2, 2 * H), dtype=torch.int64, device=dev)[:, ::2], acc.cpu().numpy()]
    for x in bad_acc:
        with pytest.raises(ValueError):
            vec.harvest(x, groups, mask)
    for x in (groups.long(), groups.cpu(), groups[:-1], torch.zeros(2 * E, dtype=torch.int32, device=dev)[::2]):
        with pytest.raises(ValueError):
            vec.harvest(acc, x, mask)
    for x in (mask.to(torch.bool), mask.cpu(), mask[:-1], mask.to(torch.int32)):
        with pytest.raises(ValueError):
            vec.harvest(acc, groups, x)
    with pytest.raises(ValueError):
        pkg.EpisodeHarvest(vec, 0)
    lib, ptr = vec._lib, lambda t: t.data_ptr()
    for n_groups, table in ((0, ptr(acc)), (2, None), (2, ptr(acc) + 4)):  # the C ABI's own checks
        assert lib.ctf_harvest_episodes(vec._h, None, n_groups, None, 0, table, None) == -1 and b"ctf_harvest_episodes" in lib.ctf_last_error()
    torch.cuda.synchronize()
    assert not bool(acc.any()) and vec.status() == 0
    vec.close()


def test_tournament_rows_equal_the_single_pairing_duels():
    A, B, per = 2, 3, 64
    kw = dict(pkg.configs.SPLIT_KWARGS, SCENARIO=pkg.CtfScenarios.arrow)
    seeds = np.arange(A * B * per, dtype=np.uint64) * 31 + 5
    agents, opponents = [StubDuelPolicy(3), StubDuelPolicy(8)], [StubDuelPolicy(5), StubDuelPolicy(13), StubDuelPolicy(21)]
    vec = pkg.VecGridworldCtf(A * B * per, device=0, py_seeds=seeds, np_seeds=seeds, tune_placement=False, **kw)
    out = pkg.batched_tournament(vec, agents, opponents)
    assert vec.status() == 0
    vec.close()
    assert out["table"].shape == (A * B, 8 + 13 * 4) and out["steps"] == 257
    assert out["result_counts"].shape == (A, B, 3) and (out["result_counts"].sum(-1) == per).all() and (out["episodes"] == per).all()
    assert np.array_equal(out["win_rate"], out["result_counts"][:, :, 0] / per)
    for a in range(A):
        for b in range(B):
            k = a * B + b
            s = seeds[k * per:(k + 1) * per]
            one = pkg.VecGridworldCtf(per, device=0, py_seeds=s, np_seeds=s, tune_placement=False, **kw)
            d = pkg.batched_duel(one, agents[a], opponents[b])
            _, _, steps = one.counters()
            caps, res = d["team_flag_captures"].long(), d["result"].long()
            want = torch.cat([torch.tensor([per, int((res > 0).sum()), int((res == 0).sum()), int((res < 0).sum())], device=caps.device),
                              caps.sum(0), steps.long().sum()[None], torch.zeros(1, dtype=torch.int64, device=caps.device),
                              d["metrics"].long().sum(0).reshape(-1)])
            assert np.array_equal(out["table"][k], want.cpu().numpy()), (a, b)
            one.close()
    assert out["table"][:, 8:].any() and len({tuple(r) for r in out["table"]}) > 1  # (the pairings do differ)

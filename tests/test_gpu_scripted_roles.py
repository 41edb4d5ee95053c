"""k_scripted_roles (ctf_scripted_roles, VecGridworldCtf.scripted_roles, scripted.ScriptedTeam) on the device: its actions must equal
the queue BFS and the sets of tests/_scripted_roles_ref.py byte for byte — on played states of three grid sizes under every mask and
several role packs, with the bytes it was not asked for and the rows either side of the buffer untouched; on the planted scenes of
tests/_scripted_roles_cases.py; with a scene's edge rows against the next env's in one wave; across two shards; without touching the
env; refused arguments; inside a captured graph; and as the opponent of the collectors.  The behavioural condition was asserted on
the restatement and the oracle first (tests/test_scripted_roles_cpu.py), with the same seeds."""
import importlib

import numpy as np
import pytest

import _scripted_cases as sc
import _scripted_roles_cases as rc
import _scripted_roles_ref as rr
from _cases import abi, pkg
from _stub_policy import StubPolicy
from test_gpu_scripted import E, SENTINEL, _arena, _big_kwargs, _final, _guarded, _host_states, _play, _vec
from test_scripted_roles_cpu import check_what_the_scenes_show

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
rollout = importlib.import_module("marl-ctf-development_amd.rollout")
duel = importlib.import_module("marl-ctf-development_amd.duel")
scripted = importlib.import_module("marl-ctf-development_amd.scripted")

NAMES = {v: k for k, v in abi.SCRIPT_ROLES.items()}


def _names(roles):
    return [NAMES[r] for r in roles]


def _ref_full(vec, roles, **kw):
    """the restatement for every agent of every env -> int8 [E, N]"""
    st = _host_states(vec)
    env_offset = kw.pop("env_offset", 0)
    out = np.zeros((vec.n_envs, vec.N_AGENTS), np.int8)
    for e in range(vec.n_envs):
        rr.state_roles(vec.cfg, {k: v[e] for k, v in st.items()}, sc.all_mask(vec.cfg), roles, env=env_offset + e, out=out[e], **kw)
    return out


def _expect(want, mask, n_rows):
    """the guarded buffer after a call for ``mask``: the sentinel everywhere but the asked agents' bytes of the inner rows"""
    n = want.shape[1]
    sel = np.array([(mask >> i) & 1 for i in range(n)], bool)
    exp = np.full((n_rows + 2, n), SENTINEL, np.int8)
    exp[1:n_rows + 1][:, sel] = want[:, sel]
    return exp


@pytest.mark.parametrize("name", ("arena", "grid7", "grid32"))
def test_every_mask_and_several_role_packs_on_played_states(name):
    kw = {"arena": _arena(GAME_STEPS=40), "grid7": sc.planted_scenes()["row0_7"][0], "grid32": _big_kwargs()}[name]
    vec = _vec(kw)
    n = vec.N_AGENTS
    assert vec.GRID_SIZE == {"arena": 15, "grid7": 7, "grid32": 32}[name] and (name != "grid32" or n == 16)
    _play(vec, 33)  # different seeds: the envs are at different states, some past an episode's end
    rng = np.random.default_rng(0x9A7D)
    packs = [rc.random_roles(rng, n), [rr.CHASER] * n, [rr.GUARD] * n]
    masks = [1 << i for i in range(n)] + sc.team_masks(vec.cfg) + [sc.all_mask(vec.cfg), 0]
    for roles in packs:
        want = _ref_full(vec, roles)
        assert len({w.tobytes() for w in want}) > 8  # desynchronised
        for m in masks:
            buf, out = _guarded(vec)
            got = vec.scripted_roles(_names(roles), agent_mask=m, out=out)
            assert got is out
            assert np.array_equal(buf.cpu().numpy(), _expect(want, m, E)), f"roles {roles}, mask 0x{m:x}"
    # team= names the same agents as the team's mask; a dict names the agents that do not run
    roles = packs[0]
    for t in (0, 1):
        assert torch.equal(vec.scripted_roles(_names(roles), team=t, out=_guarded(vec)[1]),
                           vec.scripted_roles({i: NAMES[r] for i, r in enumerate(roles) if r}, agent_mask=sc.team_masks(vec.cfg)[t], out=_guarded(vec)[1]))
    # with exploration: every epsilon of the rule
    lib, ptr = vec._lib, abi.ptr
    for eps, (step, off) in zip(sc.EPSILONS, ((0, 0), (499, 3), ((1 << 32) - 1, 65536), (7, 1))):
        buf, out = _guarded(vec)
        assert lib.ctf_scripted_roles(vec._h, ptr(out), sc.all_mask(vec.cfg), rr.role_pack(roles), eps, 0xDEADBEEF12345678, step, off, vec._stream()) == 0
        exp = _ref_full(vec, roles, epsilon_q32=eps, seed=0xDEADBEEF12345678, step=step, env_offset=off)
        assert np.array_equal(buf.cpu().numpy(), _expect(exp, sc.all_mask(vec.cfg), E)), (eps, step, off)
    assert name != "arena" or vec.status() == 0
    vec.close()


def _plant(vec, cfg, planted, envs):
    st = vec.get_states()
    for e in envs:
        st["grid"][e] = torch.from_numpy(planted["grid"]).to(vec.device)
        st["has_flag"][e] = torch.from_numpy(planted["has_flag"]).to(vec.device)
    st.pop("metrics", None)
    vec.set_states(st)
    assert vec.status() == 0


def _planted(name):
    kw, edits, roles = rc.scenes()[name]
    cfg, derived = sc.build(kw)
    return kw, cfg, sc.planted_state(cfg, derived, edits), roles


@pytest.fixture(scope="module")
def shown():
    """name -> the device's actions for every agent of the planted env, gathered by the scene tests"""
    return {}


@pytest.mark.parametrize("name", sorted(rc.scenes()))
def test_planted_scenes_through_set_states(name, shown):
    kw, cfg, planted, roles = _planted(name)
    vec = _vec(kw, n_envs=3)
    _plant(vec, cfg, planted, (1,))
    want = _ref_full(vec, roles)
    assert np.array_equal(want[1], rr.state_roles(cfg, planted, sc.all_mask(cfg), roles))  # env 1 holds the planted state
    for m in rc.masks(cfg):
        buf, out = _guarded(vec)
        vec.scripted_roles(_names(roles), agent_mask=m, out=out)
        assert np.array_equal(buf.cpu().numpy(), _expect(want, m, 3)), f"mask 0x{m:x}"
    shown[name] = vec.scripted_roles(_names(roles), agent_mask=sc.all_mask(cfg)).cpu().numpy()[1].tolist()
    vec.close()


def test_what_the_planted_scenes_show(shown):
    assert sorted(shown) == sorted(rc.scenes())  # (runs behind the scene tests, in file order)
    check_what_the_scenes_show(shown)


@pytest.mark.parametrize("g", (16, 32))
def test_group_edges(g):
    """The edges scene in ADJACENT envs with one team asked: consecutive groups of a wave are consecutive envs (four with W = 16,
    two with W = 32), so row g - 1 of one env lies one lane from row 0 of the next.  The scene has an opponent in row g - 1 with a
    chaser in row 0 of the same column and the reverse: a dilation or a frontier that ran over a group's edge would change an
    action."""
    kw, cfg, planted, roles = _planted(f"edges{g}")
    vec = _vec(kw, n_envs=4)
    _plant(vec, cfg, planted, (1, 2))
    st = _host_states(vec)
    for e in (1, 2):
        assert all(np.array_equal(st[k][e], planted[k]) for k in ("grid", "pos", "has_flag"))
    teams, _ = rr.cfg_teams_flags(cfg)
    opp = [tuple(int(v) for v in planted["pos"][j]) for j in range(cfg.n_agents) if teams[j] == 1]
    mine = [tuple(int(v) for v in planted["pos"][j]) for j in (0, 2)]
    assert (g - 1, mine[0][1]) in opp and mine[0][0] == 0 and (0, mine[1][1]) in opp and mine[1][0] == g - 1
    want = _ref_full(vec, roles)
    assert want[1][0] != 4 and want[1][2] != 4 and want[2][0] != 4 and want[2][2] != 4
    for t in (0, 1):
        buf, out = _guarded(vec)
        vec.scripted_roles(_names(roles), team=t, out=out)
        assert np.array_equal(buf.cpu().numpy(), _expect(want, sc.team_masks(cfg)[t], 4)), t
    vec.close()


def test_an_all_runner_pack_is_ctf_scripted_actions():
    vec = _vec(_arena(GAME_STEPS=40))
    _play(vec, 33)
    n = vec.N_AGENTS
    lib, ptr = vec._lib, abi.ptr
    rng = np.random.default_rng(5)
    for m in [sc.all_mask(vec.cfg)] + sc.team_masks(vec.cfg) + [1 << (n - 1)]:
        # the roles of agents that are not asked do not count: any pack whose ASKED agents all run
        pack = rr.role_pack([0 if (m >> i) & 1 else int(rng.integers(0, 3)) for i in range(n)])
        for eps in (0, 1 << 31):
            (b1, o1), (b2, o2) = _guarded(vec), _guarded(vec)
            assert lib.ctf_scripted_roles(vec._h, ptr(o1), m, pack, eps, 11, 4, 9, vec._stream()) == 0
            assert lib.ctf_scripted_actions(vec._h, ptr(o2), m, 0, eps, 11, 4, 9, vec._stream()) == 0
            assert torch.equal(b1, b2) and bool((o1 != SENTINEL).any())
    by_roles = vec.scripted_roles(["runner"] * n, team=1, epsilon=0.5, seed=3, step=8).clone()  # (both return the buffer the object owns)
    assert torch.equal(by_roles, vec.scripted_actions(team=1, epsilon=0.5, seed=3, step=8))
    vec.close()


def test_refused_arguments_leave_the_buffer_alone():
    vec = _vec(_arena(), n_envs=5)
    n = vec.N_AGENTS
    assert n < 16
    buf, out = _guarded(vec)
    lib, ptr, st = vec._lib, abi.ptr, vec._stream()
    assert lib.ctf_scripted_roles(vec._h, ptr(out), 1, 3, 0, 0, 0, 0, st) == -1                 # a nibble above 2
    assert lib.ctf_scripted_roles(vec._h, ptr(out), 1, 0xF << 60, 0, 0, 0, 0, st) == -1         # ... in the last one
    assert lib.ctf_scripted_roles(vec._h, ptr(out), 1, 3 << 4, 0, 0, 0, 0, st) == -1            # ... of an agent that is not asked
    assert lib.ctf_scripted_roles(vec._h, ptr(out), 1, 1 << (4 * n), 0, 0, 0, 0, st) == -1      # a role for agent N
    assert lib.ctf_scripted_roles(vec._h, ptr(out), 1 << n, 1, 0, 0, 0, 0, st) == -1            # a mask bit at N
    assert lib.ctf_scripted_roles(vec._h, ptr(out), 0x80000000, 1, 0, 0, 0, 0, st) == -1        # ... and far above it
    assert lib.ctf_scripted_roles(vec._h, None, 1, 1, 0, 0, 0, 0, st) == -1                     # no buffer
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()
    chase = ["chaser"] * n
    for roles, bad in ((chase, dict(agent_mask=1 << n)), (chase, dict(agent_mask=1, team=0)), (chase, dict()), (chase, dict(team=2)),
                       (chase, dict(agent_mask=1, epsilon=1.5)), (chase[:-1], dict(team=0)), (chase + ["runner"], dict(team=0)),
                       (["tagger"] * n, dict(team=0)), ({n: "guard"}, dict(team=0)), ({0: "keeper"}, dict(team=0))):
        with pytest.raises(ValueError):
            vec.scripted_roles(roles, out=out, **bad)
    with pytest.raises(ValueError):
        vec.scripted_actions(agent_mask=1, kind="chaser", out=out)  # the kinds of scripted_actions are what they were
    assert lib.ctf_scripted_actions(vec._h, ptr(out), 1, 1, 0, 0, 0, 0, st) == -1
    assert (buf == SENTINEL).all() and vec.status() == 0
    vec.close()


@pytest.mark.parametrize("rng_mode,log_metrics", [("mt19937", True), ("counter_direct", False), ("counter", True)])
def test_the_env_is_only_read(rng_mode, log_metrics):
    vec = _vec(_arena(GAME_STEPS=40), n_envs=E, rng_mode=rng_mode, log_metrics=log_metrics)
    _play(vec, 9)
    roles = rc.random_roles(np.random.default_rng(77), vec.N_AGENTS)
    before = vec.save_states().clone()
    got = vec.scripted_roles(_names(roles), agent_mask=sc.all_mask(vec.cfg), epsilon=0.25, seed=1, step=2).cpu().numpy()
    assert torch.equal(vec.save_states(), before)  # records hold the state, the generators and their positions
    assert np.array_equal(got, _ref_full(vec, roles, epsilon_q32=1 << 30, seed=1, step=2))
    assert vec.status() == 0
    vec.close()


def test_two_shards_with_env_offset_are_the_halves_of_one_batch():
    kw = _arena(GAME_STEPS=40)
    seeds = np.arange(E, dtype=np.uint64) * 13 + 5
    whole = _vec(kw)
    a = _vec(kw, n_envs=40, py_seeds=seeds[:40], np_seeds=seeds[:40])
    b = _vec(kw, n_envs=E - 40, py_seeds=seeds[40:], np_seeds=seeds[40:])
    _play(whole, 21)
    _play(a, 21)
    _play(b, 21, env_offset=40)
    roles = rc.random_roles(np.random.default_rng(78), whole.N_AGENTS)
    args = dict(agent_mask=sc.all_mask(whole.cfg), epsilon=0.5, seed=99, step=21)
    w = whole.scripted_roles(_names(roles), **args).cpu().numpy()
    assert np.array_equal(w, _ref_full(whole, roles, epsilon_q32=1 << 31, seed=99, step=21))
    assert np.array_equal(a.scripted_roles(_names(roles), **args).cpu().numpy(), w[:40])
    assert np.array_equal(b.scripted_roles(_names(roles), env_offset=40, **args).cpu().numpy(), w[40:])
    for v in (whole, a, b):
        v.close()


def test_step_and_scripted_roles_replay_from_one_captured_graph():
    """bots on both sides: every replay is (decide, step); the plain calls on a second batch of the same seeds give the same"""
    kw = _arena(GAME_STEPS=15)  # the replays pass an episode's end (auto-reset inside the graph)
    plain, graphed = _vec(kw), _vec(kw)
    mask, dev = sc.all_mask(plain.cfg), plain.device
    roles = _names(rc.random_roles(np.random.default_rng(79), plain.N_AGENTS))
    args = dict(agent_mask=mask, epsilon=0.25, seed=3, step=7)
    want = []
    acts = torch.zeros((E, plain.N_AGENTS), dtype=torch.int8, device=dev)
    for _ in range(20):
        plain.scripted_roles(roles, out=acts, **args)
        want.append(acts.cpu().numpy().copy())
        plain.step(acts, auto_reset=True)
    g_acts = torch.zeros_like(acts)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph, stream=side):
        graphed.scripted_roles(roles, out=g_acts, **args)
        graphed.step(g_acts, auto_reset=True)
    torch.cuda.synchronize(dev)
    for k in range(20):
        graph.replay()
        torch.cuda.synchronize(dev)
        assert np.array_equal(g_acts.cpu().numpy(), want[k]), k
    fa, fb = _final(graphed), _final(plain)
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    for x, y in zip(graphed.get_rng_states(), plain.get_rng_states()):
        assert torch.equal(x, y)
    assert len({w.tobytes() for w in want}) == 20 and graphed.status() == 0
    plain.close()
    graphed.close()


@pytest.mark.parametrize("team", (0, 1))
def test_collect_against_a_scripted_team_equals_the_hand_written_loop(team):
    """roles as a callable of the config: the guardians guard, the rest run"""
    kw = _arena(GAME_STEPS=25)
    T, n_envs = 40, 6
    a, b = _vec(kw, n_envs=n_envs), _vec(kw, n_envs=n_envs)
    net = StubPolicy(4)
    bot = pkg.ScriptedTeam(scripted.guardians_guard, epsilon=0.125, seed=21)
    assert isinstance(bot, pkg.ScriptedPolicy)
    out = rollout.BatchedRolloutCollector(a, T, team).collect(net, bot)
    roles = ["guard" if b.AGENT_TYPES[i] == 1 else "runner" for i in range(b.N_AGENTS)]
    assert bot._resolved == roles and "guard" in roles
    col2 = rollout.BatchedRolloutCollector(b, T, team)
    others_mask = sum(1 << i for i in range(b.N_AGENTS) if b.AGENT_TEAMS[i] != team)
    b.reset()
    acts_log, rew_log = [], []
    for t in range(T):
        o, m = b.observe()
        act = col2._policy(net, o, m, col2.trained_idx)[0]
        joint = torch.zeros((n_envs, b.N_AGENTS), dtype=torch.int8, device=b.device)
        env_act = act.to(torch.int8).transpose(0, 1)
        joint[:, col2.trained_idx] = col2.rev_lut[env_act.long()] if team == 1 else env_act
        b.scripted_roles(roles, agent_mask=others_mask, out=joint, epsilon=0.125, seed=21, step=t)
        rewards, _ = b.step(joint)
        acts_log.append(act.to(torch.float32))
        rew_log.append(rewards.index_select(1, col2.trained_idx).transpose(0, 1).clone())
    assert torch.equal(out["actions"], torch.cat(acts_log)) and torch.equal(out["rewards"], torch.cat(rew_log))
    fa, fb = _final(a), _final(b)
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    a.close()
    b.close()


def test_tournament_with_a_scripted_team_equals_the_hand_written_loop():
    kw = _arena(GAME_STEPS=30)
    agents, per = [StubPolicy(1), StubPolicy(2)], 3
    a, b = _vec(kw, n_envs=12), _vec(kw, n_envs=12)
    roles = {i: "chaser" if i % 4 == 1 else "guard" for i in range(b.N_AGENTS) if i % 4 != 3}
    res = duel.batched_tournament(a, agents, [pkg.ScriptedTeam(roles, epsilon=0.0625, seed=8), pkg.ScriptedPolicy(epsilon=0.0625, seed=9)], max_steps=29)
    assert res["steps"] == 30 and res["episodes"].tolist() == [[per, per], [per, per]]
    col = rollout.BatchedRolloutCollector(b, 1, 0)
    b.reset()
    team_rows = torch.tensor([e for e in range(12) if (e // per) % 2 == 0], device=b.device)    # blocks (a, 0): the team of roles
    runner_rows = torch.tensor([e for e in range(12) if (e // per) % 2 == 1], device=b.device)  # blocks (a, 1): the runner
    scratch = torch.zeros((12, b.N_AGENTS), dtype=torch.int8, device=b.device)
    for t in range(30):
        obs, meta = b.observe()
        acts = torch.zeros((12, b.N_AGENTS), dtype=torch.int8, device=b.device)
        for k, net in enumerate(agents):
            sl = slice(k * 2 * per, (k + 1) * 2 * per)
            acts[sl][:, col.trained_idx] = col._policy(net, obs[sl], meta[sl], col.trained_idx)[0].to(torch.int8).transpose(0, 1)
        b.scripted_roles(roles, team=1, out=scratch, step=t, epsilon=0.0625, seed=8)
        acts[team_rows[:, None], col.others_idx[None, :]] = scratch[team_rows[:, None], col.others_idx[None, :]]
        b.scripted_actions(team=1, out=scratch, step=t, epsilon=0.0625, seed=9)
        acts[runner_rows[:, None], col.others_idx[None, :]] = scratch[runner_rows[:, None], col.others_idx[None, :]]
        b.step(acts)
    fa, fb = _final(a), _final(b)
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    a.close()
    b.close()


def test_guards_tag_the_runners():
    """64 arena envs, one 500-step episode, every agent a bot, team 0 all runners.  Run A: team 1 all runners.  Run B: team 1's
    guardians guard.  Team 1's flag_dispossessions + respawn_tag_count must be higher in B.  The env is bit-exact and the actions
    byte-equal, so the counts must be those of the restatement on the oracle (tests/test_scripted_roles_cpu.py, where the reason the
    captures are not asserted is given):
      A  230 captures by team 0, 322 tags by team 1
      B  710 captures by team 0, 3375 tags by team 1"""
    n_envs = rc.BEHAVIOUR_E
    seeds = np.arange(n_envs, dtype=np.uint64)
    counts = []
    for guards in (False, True):
        vec = pkg.VecGridworldCtf(n_envs, device=0, py_seeds=seeds, np_seeds=seeds, tune_placement=False, **_arena())
        roles = _names(rc.behaviour_roles(vec.cfg, guards))
        acts = torch.empty((n_envs, vec.N_AGENTS), dtype=torch.int8, device=vec.device)
        for t in range(rc.BEHAVIOUR_STEPS):
            vec.scripted_roles(roles, agent_mask=sc.all_mask(vec.cfg), out=acts)
            _, done = vec.step(acts)
        assert bool(done.all()) and vec.status() == 0
        met, caps, _ = vec.counters()
        team1 = [i for i in range(vec.N_AGENTS) if vec.AGENT_TEAMS[i] == 1]
        counts.append((int(caps[:, 0].sum()), int(met[:, rc.DISPOSSESSIONS][:, team1].sum() + met[:, rc.RESPAWN_TAGS][:, team1].sum())))
        vec.close()
    (caps_a, tags_a), (caps_b, tags_b) = counts
    print(f"run A: {caps_a} captures, {tags_a} tags; run B: {caps_b} captures, {tags_b} tags")
    assert tags_b > tags_a, counts
    assert counts == [(230, 322), (710, 3375)]  # the CPU run's, count for count

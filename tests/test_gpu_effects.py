"""k_action_effects and k_random_effective (ctf_action_effects, ctf_random_effective_actions; VecGridworldCtf.effective_actions /
action_effects / random_effective_actions, GridworldCtf's two methods, ScriptedWanderer) on the device: masks and flag bytes must
equal tests/_effects_ref.py entry for entry — on the recorded fixture's states and the crafted edge states through set_states, in
batches of 1, 3 and 9 envs (8, 24 and 72 lanes at N = 8: under a wave and across one) and at N = 16, G = 32, in buffers with sentinel
guard rows, under team masks, single-agent masks and mask 0, with either output NULL — on every agent count; the env only read;
refused arguments; inside a captured graph; what the flags promise against what ctf_step then does; the sampler against its
restatement; the wanderer in a duel and a tournament; the drop-in facade."""
import numpy as np
import pytest

import _agent_counts as ac
import _effects_cases as ec
import _effects_ref as er
import _rule_cases as rc
import _scripted_cases as sc
from _cases import abi, pkg
from _stub_policy import StubPolicy
from test_effects_cpu import check_invariants

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MASK_SENTINEL, FLAG_SENTINEL, ACT_SENTINEL = 0x5555, 0xA5, 0x5A
FIELDS = ("grid", "pos", "hp", "has_flag", "inventory")


def _vec(kw, n_envs, seeds=None, **more):
    seeds = np.arange(n_envs, dtype=np.uint64) * 13 + 5 if seeds is None else seeds
    return pkg.VecGridworldCtf(n_envs, device=0, tune_placement=False, py_seeds=seeds, np_seeds=seeds, **more, **kw)


def _host_states(vec):
    """-> [per env: dict(grid, pos, hp, has_flag, inv)]"""
    st = {k: v.cpu().numpy() for k, v in vec.get_states(fields=FIELDS).items()}
    return [dict(grid=st["grid"][e], pos=st["pos"][e], hp=st["hp"][e], has_flag=st["has_flag"][e], inv=st["inventory"][e]) for e in range(vec.n_envs)]


def _ref_full(vec):
    """the restatement for every agent of every env -> (mask uint16 [E, N], effects uint8 [E, N, 9])"""
    rules = er.cfg_rules(vec.cfg)
    both = [er.env_effects(rules, st) for st in _host_states(vec)]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def _plant(vec, states):
    """env e := states[e] (dicts of grid, pos, hp, has_flag, inv)"""
    st = vec.get_states()
    for e, planted in enumerate(states):
        for k in FIELDS:
            st[k][e] = torch.from_numpy(np.asarray(planted["inv" if k == "inventory" else k])).to(vec.device)
    st.pop("metrics", None)
    vec.set_states(st)
    assert vec.status() == 0


def _play(vec, steps, seed=0xACE):
    acts = torch.empty((vec.n_envs, vec.N_AGENTS), dtype=torch.int8, device=vec.device)
    for t in range(steps):
        vec.random_actions(acts, seed, t, 0)
        vec.step(acts, auto_reset=True)


def _guarded(vec):
    """(mask buffer, its inner rows, flag buffer, its inner rows): a sentinel row before and after the E rows a call may write"""
    E, N = vec.n_envs, vec.N_AGENTS
    mbuf = torch.full((E + 2, N), MASK_SENTINEL, dtype=torch.int16, device=vec.device)
    fbuf = torch.full((E + 2, N, 9), FLAG_SENTINEL, dtype=torch.uint8, device=vec.device)
    return mbuf, mbuf[1:E + 1], fbuf, fbuf[1:E + 1]


def _expect(want, agent_mask, sentinel):
    """a guarded buffer after a call for ``agent_mask``: the sentinel everywhere but the asked agents' entries of the inner rows"""
    n = want.shape[1]
    sel = np.array([(agent_mask >> i) & 1 for i in range(n)], bool)
    exp = np.full((want.shape[0] + 2,) + want.shape[1:], sentinel, want.dtype)
    exp[1:-1][:, sel] = want[:, sel]
    return exp


def _check(vec, agent_masks, want=None, forms=("both", "mask", "flags")):
    """the launch for each mask, in each form (both outputs, the mask alone, the flags alone), against the restatement"""
    want_m, want_f = _ref_full(vec) if want is None else want
    check_invariants(want_m, want_f)
    for m in agent_masks:
        for form in forms:
            mbuf, mask, fbuf, flags = _guarded(vec)
            if form == "both":
                vec._call("ctf_action_effects", abi.ptr(mask), abi.ptr(flags), m, vec._stream())
            elif form == "mask":
                assert vec.effective_actions(agent_mask=m, out=mask) is mask
            else:
                assert vec.action_effects(agent_mask=m, out=flags) is flags
            exp_m = _expect(want_m.view(np.int16), m if form != "flags" else 0, np.int16(MASK_SENTINEL))
            exp_f = _expect(want_f, m if form != "mask" else 0, np.uint8(FLAG_SENTINEL))
            assert np.array_equal(mbuf.cpu().numpy(), exp_m), f"mask, {form}, agents 0x{m:x}"
            assert np.array_equal(fbuf.cpu().numpy(), exp_f), f"flags, {form}, agents 0x{m:x}"
    return want_m, want_f


def _masks(cfg):
    n = cfg.n_agents
    return [sc.all_mask(cfg)] + sc.team_masks(cfg) + [1 << i for i in range(n)] + [0]


# ---- the fixture's and the crafted states through set_states ---------------------------------------------------------------------
def _groups():
    out = {f"{block}_{name}": (kw, cfg, states, eff) for block, name, kw, cfg, states, eff in ec.fixture_entries()}
    out.update({name: (kw, cfg, states, None) for name, (kw, cfg, states) in ec.edge_groups().items()})
    return out


GROUPS = sorted(_groups())


@pytest.mark.parametrize("name", GROUPS)
def test_fixture_and_edge_states_through_set_states(name):
    kw, cfg, states, recorded = _groups()[name]
    sizes = (1, 3, 9) if name == "played_arena" else (9,)  # N = 8: 8, 24 and 72 lanes; elsewhere batches of nine envs
    if name == "played_arena":
        assert cfg.n_agents == 8
    if name == "large32":
        assert cfg.n_agents == 16 and cfg.grid_size == 32
    vecs = {E: _vec(kw, E) for E in sizes}
    masks, k, batch = _masks(cfg), 0, 0
    while k < len(states):
        E = sizes[batch % len(sizes)]
        vec = vecs[E]
        idx = [min(k + j, len(states) - 1) for j in range(E)]  # (the last batch repeats the last state)
        _plant(vec, [states[j] for j in idx])
        host = _host_states(vec)
        assert all(np.array_equal(host[e][f], states[j][f]) for e, j in enumerate(idx) for f in ec.FIELDS)
        rules = er.cfg_rules(cfg)
        both = [er.env_effects(rules, states[j]) for j in idx]
        want = (np.stack([b[0] for b in both]), np.stack([b[1] for b in both]))
        if recorded is not None:
            assert np.array_equal(want[1], recorded[idx])  # the reference's own bytes
        # the full mask in every form; a team mask, a single-agent mask or mask 0 in turn
        _check(vec, [masks[0]], want)
        _check(vec, [masks[1 + batch % (len(masks) - 1)]], want, forms=("both", "mask", "flags")[batch % 3:batch % 3 + 1])
        k += E
        batch += 1
    _check(vec, masks, want)  # every mask on the last batch
    for vec in vecs.values():
        assert vec.status() == 0
        vec.close()


@pytest.mark.parametrize("c", ac.CONFIGS, ids=ac.config_id)
def test_every_agent_count(c):
    cfg = ac.build(*c)
    vec = _vec(ac.config_kwargs(*c), 3)
    _play(vec, 17)
    full = sc.all_mask(cfg)
    want_m, _ = _check(vec, [full] + sc.team_masks(cfg) + [1 << (cfg.n_agents - 1)])
    buf = torch.full((5, cfg.n_agents), ACT_SENTINEL, dtype=torch.int8, device=vec.device)
    vec.random_effective_actions(buf[1:4], 77 + c[0], 5, team=1, env_offset=9)
    exp = np.full((5, cfg.n_agents), ACT_SENTINEL, np.int8)
    for e in range(3):
        er.sample_env(want_m[e], 77 + c[0], 9 + e, 5, sc.team_masks(cfg)[1], exp[1 + e])
    assert np.array_equal(buf.cpu().numpy(), exp)
    assert vec.status() == 0
    vec.close()


@pytest.mark.parametrize("rng_mode,log_metrics", [("mt19937", True), ("counter_direct", False)])
def test_the_env_is_only_read_in_every_mode(rng_mode, log_metrics):
    vec = _vec(dict(sc.workloads()["arena"], GAME_STEPS=40), 37, rng_mode=rng_mode, log_metrics=log_metrics)
    n, full = vec.N_AGENTS, sc.all_mask(vec.cfg)
    _play(vec, 21)
    before = vec.save_states().clone()
    want_m, _ = _check(vec, [full, 1 << (n - 1)])
    acts = torch.zeros((37, n), dtype=torch.int8, device=vec.device)
    vec.random_effective_actions(acts, 3, 4)
    assert torch.equal(vec.save_states(), before)  # records hold the state, the generators and their positions
    assert np.array_equal(acts.cpu().numpy(), np.stack([er.sample_env(want_m[e], 3, e, 4, full, np.zeros(n, np.int8)) for e in range(37)]))
    assert vec.status() == 0
    vec.close()


def test_refused_arguments_leave_the_buffers_alone():
    vec = _vec(dict(sc.workloads()["arena"]), 5)
    n = vec.N_AGENTS
    assert n < 16
    mbuf, mask, fbuf, flags = _guarded(vec)
    abuf = torch.full((7, n), ACT_SENTINEL, dtype=torch.int8, device=vec.device)
    acts = abuf[1:6]
    lib, ptr, st = vec._lib, abi.ptr, vec._stream()
    call = lambda m, f, agents: lib.ctf_action_effects(vec._h, m, f, agents, st)  # noqa: E731
    assert call(None, None, 1) == -1                                # both outputs NULL
    assert call(None, None, 0) == -1                                # ... with an empty mask as well
    assert call(ptr(mask), ptr(flags), 1 << n) == -1                # a mask bit at N
    assert call(ptr(mask), ptr(flags), 0x80000000) == -1            # ... and far above it
    assert call(None, ptr(flags), 1 << n) == -1
    assert call(mask.data_ptr() + 1, ptr(flags), 1) == -1           # an odd mask address
    assert call(mask.data_ptr() + 1, None, 0) == -1
    assert lib.ctf_action_effects(None, ptr(mask), ptr(flags), 1, st) == -1  # a null handle
    draw = lambda a, agents: lib.ctf_random_effective_actions(vec._h, a, agents, 1, 2, 3, st)  # noqa: E731
    assert draw(None, 1) == -1 and draw(ptr(acts), 1 << n) == -1 and draw(ptr(acts), 0x80000000) == -1
    assert lib.ctf_random_effective_actions(None, ptr(acts), 1, 1, 2, 3, st) == -1
    torch.cuda.synchronize()
    for method, out in ((vec.effective_actions, mask), (vec.action_effects, flags)):
        for bad in (dict(agent_mask=1 << n), dict(agent_mask=-1), dict(agent_mask=1, team=0), dict(team=2),
                    dict(out=torch.zeros((5, n), dtype=torch.int8, device=vec.device)), dict(out=torch.zeros((4, n, 9), dtype=torch.uint8, device=vec.device)),
                    dict(out=out.cpu())):
            with pytest.raises(ValueError):
                method(**dict(dict(out=out), **bad))
    for bad in (dict(agent_mask=1 << n), dict(agent_mask=1, team=1), dict(team=-1)):
        with pytest.raises(ValueError):
            vec.random_effective_actions(acts, 1, 2, **bad)
    with pytest.raises(ValueError):
        vec.random_effective_actions(acts.to(torch.int16), 1, 2)
    torch.cuda.synchronize()
    assert (mbuf == MASK_SENTINEL).all() and (fbuf == FLAG_SENTINEL).all() and (abuf == ACT_SENTINEL).all() and vec.status() == 0
    # the buffers the object owns; neither argument: all agents
    owned_m, owned_f = vec.effective_actions(), vec.action_effects()
    want_m, want_f = _ref_full(vec)
    assert owned_m.dtype == torch.int16 and owned_f.dtype == torch.uint8 and vec.effective_actions() is owned_m and vec.action_effects() is owned_f
    assert np.array_equal(owned_m.cpu().numpy().view(np.uint16), want_m) and np.array_equal(owned_f.cpu().numpy(), want_f)
    assert np.array_equal(pkg.effects_table(owned_m).cpu().numpy(), want_f != 0)
    vec.close()


def test_one_launch_in_a_captured_graph_gives_the_new_states_effects():
    vec = _vec(dict(sc.workloads()["arena"], GAME_STEPS=40), 5)
    n, full, dev = vec.N_AGENTS, sc.all_mask(vec.cfg), vec.device
    _play(vec, 9)
    mbuf, mask, fbuf, flags = _guarded(vec)
    abuf = torch.full((7, n), ACT_SENTINEL, dtype=torch.int8, device=dev)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph, stream=side):
        vec._call("ctf_action_effects", abi.ptr(mask), abi.ptr(flags), full, vec._stream())
        vec.random_effective_actions(abuf[1:6], 0xD1CE, 7, env_offset=2)
    torch.cuda.synchronize(dev)
    seen = []
    acts = torch.empty((vec.n_envs, n), dtype=torch.int8, device=dev)
    for k in range(4):
        want_m, want_f = _ref_full(vec)
        mbuf.fill_(MASK_SENTINEL)
        fbuf.fill_(FLAG_SENTINEL)
        abuf.fill_(ACT_SENTINEL)
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert np.array_equal(mbuf.cpu().numpy(), _expect(want_m.view(np.int16), full, np.int16(MASK_SENTINEL))), k
        assert np.array_equal(fbuf.cpu().numpy(), _expect(want_f, full, np.uint8(FLAG_SENTINEL))), k
        drawn = np.stack([er.sample_env(want_m[e], 0xD1CE, 2 + e, 7, full, np.zeros(n, np.int8)) for e in range(vec.n_envs)])
        assert np.array_equal(abuf.cpu().numpy(), _expect(drawn, full, np.int8(ACT_SENTINEL))), k
        seen.append(want_f.tobytes())
        for t in range(3):
            vec.random_actions(acts, 0xBEE, 3 * k + t, 0)
            vec.step(acts, auto_reset=True)
    assert len(set(seen)) == 4 and vec.status() == 0
    vec.close()


# ---- what the flags promise is what ctf_step does ----------------------------------------------------------------------------------
# 7 x 7, the two flags two cells apart ((2, 3), (3, 3) and (4, 3) touch both); nobody tags, nobody heals.  Agent 0 a scout at (1, 3)
# (down: pickup and capture), 1 a miner of the other team at (5, 5) with one block, tile 2 to its right and tile 3 below it, 2 a vaulter
# at (5, 3) (a jump up lands between the flags), 3 a scout in a corner behind two blocks
PROMISE = ec._open_map(7, [(3, 2), (3, 4)], [(0, 0), (0, 6)], [(0, 0), (1, 3), (0, 2), (1, 0)], TAG_PROBABILITY=0.0, AGENT_HP_HEALING_PER_STEP=0.0,
                      HOME_FLAG_CAPTURE=True)
PROMISE_POS = {0: (1, 3), 1: (5, 5), 2: (5, 3), 3: (6, 0)}
PROMISE_STATES = {
    "tile2": ec.place(PROMISE, PROMISE_POS, inv={1: 1}, tiles={(5, 6): 2, (6, 5): 3, (5, 0): 1, (6, 1): 1}),
    "tile3": ec.place(PROMISE, PROMISE_POS, inv={1: 1000}, tiles={(5, 6): 3, (6, 5): 2, (5, 0): 1, (6, 1): 1}),  # the same dig one hit on, at the cap
    # both flags away (a carrier whose own flag is away does not capture); 1.5 - 0.5 > 1.0 is false: no jump
    "carrying": ec.place(PROMISE, PROMISE_POS, inv={1: 0}, flag=(0, 1), hp={2: 1.5}),
}


@pytest.mark.parametrize("name", sorted(PROMISE_STATES))
def test_what_the_flags_promise_is_what_the_step_does(name):
    state = PROMISE_STATES[name]
    n = len(PROMISE["AGENT_CONFIG"])
    E = 9 * n
    vec = _vec(PROMISE, E)
    assert vec.cfg.tag_probability == 0 and vec.cfg.heal_per_step == 0 and vec.cfg.log_metrics
    rules, cost = er.cfg_rules(vec.cfg), float(vec.cfg.vault_hp_cost)
    _plant(vec, [state] * E)
    eff = vec.action_effects().cpu().numpy()
    want = er.env_effects(rules, state)[1]
    assert (eff == want[None]).all()
    if name == "tile2":
        assert want[0, 1] == 13 and want[2, 5] == 15 and want[1, 2] == 16 and want[1, 1] == 48 and want[1, 5] == 64 and (want[3] == 0).all()
    elif name == "tile3":
        assert want[1, 2] == 48 and want[1, 1] == 16
    else:
        assert want[0, 1] == 1 and (want[2, 5:] == 0).all() and (want[1, 5:] == 0).all()
    acts = torch.full((E, n), 4, dtype=torch.int8, device=vec.device)
    for e in range(E):
        acts[e, e // 9] = e % 9
    before = {k: v.cpu().numpy() for k, v in vec.get_states().items()}
    vec.step(acts)
    after = {k: v.cpu().numpy() for k, v in vec.get_states().items()}
    assert vec.status() == 0
    M = {m: k for k, m in enumerate(abi.METRIC_NAMES)}
    counter_of = {"flag_pickups": er.PICKS_UP, "flag_captures": er.CAPTURES, "blocks_mined": er.BREAKS, "blocks_laid": er.LAYS}
    for e in range(E):
        i, a = e // 9, e % 9
        f = int(eff[e, i, a])
        team, kind = rules["teams"][i], rules["types"][i]
        b = {k: v[e] for k, v in before.items()}
        s = {k: v[e] for k, v in after.items()}
        what = (name, i, a, f)
        others = [j for j in range(n) if j != i]
        for k in ("pos", "hp", "has_flag", "inventory"):
            assert np.array_equal(b[k][others].view(np.uint8), s[k][others].view(np.uint8)), what
        assert (not np.array_equal(b["pos"][i], s["pos"][i])) == bool(f & er.MOVES), what
        if f & er.JUMPS:
            assert s["hp"][i] == b["hp"][i] - cost and s["hp"][i] < b["hp"][i], what
        else:
            assert s["hp"][i].tobytes() == b["hp"][i].tobytes(), what
        for metric, flag in counter_of.items():
            rose = s["metrics"][M[metric]] - b["metrics"][M[metric]]
            assert rose.tolist() == [int(j == i and bool(f & flag)) for j in range(n)], (what, metric)
        grid = b["grid"].copy()
        me = tuple(int(x) for x in b["pos"][i])
        d = er.delta(kind, a)
        to = (me[0] + d[0], me[1] + d[1]) if d is not None else None
        carrying, inv = int(b["has_flag"][i]), int(b["inventory"][i])
        if f & er.MOVES:
            assert tuple(int(x) for x in s["pos"][i]) == to and bool(f & er.JUMPS) == (a >= 5), what
            grid[me], grid[to] = 0, 4 + kind + 4 * team
            other = rules["flag_pos"][1 - team]
            if f & er.PICKS_UP:
                grid[other], carrying = 1, 1
            if f & er.CAPTURES:
                grid[other], carrying = 12 + (1 - team), 0
            assert s["team_captures"][team] == b["team_captures"][team] + bool(f & er.CAPTURES), what
        elif f & er.MINES:
            assert grid[to] == (3 if f & er.BREAKS else 2), what
            grid[to] = 0 if f & er.BREAKS else 3
            inv += 1 if f & er.BREAKS and inv < 1000 else 0
        elif f & er.LAYS:
            assert grid[to] == 0, what
            grid[to], inv = 2, inv - 1
        assert np.array_equal(s["grid"], grid) and int(s["has_flag"][i]) == carrying and int(s["inventory"][i]) == inv, what
        if f == 0:
            assert all(np.array_equal(b[k], s[k]) for k in ("grid", "pos", "has_flag", "inventory")), what
    vec.close()


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
def test_the_sampler_against_its_restatement():
    vec = _vec(dict(sc.workloads()["arena"], GAME_STEPS=40), 5)
    n, full = vec.N_AGENTS, sc.all_mask(vec.cfg)
    _play(vec, 17)
    want_m, _ = _ref_full(vec)
    seen = set()
    for seed, step, offset, agents in ((0, 0, 0, full), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE, full), (0x123456789ABCDEF, 41, 1000, vec.team_mask(0)),
                                       (7, 8, 9, vec.team_mask(1)), (7, 9, 9, 1 << (n - 1)), (7, 9, 9, 0)):
        buf = torch.full((7, n), ACT_SENTINEL, dtype=torch.int8, device=vec.device)
        assert vec.random_effective_actions(buf[1:6], seed, step, agent_mask=agents, env_offset=offset) is not None
        drawn = np.stack([er.sample_env(want_m[e], seed, (offset + e) & 0xFFFFFFFF, step, full, np.zeros(n, np.int8)) for e in range(5)])
        assert np.array_equal(buf.cpu().numpy(), _expect(drawn, agents, np.int8(ACT_SENTINEL))), (seed, step, offset)
        got = buf[1:6].cpu().numpy()
        for e in range(5):
            for i in range(n):
                if (agents >> i) & 1:
                    assert (want_m[e, i] >> got[e, i]) & 1 or (want_m[e, i] == 0 and got[e, i] == 4)  # the drawn action does something
        seen.add(drawn.tobytes())
    assert len(seen) >= 4
    # the wanderer: calls count the steps, and the same object replays the same actions after restart()
    bot = pkg.ScriptedWanderer(seed=9)
    first = bot.act(vec, full).clone()
    second = bot.act(vec, full).clone()
    assert bot.calls == 2 and not torch.equal(first, second)
    want = lambda step: np.stack([er.sample_env(want_m[e], 9, e, step, full, np.zeros(n, np.int8)) for e in range(5)])  # noqa: E731
    assert np.array_equal(first.cpu().numpy(), want(0)) and np.array_equal(second.cpu().numpy(), want(1))
    bot.restart()
    assert torch.equal(bot.act(vec, full), first) and bot.calls == 1
    assert vec.status() == 0
    vec.close()


def test_an_agent_none_of_whose_actions_does_anything_gets_4():
    walled = rc.state("term", tiles={(0, 1): 1, (1, 0): 1, (5, 6): 1, (6, 5): 1})  # scouts 2 at (0, 0) and 3 at (6, 6) behind two blocks each
    kw, cfg = ec.config("planted", "term")
    vec = _vec(kw, 3)
    _plant(vec, [{f: walled[f] for f in ec.FIELDS}] * 3)
    want_m, _ = _check(vec, [sc.all_mask(cfg)])
    assert want_m[0, 2] == 0 and want_m[0, 3] == 0 and want_m[0, 0] != 0
    acts = torch.full((3, 4), ACT_SENTINEL, dtype=torch.int8, device=vec.device)
    for step in range(4):
        vec.random_effective_actions(acts, 11, step)
        got = acts.cpu().numpy()
        assert (got[:, 2:] == 4).all() and ((want_m[:, :2] >> got[:, :2]) & 1).all()
    vec.close()


# ---- where a bot sits ----------------------------------------------------------------------------------------------------------------
def test_the_wanderer_in_a_duel_and_a_tournament():
    kw = dict(sc.workloads()["arena"], GAME_STEPS=20)
    a, b = _vec(kw, 3), _vec(kw, 3)
    bot = pkg.ScriptedWanderer(seed=4)
    res = pkg.batched_duel(a, StubPolicy(1), bot, max_steps=19)
    assert res["steps"] == 20 and bot.calls == 20 and a.status() == 0
    out = pkg.batched_tournament(b, [StubPolicy(1)], [pkg.ScriptedWanderer(seed=4), pkg.ScriptedPolicy(), StubPolicy(2)], max_steps=19)
    assert out["steps"] == 20 and out["episodes"].tolist() == [[1, 1, 1]] and b.status() == 0
    a.close()
    b.close()


def test_the_drop_in_facade_gives_row_0_of_a_one_env_batch():
    kw = dict(sc.workloads()["arena"])
    env = pkg.GridworldCtf(rng="device", seed=5, device=0, **kw)
    vec = _vec(kw, 1, seeds=np.array([5], np.uint64))
    n = env.N_AGENTS
    seen = set()
    for t in range(6):
        eff, mask = env.action_effects(), env.effective_actions()
        assert isinstance(eff, np.ndarray) and eff.shape == (n, 9) and eff.dtype == np.uint8 and mask.shape == (n,) and mask.dtype == np.int16
        assert np.array_equal(env.grid, vec.get_states(fields=("grid",))["grid"][0].cpu().numpy())
        assert np.array_equal(eff, vec.action_effects()[0].cpu().numpy()) and np.array_equal(mask, vec.effective_actions()[0].cpu().numpy())
        want_m, want_f = _ref_full(vec)
        assert np.array_equal(eff, want_f[0]) and np.array_equal(mask.view(np.uint16), want_m[0])
        seen.add(eff.tobytes())
        acts = [(3 * t + i) % 9 for i in range(n)]
        env.step(acts)
        vec.step(torch.tensor([acts], dtype=torch.int8, device=vec.device))
    assert len(seen) > 1 and vec.status() == 0
    vec.close()

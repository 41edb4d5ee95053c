"""The inputs of the agent-count sweep (tests/_agent_counts.py), checked with the CPU oracle alone, and the oracle against the live
reference on the same 29 configurations.

tests/test_gpu_agent_counts.py follows one oracle env per device env and drops an env only where the oracle itself reports a
non-zero status (no respawn cell).  Whether its runs then still test anything — enough envs left, episodes that end, captures,
counters in the last counter word — is a property of the configurations, asserted here at the env counts, seeds, action streams
and step counts that file uses, not measured there."""
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import _refimport  # noqa: E402
import make_golden_live as live  # noqa: E402

import oracle  # noqa: E402
import _agent_counts as ac  # noqa: E402
from _cases import abi, view_arrays  # noqa: E402

IDS = [ac.config_id(c) for c in ac.CONFIGS]


@pytest.fixture(scope="module")
def runs():
    """every oracle-only run of the sweep, once: (n, lop, which) -> oracle_run's dict"""
    out = {}
    for n, lop in ac.CONFIGS:
        cfg = ac.build(n, lop)
        out[n, lop, "main"] = ac.oracle_run(cfg, ac.seeds(), ac.STEPS)
        out[n, lop, "stagger"] = ac.oracle_run(cfg, ac.seeds(), ac.STEPS, stagger=True)
        if n in ac.COUNTER_N:
            out[n, lop, "counter"] = ac.oracle_run(ac.build(n, lop, counter=True), ac.seeds(), ac.STEPS)
        out[n, lop, "direct"] = ac.oracle_run(ac.build(n, lop, counter=True), ac.seeds(), ac.DIRECT_STEPS)
        if (n, lop) in ac.LANE_CONFIGS:
            out[n, lop, "lanes"] = ac.oracle_run(cfg, ac.lane_seeds(), ac.LANE_STEPS, act_seed=ac.LANE_SEED, env_offset=ac.LANE_OFFSET)
    return out


def test_the_generator_covers_what_it_says():
    assert len(ac.CONFIGS) == 29 and {n for n, _ in ac.CONFIGS} == set(range(2, 17))
    shapes = {}
    for n, lop in ac.CONFIGS:
        cfg = ac.build(n, lop)
        g = cfg.grid_size
        assert cfg.n_agents == n and int(cfg.game_steps) == ac.GAME_STEPS and g == ac.grid_size(n, lop)
        shapes[n, lop] = ((g * g + 15) // 16 * 16, tuple(cfg.n_opponents))
        t = ac.teams(n, lop)
        assert [int(cfg.agent_team[i]) for i in range(n)] == t and 0 < sum(t) < n
    assert {gs for gs, _ in shapes.values()} == {64, 96, 112, 128}
    # the lopsided configs above eight agents: opponent lists cut to N // 2, of different lengths
    assert [shapes[n, 1][1] for n in (10, 12, 14, 16)] == [(5, 2), (6, 3), (7, 3), (8, 4)]
    assert all(shapes[n, 0][1] == (n // 2, n // 2) for n in range(2, 17))


@pytest.mark.parametrize("config", ac.CONFIGS, ids=IDS)
def test_every_run_keeps_its_envs_and_ends_episodes(runs, config):
    n, lop = config
    for which in ("main", "stagger", "counter", "lanes"):
        r = runs.get((n, lop, which))
        if r is None:
            continue
        count = len(r["alive"])
        assert 4 * int((~r["alive"]).sum()) <= count, f"{which}: the oracle drops {(~r['alive']).sum()} of {count} envs"
        assert (r["episodes"][r["alive"]] >= 1).all(), f"{which}: a surviving env ends no episode"
    ac.lockstep_mask(runs[n, lop, "main"]["alive_at_30"])  # (asserts that 7 and 9 survivors can be picked)
    assert runs[n, lop, "main"]["alive_at_30"][64:].any()


@pytest.mark.parametrize("config", ac.CONFIGS, ids=IDS)
def test_the_counter_direct_run_keeps_its_envs_and_ends_an_episode(runs, config):
    """test_counter_direct_step_at_every_count's input, at its seeds, action stream and steps, on the counter tape"""
    r = runs[config[0], config[1], "direct"]
    assert len(r["alive"]) == ac.E and int((~r["alive"]).sum()) <= ac.DIRECT_DROP_CAP, f"the oracle drops {(~r['alive']).sum()} envs"
    assert (r["episodes"][r["alive"]] == 1).all(), "every followed env ends one episode"


def test_the_larger_counts_draw_past_the_np_window():
    """a step's tag compares take two np.random words per (damage-dealing agent, opponent) pair: more than the window's bytes from
    9-even and 12-lop upwards, where the last compares of every step are computed on demand"""
    import _counter_direct_cases as cd

    np_cap = cd.window_caps()[0]
    words = {}
    for n, lop in ac.CONFIGS:
        cfg = ac.build(n, lop, counter=True)
        assert all(cfg.type_damage[cfg.agent_type[i]] > 0 for i in range(n))
        words[n, lop] = 2 * sum(int(cfg.n_opponents[cfg.agent_team[i]]) for i in range(n))
    past = sorted(c for c, w in words.items() if w > np_cap)
    assert past == sorted([(n, 0) for n in range(9, 17)] + [(n, 1) for n in range(12, 17)]), words


def test_the_sweep_sees_captures_and_the_last_counter_word(runs):
    for which in ("main", "stagger"):
        assert any(runs[n, 0, which]["captures"] for n in (9, 11, 13, 15)), f"{which}: no capture at an odd N > 8"
        assert any(runs[n, 1, which]["captures"] for n in range(9, 17)), f"{which}: no capture at a lopsided N > 8"
    for n in (10, 15, 16):  # metric 12 of agent N - 1: the word the partial rounds of k_harvest_3 / k_harvest_4 carry
        assert any(runs[n, lop, "stagger"]["last_word"].any() for lop in (0, 1)), n
        taken = [runs[n, lop, "main"]["last_word_at_30"] & runs[n, lop, "main"]["alive_at_30"] for lop in (0, 1)]
        assert all(t.any() for t in taken), n


LIVE_ENVS = (0, 1, 76)  # of the main run's seeds


@pytest.fixture(scope="module")
def reference():
    cwd = os.getcwd()
    before = set(sys.modules)
    Ref, _ = _refimport.import_reference()  # (leaves cwd in the reference: its ctor opens cwd/img/*.png)
    stubs = [m for m in ("IPython", "IPython.display", "seaborn", "imageio", "wandb", "ray") if m not in before]
    yield Ref
    for m in stubs:  # (later test modules must not find the stand-ins: matplotlib asks a loaded IPython for its shell)
        sys.modules.pop(m, None)
    os.chdir(cwd)


@pytest.mark.skipif(not _refimport.available(), reason="the reference is present in the build container only")
@pytest.mark.parametrize("config", ac.CONFIGS, ids=IDS)
def test_oracle_equals_the_live_reference_on_the_sweep(reference, config):
    """Three envs of the main run per config (its seeds, its action stream, its 70 auto-reset steps), the reference driven as
    tests/golden/make_golden_live.py drives it: every step grid, positions, f64 hp, flags, inventory, `_arr`, f64 rewards, done and
    both MT positions, every third step all N observations and metadata rows, at the end counters, visitation maps, captures and
    both generators' whole states.  Where the reference raises (no open respawn cell) the oracle reports CTF_ST_NO_RESPAWN."""
    n, lop = config
    kw = ac.config_kwargs(n, lop)
    cfg = ac.build(n, lop)
    g = cfg.grid_size
    for e in LIVE_ENVS:
        seed = int(ac.seeds()[e])
        ctx = f"{ac.config_id(config)} env {e}"
        random.seed(seed)
        np.random.seed(seed)
        env = reference(**kw)
        teams = [env.AGENT_TEAMS[i] for i in range(n)]
        o = oracle.OracleEnv(cfg)
        o.seed(seed, seed)
        done = False
        for t in range(ac.STEPS):
            actions = oracle.philox_actions(n, ac.ACT_SEED, t, e)
            if done:
                env.reset()
                o.reset()
            try:
                _, rewards, done = env.step([int(a) for a in actions])
            except ValueError:  # the reference's own failure: no open cell round the spawn
                assert o.step(actions)[2] & abi.ST_NO_RESPAWN, (ctx, t)
                break
            rw, dn, status = o.step(actions)
            assert status == 0, (ctx, t, status)
            s = view_arrays(o.get_state(), n, g)
            py, npw = o.get_rng_state()
            want = live.state_digest(env.grid, [list(env.agent_positions[i]) for i in range(n)], [float(env.agent_hp[i]) for i in range(n)],
                                     env.has_flag, [env.block_inventory[i] for i in range(n)], list(env._arr), [float(r) for r in rewards],
                                     done, random.getstate()[1][624], np.random.get_state()[2])
            got = live.state_digest(s["grid"], s["pos"], s["hp"], s["has_flag"], s["inv"], s["perm"], rw, dn, py[624], npw[624])
            assert got == want, f"{ctx} step {t}: grid / positions / hp / flags / inventory / _arr / rewards / done / MT positions"
            if live.observed(t, ac.STEPS):
                want = live.obs_digest(np.stack([env.standardise_state(i, reverse_grid=teams[i] == 1)[0] for i in range(n)]),
                                       np.stack([env.get_env_metadata(i)[0] for i in range(n)]))
                assert live.obs_digest(*o.observe()) == want, f"{ctx} step {t}: observations / metadata"
        else:
            names = abi.METRIC_NAMES
            assert np.array_equal(s["metrics"], np.array([[env.metrics["agent_" + m].get(i, 0) for i in range(n)] for m in names], np.int32)), ctx
            assert np.array_equal(s["visitation"], np.stack([env.metrics["agent_visitation_maps"][i] for i in range(n)]).astype(np.uint8)), ctx
            assert s["team_captures"] == [env.metrics["team_flag_captures"][0], env.metrics["team_flag_captures"][1]], ctx
            st = np.random.get_state()
            assert live.rng_digest(py, npw[:624], npw[624]) == live.rng_digest(random.getstate()[1], st[1], st[2]), ctx

"""The configurations of the agent-count sweep (tests/test_agent_counts_cpu.py, tests/test_gpu_agent_counts.py): for every N in
2..16 an ``even`` config (teams i % 2) and, from N = 3 on, a ``lop`` one (the first max(1, N // 4) agents against the rest), each on
a random map whose grid size varies with N so that GS = G * G rounded up to 16 takes the values 64, 96, 112 and 128.  One
deterministic generator, and the oracle-only runs whose outcome the GPU tests rely on (which envs the oracle itself drops for want
of a respawn cell, how many episodes and captures a config sees): the CPU test asserts those conditions at exactly the env counts,
seeds, action streams and step counts the GPU tests use, so that no GPU test measures its own inputs."""
import numpy as np

import oracle
from _cases import abi, cfgmod, view_arrays
from test_gpu_random_configs import random_scenario

E = 77            # 2 * 32 + 13 = 64 + 13: ragged for the harvest's 32-env waves and for the snapshot's 64-record groups
STEPS = 70        # of the main run: two episodes of GAME_STEPS 30 and ten steps of a third
GAME_STEPS = 30
ACT_SEED = 99
STAGGER_SEED = 0x5747  # bench.stagger_phases' action stream
LANE_E, LANE_STEPS, LANE_SEED, LANE_OFFSET = 65, 40, 0xBEEF, 5  # test_gpu_parity._lane_width_against_oracle's streams
GRIDS = (7, 8, 9, 10, 11)

CONFIGS = [(n, lop) for n in range(2, 17) for lop in (0, 1) if not (lop and n == 2)]
LANE_CONFIGS = [(10, 1), (12, 1), (14, 1), (16, 1), (9, 0), (13, 0), (15, 0)]
COUNTER_N = (3, 6, 12, 15, 16)  # the snapshot also in counter mode
BARE_N = (5, 16)                # ... and with log_metrics off
DIRECT_STEPS, DIRECT_DROP_CAP = 40, 2  # the counter_direct run: one episode and ten steps; the envs a config may lose to a full spawn window


def config_id(c):
    return f"{c[0]}-{'lop' if c[1] else 'even'}"


def grid_size(n, lop):
    if (n, lop) == (16, 0):  # sixteen agents in two even teams on 8 x 8 run out of respawn cells in more than a quarter of the envs
        return 9
    return GRIDS[n % 5]


def teams(n, lop):
    return [0 if i < max(1, n // 4) else 1 for i in range(n)] if lop else [i % 2 for i in range(n)]


def config_kwargs(n, lop):
    """the env kwargs of config (n, lop)"""
    g = grid_size(n, lop)
    rng = np.random.default_rng(7000 + 10 * n + lop)
    scen = random_scenario(rng, g, n)
    t = teams(n, lop)
    return dict(
        SCENARIO=scen, GRID_SIZE=g, AGENT_CONFIG={i: {"team": t[i], "type": int(rng.integers(min(4, n)))} for i in range(n)},  # (type id < N: see wild_config)
        GAME_STEPS=GAME_STEPS, MAP_SYMMETRY_CHECK=False, USE_ADJUSTED_REWARDS=bool(n % 2), HOME_FLAG_CAPTURE=n % 3 == 0,
        DROP_FLAG_WHEN_NO_HP=n % 2 == 0, TAG_PROBABILITY=0.75, AGENT_TYPE_HP={0: 2, 1: 3, 2: 2.5, 3: 1.5},
        AGENT_TYPE_DAMAGE={0: 1, 1: 0.5, 2: 0.75, 3: 1}, VAULT_HP_COST=0.5, VAULT_MIN_HP=0.75, AGENT_HP_HEALING_PER_STEP=0.25,
    )


def build(n, lop, log_metrics=True, counter=False):
    """-> the ctf_config of config (n, lop)"""
    return cfgmod.build_config(config_kwargs(n, lop), log_metrics=log_metrics, rng_mode=abi.RNG_COUNTER if counter else abi.RNG_MT19937)[0]


def seeds(n_envs=E):
    return np.arange(n_envs, dtype=np.uint64) * 31 + 7


def lane_seeds():
    return np.arange(LANE_E, dtype=np.uint64) * 131 + 3  # _lane_width_against_oracle's


def oracles(cfg, seed_list):
    refs = [oracle.OracleEnv(cfg) for _ in seed_list]
    for r, s in zip(refs, seed_list):
        r.seed(int(s), int(s))
    return refs


def lockstep_mask(alive):
    """The mask of the lockstep harvest that isolates the hand-over from batches of eight to single envs: of the envs still followed
    exactly 7 of the first wave's 32 (no batch of eight), exactly 9 of the second's (one batch, then one env), all of the third's."""
    alive = np.asarray(alive, bool)
    mask = np.zeros(E, np.uint8)
    for lo, count in ((0, 7), (32, 9)):
        picked = [e for e in range(lo, lo + 32) if alive[e]][1::2][:count]  # every other one: gaps inside the ballot
        assert len(picked) == count
        mask[picked] = 1
    mask[64:] = alive[64:]
    return mask


def oracle_run(cfg, seed_list, steps, act_seed=ACT_SEED, env_offset=0, stagger=False):
    """The oracle alone over one of the sweep's runs: ``steps`` auto-reset steps of every env on philox_actions(N, act_seed, t,
    env_offset + e), after bench.stagger_phases' prelude when ``stagger``.  An env is dropped at its first non-zero status.
    -> dict: alive bool [E], episodes int [E] (full episodes ended while followed), captures (both teams, over those episodes),
    last_word bool [E] (metric 12 of agent N - 1, the last counter word, was non-zero at an episode end), and for the lockstep
    harvest, which reads the envs after step GAME_STEPS: alive_at_30 and last_word_at_30."""
    n, g, gs = cfg.n_agents, cfg.grid_size, int(cfg.game_steps)
    refs = oracles(cfg, seed_list)
    count = len(refs)
    alive = np.ones(count, bool)
    if stagger:
        for s in range(gs):
            for e, r in enumerate(refs):
                if not alive[e]:
                    continue
                if r.get_state().done:
                    r.reset()
                if r.step(oracle.philox_actions(n, STAGGER_SEED, s, env_offset + e))[2]:
                    alive[e] = False
                if e % gs == s:
                    r.reset()
    episodes, captures, last_word = np.zeros(count, np.int64), 0, np.zeros(count, bool)
    alive_at_30 = last_word_at_30 = None
    for t in range(steps):
        for e, r in enumerate(refs):
            if not alive[e]:
                continue
            if r.get_state().done:
                r.reset()
            _, done, status = r.step(oracle.philox_actions(n, act_seed, t, env_offset + e))
            if status:
                alive[e] = False
            elif done:
                s = view_arrays(r.get_state(), n, g)
                assert s["step_count"] == gs
                episodes[e] += 1
                captures += sum(s["team_captures"])
                last_word[e] |= bool(s["metrics"][abi.N_METRICS - 1][n - 1])
        if t == gs - 1:
            alive_at_30, last_word_at_30 = alive.copy(), last_word.copy()
    return dict(alive=alive, episodes=episodes, captures=int(captures), last_word=last_word, alive_at_30=alive_at_30,
                last_word_at_30=last_word_at_30)

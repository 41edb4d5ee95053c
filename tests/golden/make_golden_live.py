"""The reference on the seeded random configurations of tests/test_oracle_vs_live_reference.py, recorded (live/reference.npz).

Runs where the reference is importable (through _refimport.py):

    python tests/golden/make_golden_live.py

For every block of that test (0-11: capture-dense small maps in the style of make_golden_fuzz.py; wild0-11: tests/_cases.py
wild_config) and every trial of the block, the reference env is driven by the trial's action tape and recorded per step as two 64-bit
digests — the state (grid, positions, f64 hp, flags, inventory, `_arr`, f64 rewards, done, both MT positions) and, every third step
and at the last, all N observations + metadata rows — and at the end of the trial in full: counters, visitation maps, team
captures, and a digest of both generators' whole states.  A trial on which the reference raises (no open respawn cell) records the step.  The
configurations and tapes are functions of the block's seed only (draw_trials), so the test rebuilds them without the reference.
"""
import hashlib
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/ (_cases)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository (the package, oracle)
OUT = os.path.join(HERE, "live", "reference.npz")  # its own folder: every golden/*.npz is a trajectory case (tests/_cases.py)
BLOCKS = list(range(12)) + [f"wild{k}" for k in range(12)]
TRIALS = 10


def _random_case(rng):
    import make_golden_fuzz as mgf

    scen, agents = mgf.random_scenario(rng, "Live")
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]
    hp = pick([0.25, 0.5, 1.0])
    kw = dict(GRID_SIZE=scen["GRID_SIZE"], AGENT_CONFIG=agents, GAME_STEPS=int(rng.integers(40, 121)), MAP_SYMMETRY_CHECK=False,
              HOME_FLAG_CAPTURE=bool(rng.integers(0, 2)), DROP_FLAG_WHEN_NO_HP=bool(rng.integers(0, 2)),
              USE_ADJUSTED_REWARDS=bool(rng.integers(0, 2)), TAG_PROBABILITY=pick([0.2, 0.5, 0.9, 1.0]),
              AGENT_TYPE_HP={0: 10 * hp, 1: 8 * hp, 2: 8 * hp, 3: 7 * hp}, AGENT_TYPE_DAMAGE={0: 1, 1: 0.5, 2: 0.5, 3: 1},
              GUARDIAN_DAMAGE_MULTIPLIER=pick([1.0, 5.0]), VAULT_HP_COST=pick([0.25, 1.25]), VAULT_MIN_HP=pick([0.5, 2.5]),
              AGENT_HP_HEALING_PER_STEP=pick([0.0, 0.1, 0.25]))
    return scen, kw


def draw_trials(block):
    """-> [(trial, scenario, kwargs, seed, actions int8 [T, n])] of one block, from the block's seed alone."""
    from _cases import wild_config

    wild = isinstance(block, str)
    rng = np.random.default_rng(888_000 + int(block[4:])) if wild else np.random.default_rng(777_000 + block)
    out = []
    for trial in range(TRIALS):
        drawn = wild_config(rng) if wild else _random_case(rng)
        if drawn is None:
            continue
        scen, kw = drawn
        seed = int(rng.integers(0, 2 ** 31))
        n = len(kw["AGENT_CONFIG"])
        T = kw["GAME_STEPS"] + 5
        actions = np.where(rng.random((T, n)) < 0.15, rng.integers(5, 9, (T, n)), rng.integers(0, 5, (T, n))).astype(np.int8)
        out.append((trial, scen, kw, seed, actions))
    return out


def _digest(*arrays):
    h = hashlib.blake2b(digest_size=8)
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint64)[0]


def state_digest(grid, pos, hp, has_flag, inv, perm, rewards, done, py_pos, np_pos):
    return _digest(np.asarray(grid, np.uint8), np.asarray(pos, np.int8), np.asarray(hp, np.float64), np.asarray(has_flag, np.uint8),
                   np.asarray(inv, np.int32), np.asarray(perm, np.uint8), np.asarray(rewards, np.float64), np.uint8(done),
                   np.int64(py_pos), np.int64(np_pos))


def obs_digest(obs, meta):
    return _digest(np.asarray(obs, np.uint8), np.asarray(meta, np.float16).view(np.uint16))


def rng_digest(py_words, np_key, np_pos):
    """Both generators' whole states: random's 624 words + position, np.random's 624 words + position."""
    return _digest(np.asarray(py_words, np.uint32), np.asarray(np_key, np.uint32), np.int64(np_pos))


def observed(t, T):
    return t % 3 == 0 or t == T - 1


def key(block, trial, what):
    return f"b{block}_t{trial}_{what}"


def record_block(Ref, block, metric_names):
    rec = {}
    for trial, scen, kw, seed, actions in draw_trials(block):
        n, T = len(kw["AGENT_CONFIG"]), len(actions)
        random.seed(seed)
        np.random.seed(seed)
        env = Ref(SCENARIO=scen, **kw)
        teams = [env.AGENT_TEAMS[i] for i in range(n)]
        rec[key(block, trial, "tiles_used")] = np.array([int(x) for x in env.TILES_USED], np.int32)
        states, views, raised = [], [], -1
        for t in range(T):
            try:
                _, rewards, done = env.step([int(a) for a in actions[t]])
            except ValueError:  # the reference's own failure: no open cell round the spawn
                raised = t
                break
            states.append(state_digest(env.grid, [list(env.agent_positions[i]) for i in range(n)], [float(env.agent_hp[i]) for i in range(n)],
                                       env.has_flag, [env.block_inventory[i] for i in range(n)], list(env._arr),
                                       [float(r) for r in rewards], done, random.getstate()[1][624], np.random.get_state()[2]))
            if observed(t, T):
                views.append(obs_digest(np.stack([env.standardise_state(i, reverse_grid=teams[i] == 1)[0] for i in range(n)]),
                                        np.stack([env.get_env_metadata(i)[0] for i in range(n)])))
        rec[key(block, trial, "raised")] = np.int32(raised)
        rec[key(block, trial, "states")] = np.array(states, np.uint64)
        rec[key(block, trial, "views")] = np.array(views, np.uint64)
        if raised < 0:
            rec[key(block, trial, "metrics")] = np.array([[env.metrics["agent_" + name].get(i, 0) for i in range(n)] for name in metric_names],
                                                         np.int32)
            rec[key(block, trial, "visitation")] = np.stack([env.metrics["agent_visitation_maps"][i] for i in range(n)]).astype(np.int32)
            rec[key(block, trial, "team_captures")] = np.array([env.metrics["team_flag_captures"][0], env.metrics["team_flag_captures"][1]],
                                                               np.int32)
            st = np.random.get_state()
            rec[key(block, trial, "rng_states")] = np.array([rng_digest(random.getstate()[1], st[1], st[2])], np.uint64)
    return rec


def main():
    import _refimport
    from _cases import abi

    cwd = os.getcwd()
    Ref, _ = _refimport.import_reference()  # (leaves cwd in the reference: its ctor opens cwd/img/*.png)
    rec = {}
    for block in BLOCKS:
        rec.update(record_block(Ref, block, abi.METRIC_NAMES))
    os.chdir(cwd)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: {len(rec)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

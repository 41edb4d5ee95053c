"""TEST INFRASTRUCTURE: the crafted-generator cases of tests/test_rng_edges_cpu.py and tests/test_gpu_rng_edges.py, and the
ORACLE-FIRST GATE every one of them passes before a device sees it.

A case is a configuration, one generator state (or counter pair) per env, and a number of steps under the synthetic Philox action
stream.  ``oracle_gate(case)`` steps the C oracle through it and returns what the device is then compared with; it refuses a case in
which the oracle reports a status it may not, or in which a step draws 400 words of np.random or 200 of random: py_shuffle and
np_randint loop until a word is accepted, so a state that rejects without end must never reach a kernel.  (Both bounds are far
inside the 624 words a step may draw; a crafted run of rejections always ends inside its block, on ordinary words.)"""
import functools
from types import SimpleNamespace

import numpy as np

import oracle
from _cases import Case, abi, cfgmod, view_arrays
from _mt_craft import (MT_N, at_position, np_block_at_threshold, np_block_with_outputs, p_above, p_equal, py_rejection_run, seeded_np,
                       seeded_py, untwist)

ACT_SEED = 0x51ED
MAX_NP_WORDS, MAX_PY_WORDS = 400, 200  # per step, exclusive
TAG_COUNT = abi.METRIC_NAMES.index("tag_count")
VIEW_KEYS = ("grid", "pos", "hp", "has_flag", "inv", "perm", "metrics", "visitation", "step_count", "done", "team_captures")


def make_case(name, kwargs, steps, py_states=None, np_states=None, counters=None, seeds=None, allow_status=0):
    n_envs = len(py_states if py_states is not None else counters)
    return SimpleNamespace(name=name, kwargs=kwargs, steps=steps, n_envs=n_envs, allow_status=allow_status, seeds=seeds,
                           py_states=None if py_states is None else np.ascontiguousarray(py_states, dtype=np.uint32),
                           np_states=None if np_states is None else np.ascontiguousarray(np_states, dtype=np.uint32),
                           counters=None if counters is None else np.ascontiguousarray(counters, dtype=np.uint64),
                           rng_mode="counter" if counters is not None else "mt19937")


# ---- 3a: the threshold edge of the hit bit ------------------------------------------------------------------------------------------
THRESHOLDS = (0x5555555, 1, (1 << 27) - 2)
DENSE_ENVS, DENSE_STEPS = 64, 2
DENSE_MAP_SEED = 4


def dense_kwargs(tag_probability):
    """5 x 5, 2 v 2, every type deals damage, one hp: agents stand next to each other from the first step and a tag is a respawn (a
    randint).  The map: tests/test_gpu_random_configs.random_scenario, its seed chosen with the oracle alone."""
    from test_gpu_random_configs import random_scenario

    scen = random_scenario(np.random.default_rng(DENSE_MAP_SEED), 5, 4)
    return dict(SCENARIO=scen, AGENT_CONFIG={i: {"team": i % 2, "type": i} for i in range(4)}, GAME_STEPS=30, MAP_SYMMETRY_CHECK=False,
                TAG_PROBABILITY=tag_probability, AGENT_TYPE_HP={0: 1, 1: 1.5, 2: 1, 3: 0.5}, AGENT_TYPE_DAMAGE={0: 1, 1: 0.5, 2: 0.75, 3: 1},
                VAULT_HP_COST=0.5, VAULT_MIN_HP=0.75, AGENT_HP_HEALING_PER_STEP=0.25)


def _dense_py_states():
    return np.stack([seeded_py(4000 + e) for e in range(DENSE_ENVS)])


@functools.lru_cache(maxsize=None)
def threshold_case(th, which):
    """every rand() of env e's np.random block is p_equal(th); TAG_PROBABILITY is that (`equal`: all miss) or one unit of 2^-53 more
    (`above`: all hit).  Env e starts at position e, with its own low bits."""
    rng = np.random.default_rng(th)
    np_states = np.stack([at_position(np.append(np_block_at_threshold(th, rng), 0), e) for e in range(DENSE_ENVS)])
    p = dict(equal=p_equal, above=p_above)[which](th)
    return make_case(f"threshold {th:#x} {which}", dense_kwargs(p), DENSE_STEPS, _dense_py_states(), np_states)


@functools.lru_cache(maxsize=None)
def end_case(which):
    """the two ends of the compare: the smallest draw (0) under the smallest probability (2^-53) hits, the largest draw
    (1 - 2^-53) under the largest probability below 1 misses.  Ordinary blocks, crafted at the words the two steps draw."""
    value, p = dict(lowest=(0, 2.0 ** -53), highest=(0xFFFFFFFF, 1.0 - 2.0 ** -53))[which]
    np_states = np.stack([at_position(np.append(np_block_with_outputs(seeded_np(7000 + e), e, 128, value), 0), e) for e in range(DENSE_ENVS)])
    return make_case(f"end {which}", dense_kwargs(p), DENSE_STEPS, _dense_py_states(), np_states)


TWISTED_STEPS = 4


@functools.lru_cache(maxsize=None)
def twisted_threshold_case(th, which):
    """The same edge on a block the STEP LAUNCHES make.  An import digests the block it is handed and the one after it (k_rng_refill),
    so env e is handed the block TWO before a threshold block (_mt_craft.untwist, twice), 3 + e % 29 words before its end, on the
    8 x 8 map with 8 v 8 agents (~260 np.random words per step): step one moves into the middle block, step three or four into the
    threshold block — the real twist of the twist of what was handed over, regenerated and digested by a tail block of k_step or, when
    there are none, by the one-lane safety net of the step that needs it."""
    from test_gpu_random_configs import config_kwargs

    rng = np.random.default_rng(th + 1)
    np_states = []
    for e in range(DENSE_ENVS):
        middle = untwist(np_block_at_threshold(th, rng), reachable=True)[0]
        np_states.append(at_position(np.append(untwist(middle)[0], 0), MT_N - 3 - e % 29))
    p = dict(equal=p_equal, above=p_above)[which](th)
    kwargs = dict(config_kwargs(8, 16), TAG_PROBABILITY=p)
    return make_case(f"twisted threshold {th:#x} {which}", kwargs, TWISTED_STEPS, _dense_py_states(), np.stack(np_states), allow_status=abi.ST_NO_RESPAWN)


# ---- 3b: every start position -------------------------------------------------------------------------------------------------------
SWEEP_ENVS = MT_N + 1


def _sweep_states(seed_base):
    py = np.stack([at_position(seeded_py(seed_base + e), e) for e in range(SWEEP_ENVS)])
    npw = np.stack([at_position(seeded_np(seed_base + e), (233 * e) % SWEEP_ENVS) for e in range(SWEEP_ENVS)])
    return py, npw


@functools.lru_cache(maxsize=None)
def sweep_arena_case(steps=12):
    """arena_stress, 625 envs: env e's `random` generator stands at position e, its np.random generator at (233 e) mod 625"""
    py, npw = _sweep_states(90_000)
    return make_case(f"sweep arena {steps}", Case("arena_stress").kwargs, steps, py, npw)


@functools.lru_cache(maxsize=None)
def sweep_8v8_case(steps=6, seed_base=50_000):
    """the same sweep on the 8 x 8 map with 8 v 8 agents of tests/test_gpu_random_configs.CASES: ~260 np.random words per step"""
    from test_gpu_random_configs import config_kwargs

    py, npw = _sweep_states(seed_base)
    return make_case(f"sweep 8v8 {steps}", config_kwargs(8, 16), steps, py, npw, allow_status=abi.ST_NO_RESPAWN)


# ---- 3c: rejection runs in the shuffle -----------------------------------------------------------------------------------------------
REJECTION_SPECS = ((100, 10), (100, 70), (560, 70), (600, 30), (623, 5), (624, 3), (3, 61), (2, 62), (1, 63))
REJECTION_ENVS = 48


@functools.lru_cache(maxsize=None)
def rejection_case(specs=REJECTION_SPECS):
    """arena_stress, 48 envs: env e's `random` generator is _mt_craft.py_rejection_run(seed 3000 + e, *specs[e % len(specs)]); one step
    on the crafted words, three more on ordinary ones"""
    py = np.stack([at_position(np.append(py_rejection_run(seeded_py(3000 + e), *specs[e % len(specs)]), 0), specs[e % len(specs)][0])
                   for e in range(REJECTION_ENVS)])
    npw = np.stack([seeded_np(3000 + e) for e in range(REJECTION_ENVS)])
    return make_case(f"rejection {specs}", Case("arena_stress").kwargs, 4, py, npw)


# ---- 3e: counters --------------------------------------------------------------------------------------------------------------------
COUNTER_KS = (0, 1, 7, 1 << 33)


@functools.lru_cache(maxsize=None)
def counter_case(k):
    """counter mode, arena_stress, 625 envs: the `random` tape at word 624 k + e, the np.random tape at 624 k' + (233 e) mod 625 with
    k' the next entry of COUNTER_KS — every offset into a block, 0 and the block boundary itself (e = 624: word 0 of block k + 1)"""
    k2 = COUNTER_KS[(COUNTER_KS.index(k) + 1) % len(COUNTER_KS)]
    e = np.arange(SWEEP_ENVS, dtype=np.uint64)
    counters = np.stack([np.uint64(MT_N * k) + e, np.uint64(MT_N * k2) + (np.uint64(233) * e) % np.uint64(SWEEP_ENVS)], axis=1)
    py_seeds = e * np.uint64(0x9E3779B97F4A7C15) + np.uint64(77)  # any 64-bit values
    seeds = np.stack([py_seeds, py_seeds ^ np.uint64(0xABCDEF0123456789)], axis=1)
    return make_case(f"counters k={k}", Case("arena_stress").kwargs, 8, counters=counters, seeds=seeds)


# ---- the gate -------------------------------------------------------------------------------------------------------------------------
def case_config(case):
    return cfgmod.build_config(case.kwargs, log_metrics=True, rng_mode=abi.RNG_COUNTER if case.rng_mode == "counter" else abi.RNG_MT19937)[0]


def words_drawn(before, after):
    """words a step consumed from a generator that went from position `before` to `after` (fewer than 624: the gate's bounds)"""
    return after - before if after >= before else MT_N - before + after


_RUNS = {}


def oracle_gate(case):
    """Steps the oracle through `case` and returns the reference of the device run (computed once per case):
    rewards f64 [T, E, N], done u8 [T, E], live bool [T, E] (env e's step t counts: it has not run out of respawn cells),
    start_py / start_np i64 [T, E] (positions, or counters, before step t), words_py / words_np i64 [T, E], counters u64 [T, E, 2]
    (counter mode, after step t), tags i64 [E] (the tag_count metric at the end), views (view_arrays of every env at the end),
    py_final / np_final u32 [E, 625].
    Asserts the gate's conditions: no status outside case.allow_status, fewer than 400 / 200 words per step."""
    if case.name not in _RUNS:
        _RUNS[case.name] = _run_oracle(case)
    return _RUNS[case.name]


def _run_oracle(case):
    cfg = case_config(case)
    E, T, N, G = case.n_envs, case.steps, cfg.n_agents, cfg.grid_size
    counter = case.rng_mode == "counter"
    refs = [oracle.OracleEnv(cfg) for _ in range(E)]
    for e, r in enumerate(refs):
        if counter:
            r.seed(int(case.seeds[e, 0]), int(case.seeds[e, 1]))
            r.set_rng_counters(int(case.counters[e, 0]), int(case.counters[e, 1]))
        else:
            r.set_rng_state(case.py_states[e], case.np_states[e])

    def where(r):
        if counter:
            return r.get_rng_counters()
        a, b = r.get_rng_state()
        return int(a[MT_N]), int(b[MT_N])

    out = SimpleNamespace(rewards=np.zeros((T, E, N), np.float64), done=np.zeros((T, E), np.uint8), live=np.zeros((T, E), bool),
                          start_py=np.zeros((T, E), np.int64), start_np=np.zeros((T, E), np.int64), words_py=np.zeros((T, E), np.int64),
                          words_np=np.zeros((T, E), np.int64), counters=np.zeros((T, E, 2), np.uint64))
    alive = np.ones(E, bool)
    for t in range(T):
        for e, r in enumerate(refs):
            if not alive[e]:
                continue
            if r.get_state().done:
                r.reset()
            b_py, b_np = where(r)
            rw, dn, status = r.step(oracle.philox_actions(N, ACT_SEED, t, e))
            a_py, a_np = where(r)
            d_py, d_np = (a_py - b_py, a_np - b_np) if counter else (words_drawn(b_py, a_py), words_drawn(b_np, a_np))
            ctx = f"{case.name}: env {e} step {t}"
            assert status & ~case.allow_status == 0, f"{ctx}: oracle status {status}"
            assert d_np < MAX_NP_WORDS and d_py < MAX_PY_WORDS, f"{ctx}: {d_py} words of random, {d_np} of np.random in one step"
            out.start_py[t, e], out.start_np[t, e], out.words_py[t, e], out.words_np[t, e] = b_py, b_np, d_py, d_np
            if status:
                alive[e] = False
                continue
            out.live[t, e], out.rewards[t, e], out.done[t, e] = True, rw, dn
            if counter:
                out.counters[t, e] = (a_py, a_np)
    out.alive = alive
    out.views = [view_arrays(r.get_state(), N, G) for r in refs]
    out.tags = np.array([v["metrics"][TAG_COUNT].sum() for v in out.views], np.int64)
    if not counter:
        states = [r.get_rng_state() for r in refs]
        out.py_final, out.np_final = np.stack([s[0] for s in states]), np.stack([s[1] for s in states])
    return out


def crossed(run, stream):
    """bool [T, E]: the step drew from the block after the one it started in (MT19937 mode)"""
    start, words = (run.start_py, run.words_py) if stream == "py" else (run.start_np, run.words_np)
    return run.live & (start + words > MT_N)


# ---- what the cases must reach, computed from the oracle's positions ------------------------------------------------------------------
def np_pairs(cfg):
    """rand() draws per step: one per opponent of every agent whose type deals damage (ctf_derive.h: np_pairs)"""
    return sum(cfg.n_opponents[cfg.agent_team[i]] for i in range(cfg.n_agents) if cfg.type_damage[cfg.agent_type[i]] > 0)


def check_threshold(run_equal, run_above, pairs):
    """`equal`: no rand() is below the probability it equals — no tag, no respawn, 2 * pairs words per step; `above`: tags"""
    assert not run_equal.tags.any(), f"{int(run_equal.tags.sum())} tags although every rand() equals TAG_PROBABILITY"
    assert run_above.tags.sum() > 0, "no tag although every rand() is below TAG_PROBABILITY"
    assert (run_equal.words_np == 2 * pairs).all() and (run_above.words_np >= 2 * pairs).all()
    untagged = run_above.tags == 0  # the same trajectory under either probability: a hit on an agent out of reach changes nothing
    assert (run_above.words_np[:, untagged] == run_equal.words_np[:, untagged]).all()


def check_twisted(run_equal, run_above):
    """the last step starts inside the threshold block, two blocks on from the one handed over; there `equal` tags nobody"""
    for run in (run_equal, run_above):
        assert (run.start_np[-1] < run.start_np[-2]).all() and (run.start_np[1] < run.start_np[0]).all()
    live = run_equal.live[-1]
    assert live.sum() >= live.size // 2 and (run_equal.words_np[-1][live] == run_equal.words_np[-1][live].min()).all()  # no respawn: no tag
    assert run_above.tags.sum() > run_equal.tags.sum()


def check_sweep_coverage(case, run, min_crossing=150):
    """the start positions reach every alignment of the three digest windows at the end of a block, and enough envs go over it"""
    cfg = case_config(case)
    s_np, s_py = run.start_np[0], run.start_py[0]
    near_np, near_py = s_np >= MT_N - 2 * np_pairs(cfg), s_py >= MT_N - (cfg.n_agents - 1)
    assert sorted(s_np[near_np]) == list(range(MT_N - 2 * np_pairs(cfg), MT_N + 1)) and sorted(s_py[near_py]) == list(range(MT_N - cfg.n_agents + 1, MT_N + 1))
    assert (s_np + run.words_np[0] >= MT_N)[near_np & run.live[0]].all(), "an np.random generator near the end of its block did not leave it in step one"
    assert (s_py + run.words_py[0] >= MT_N)[near_py & run.live[0]].all(), "a random generator near the end of its block did not leave it in step one"
    assert len(set(s_np[near_np] % 32)) == 32 and len(set(s_np[near_np] % 8)) == 8 and len(set(s_py[near_py] % 4)) == 4
    n_np, n_py = int(crossed(run, "np").any(0).sum()), int(crossed(run, "py").any(0).sum())
    assert n_np >= min_crossing and n_py >= min_crossing, f"{n_np} envs cross a seam of np.random, {n_py} of random: fewer than {min_crossing}"


def check_second_hop(run, mirror=208):
    """a step reads a hit bit past the mirror behind its ring's digests: stream_slow's hop into the other ring's own array"""
    reach = np.where(run.live, run.start_np + run.words_np, 0)
    assert reach.max() > MT_N + mirror, f"no step draws past position {MT_N + mirror} of its block (furthest: {int(reach.max())})"


def check_rejection_reach(run, window=64):
    """a crafted step draws more `random` words than the top-byte window holds: the shuffle's slow path"""
    assert run.words_py[0].max() > window, f"the crafted step draws at most {int(run.words_py[0].max())} words of random: inside the {window}-byte window"

"""A plain restatement of the action-effect rule (include/ctf_env.h, ctf_action_effects; csrc/ctf_effects.h): one agent and one
action at a time, written from the reference's ``act`` (gridworld_ctf.py:700-732 and the helpers it calls, :569-690), with tuples,
dicts and early returns — no packed words, no clamped loads — plus the sampler of ctf_random_effective_actions on tests/_philox.py.
What tests/test_effects_cpu.py holds the header's host form to, and tests/test_gpu_effects.py the kernels."""
import numpy as np

import _philox

MOVES, JUMPS, PICKS_UP, CAPTURES, MINES, BREAKS, LAYS = 1, 2, 4, 8, 16, 32, 64
EFFECT_TAG = 0x45464631  # "EFF1"
N_ACTIONS = 9
UNIT = {0: (-1, 0), 1: (1, 0), 2: (0, 1), 3: (0, -1)}
# the effect bytes the rule can produce: JUMPS, PICKS_UP, CAPTURES only with MOVES; BREAKS only with MINES; MOVES, MINES, LAYS exclusive
VALID = frozenset([0, LAYS, MINES, MINES | BREAKS] + [MOVES | j | p | c for j in (0, JUMPS) for p in (0, PICKS_UP) for c in (0, CAPTURES)])


def delta(agent_type, action):
    """ACTION_DELTAS (:100-145): None where the action aims nowhere"""
    if action <= 3:
        return UNIT[action]
    if action == 4 or agent_type in (0, 1):
        return None
    dr, dc = UNIT[action - 5]
    return (2 * dr, 2 * dc) if agent_type == 2 else (dr, dc)


def cheb(a, b):
    return max(abs(a[0] - b[0]), abs(a[1] - b[1]))


def effect(rules, st, i, action):
    """``rules``: dict(teams, types, flag_pos, spawn_pos, home_flag_capture, vault_cost, vault_min); ``st``: dict(grid, pos, hp,
    has_flag, inv) of one env -> the flag byte of act(i, action) on the state as it stands"""
    grid = np.asarray(st["grid"])
    g = grid.shape[0]
    me = (int(st["pos"][i][0]), int(st["pos"][i][1]))
    team, kind = rules["teams"][i], rules["types"][i]
    d = delta(kind, action)
    if d is None or not (0 <= me[0] < g and 0 <= me[1] < g):
        return 0
    to = (me[0] + d[0], me[1] + d[1])
    if not (0 <= to[0] < g and 0 <= to[1] < g):
        return 0
    tile = int(grid[to])
    vault = action >= 5 and kind == 2 and (float(st["hp"][i]) - rules["vault_cost"]) > rules["vault_min"]
    if tile == 0 and (action <= 3 or vault):
        out = MOVES | (JUMPS if action >= 5 else 0)
        other, home = tuple(rules["flag_pos"][1 - team]), tuple(rules["flag_pos"][team])
        carrying = bool(st["has_flag"][i])
        if cheb(to, other) <= 1 and int(grid[other]) == 12 + (1 - team):
            out |= PICKS_UP
            carrying = True
        if cheb(to, home) <= 1 and carrying and (not rules["home_flag_capture"] or int(grid[home]) == 12 + team):
            out |= CAPTURES
        return out
    if kind != 3:
        return 0
    if action >= 5:
        ok = int(st["inv"][i]) > 0 and tile == 0 and all(cheb(to, tuple(rules["spawn_pos"][t])) > 1 for t in (0, 1))
        return LAYS if ok else 0
    if tile == 2:
        return MINES
    if tile == 3:
        return MINES | BREAKS
    return 0


def env_effects(rules, st):
    """-> (mask uint16 [N], effects uint8 [N, 9]) of one env"""
    n = len(rules["teams"])
    eff = np.array([[effect(rules, st, i, a) for a in range(N_ACTIONS)] for i in range(n)], np.uint8)
    return pack_mask(eff), eff


def pack_mask(eff):
    """effects uint8 [..., 9] -> uint16 [...]: bit a = (effect a != 0)"""
    return ((np.asarray(eff) != 0).astype(np.uint16) << np.arange(N_ACTIONS, dtype=np.uint16)).sum(axis=-1).astype(np.uint16)


def cfg_rules(cfg):
    """the rule's constants from a ctf_config"""
    n = cfg.n_agents
    cell = lambda p: (int(p[0]), int(p[1]))
    return dict(teams=[int(cfg.agent_team[i]) for i in range(n)], types=[int(cfg.agent_type[i]) for i in range(n)],
                flag_pos=[cell(cfg.flag_pos[t]) for t in (0, 1)], spawn_pos=[cell(cfg.spawn_pos[t]) for t in (0, 1)],
                home_flag_capture=bool(cfg.home_flag_capture), vault_cost=float(cfg.vault_hp_cost), vault_min=float(cfg.vault_min_hp))


def sample(mask, seed, env, step, agent):
    """ctf_random_effective_actions' draw for one agent: ``mask`` its 9-bit mask, ``env`` the env's global index"""
    bits = [a for a in range(N_ACTIONS) if (int(mask) >> a) & 1]
    if not bits:
        return 4
    seed = int(seed)
    w0 = int(_philox.philox4x32_10((env, step, agent, EFFECT_TAG), (seed & 0xFFFFFFFF, seed >> 32))[0])
    return bits[(w0 * len(bits)) >> 32]


def sample_env(mask, seed, env, step, agent_mask, out):
    """one env: out[i] = the draw of every agent of ``agent_mask``; the other entries of ``out`` stay"""
    for i in range(len(mask)):
        if (agent_mask >> i) & 1:
            out[i] = sample(mask[i], seed, env, step, i)
    return out

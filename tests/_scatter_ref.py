"""A plain restatement of the scattered reset's placement (include/ctf_env.h, ctf_reset_scattered), written from the header's text on
tests/_philox.py: ``place_one`` is the rule one env and one agent at a time, with lists and a set; ``place`` is the same rule for a
batch of envs at once (NumPy over the env axis) — tests/test_scatter_cpu.py holds the two to each other — and ``state`` / ``visitation``
build what the env then holds.  What the CPU test holds the host form of csrc/ctf_scatter.h to, and tests/test_gpu_scatter.py the kernel."""
import numpy as np

import _philox

SCATTER_TAG = 0x53435431  # "SCT1"
OWN_SIDE = 1
U32 = 0xFFFFFFFF


def cheb(a, b):
    return max(abs(a[0] - b[0]), abs(a[1] - b[1]))


def cfg_rules(cfg):
    """the rule's constants from a ctf_config"""
    n, g = cfg.n_agents, cfg.grid_size
    cell = lambda p: (int(p[0]), int(p[1]))
    return dict(n=n, g=g, init=np.array(cfg.init_grid[:g * g], np.uint8).reshape(g, g), starts=[cell(cfg.start_pos[i]) for i in range(n)],
                teams=[int(cfg.agent_team[i]) for i in range(n)], flags=[cell(cfg.flag_pos[t]) for t in (0, 1)])


def candidates(rules, i, radius, own_side):
    """C_i before anything is taken: ascending row-major cell indices"""
    g, s, t = rules["g"], rules["starts"][i], rules["teams"][i]
    out = []
    for r in range(g):
        for c in range(g):
            if (r, c) == s:
                out.append(r * g + c)
            elif rules["init"][r, c] == 0 and cheb((r, c), s) <= radius and (not own_side or cheb((r, c), rules["flags"][t]) <= cheb((r, c), rules["flags"][1 - t])):
                out.append(r * g + c)
    return out


def word(seed, env, r, agent):
    seed = int(seed)
    return int(_philox.philox4x32_10((env & U32, r & U32, agent, SCATTER_TAG), (seed & U32, seed >> 32))[0])


def place_one(rules, agent_mask, radius, own_side, seed, env, r):
    """one env (``env`` its GLOBAL index, ``r`` = (round + episode) mod 2^32) -> [cell index of agent i]"""
    g, taken, cells = rules["g"], set(), []
    for i in range(rules["n"]):
        s = rules["starts"][i][0] * g + rules["starts"][i][1]
        cell = s
        if (agent_mask >> i) & 1:
            cand = [c for c in candidates(rules, i, radius, own_side) if c not in taken]
            cell = cand[(word(seed, env, r, i) * len(cand)) >> 32]
        taken.add(cell)
        cells.append(cell)
    return cells


def place(rules, agent_mask, radius, own_side, seed, envs, rounds):
    """``envs`` GLOBAL env indices [E], ``rounds`` scalar or [E] (round + episode, wrapped here) -> cells int64 [E, N]"""
    n, g = rules["n"], rules["g"]
    envs = np.asarray(envs, np.uint64) & np.uint64(U32)
    rounds = np.broadcast_to(np.asarray(rounds, np.uint64) & np.uint64(U32), envs.shape)
    seed = int(seed)
    taken = np.zeros((len(envs), g * g), bool)
    cells = np.zeros((len(envs), n), np.int64)
    rows = np.arange(len(envs))
    for i in range(n):
        s = rules["starts"][i][0] * g + rules["starts"][i][1]
        cell = np.full(len(envs), s, np.int64)
        if (agent_mask >> i) & 1:
            cand = np.zeros(g * g, bool)
            cand[candidates(rules, i, radius, own_side)] = True
            avail = cand[None, :] & ~taken
            count = avail.sum(axis=1).astype(np.uint64)
            w0 = _philox.philox4x32_10((envs, rounds, i, SCATTER_TAG), (seed & U32, seed >> 32))[0].astype(np.uint64)
            k = (w0 * count) >> np.uint64(32)
            cell = ((np.cumsum(avail, axis=1) == (k + np.uint64(1))[:, None].astype(np.int64)) & avail).argmax(axis=1)
        taken[rows, cell] = True
        cells[:, i] = cell
    return cells


def state(rules, cells):
    """cells [N] of one env -> (grid uint8 [G, G], pos int8 [N, 2]) after the placement"""
    g = rules["g"]
    grid = rules["init"].copy()
    for i, cell in enumerate(cells):
        s = rules["starts"][i]
        grid[s] = 0
        grid[int(cell) // g, int(cell) % g] = rules["init"][s]
    return grid, np.array([[int(c) // g, int(c) % g] for c in cells], np.int8)


def visitation(rules, cells):
    """the maps of one env at step 0: uint8 [N, G, G], 1 at each agent's cell"""
    g = rules["g"]
    out = np.zeros((rules["n"], g, g), np.uint8)
    for i, cell in enumerate(cells):
        out[i, int(cell) // g, int(cell) % g] = 1
    return out

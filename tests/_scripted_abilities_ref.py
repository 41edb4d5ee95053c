"""An independent restatement of the scripted ABILITIES (include/ctf_env.h, ctf_scripted_abilities): one agent at a time, a heapq
Dijkstra over a 2-D list for the digger, a queue breadth-first search with eight moves for the vaulter, no bit masks.  The roles, the
goal sets, who is decided before the search and the exploration rule are those of tests/_scripted_roles_ref.py.  What
tests/test_scripted_abilities_cpu.py holds csrc/ctf_scripted.h to, and tests/test_gpu_scripted_abilities.py the kernel."""
import heapq
from collections import deque

import numpy as np

import _scripted_ref as ref
import _scripted_roles_ref as rr

WALKER, DIGGER, VAULTER = 0, 1, 2
CLASS_NAMES = {WALKER: "walker", DIGGER: "digger", VAULTER: "vaulter"}
ENTRY_COST = {0: 1, 3: 2, 2: 3}  # OPEN; DESTRUCTIBLE_TILE2: one hit, then the move; DESTRUCTIBLE_TILE1: two hits, then the move
JUMPS = {5: (-2, 0), 6: (2, 0), 7: (0, 2), 8: (0, -2)}
VAULT_MOVES = tuple(enumerate(ref.DELTAS)) + tuple(sorted(JUMPS.items()))  # in the order of the action numbers: 0, 1, 2, 3, 5, 6, 7, 8


def agent_class(agent_type, hp, ability, vault_cost, vault_min):
    """the movement class of an agent from its type, its hp (np.float64) and its ability bit"""
    if not ability:
        return WALKER
    if agent_type == 3:
        return DIGGER
    if agent_type == 2 and (np.float64(hp) - np.float64(vault_cost)) > np.float64(vault_min):
        return VAULTER
    return WALKER


def dig_distances(grid, goals):
    """D over the cells a digger may enter (tiles 0, 2, 3) to those of ``goals`` it may enter: the least sum of entry costs, the goal
    cell's own counted, the start cell's not; D of a goal cell is 0; -1 = not reachable / a wall"""
    cells = np.asarray(grid).tolist()
    g = len(cells)
    d = [[-1] * g for _ in range(g)]
    heap = []
    for r, c in sorted(goals):
        if 0 <= r < g and 0 <= c < g and cells[r][c] in ENTRY_COST:
            d[r][c] = 0
            heap.append((0, r, c))
    heapq.heapify(heap)
    done = set()
    while heap:
        dist, r, c = heapq.heappop(heap)
        if (r, c) in done:
            continue
        done.add((r, c))
        step = dist + ENTRY_COST[cells[r][c]]  # a neighbour's path enters (r, c) first
        for dr, dc in ref.DELTAS:
            rr_, cc = r + dr, c + dc
            if 0 <= rr_ < g and 0 <= cc < g and cells[rr_][cc] in ENTRY_COST and (d[rr_][cc] < 0 or step < d[rr_][cc]):
                d[rr_][cc] = step
                heapq.heappush(heap, (step, rr_, cc))
    return d


def dig_towards(grid, d, p):
    """the lowest-numbered of 0..3 whose neighbour n of ``p`` has the minimum finite w(n) + D(n); none: 4"""
    cells = np.asarray(grid).tolist()
    g = len(d)
    best, act = None, 4
    for k, (dr, dc) in enumerate(ref.DELTAS):
        r, c = int(p[0]) + dr, int(p[1]) + dc
        if 0 <= r < g and 0 <= c < g and d[r][c] >= 0:
            cost = ENTRY_COST[cells[r][c]] + d[r][c]
            if best is None or cost < best:
                best, act = cost, k
    return act


def vault_distances(grid, goals):
    """d over the OPEN cells with the four unit moves and the four jumps, every move 1 (a jump needs its landing cell open, whatever
    it passes over); -1 = not reachable / a wall"""
    cells = np.asarray(grid).tolist()
    g = len(cells)
    d = [[-1] * g for _ in range(g)]
    queue = deque()
    for r, c in sorted(goals):
        if 0 <= r < g and 0 <= c < g and cells[r][c] == 0:
            d[r][c] = 0
            queue.append((r, c))
    while queue:
        r, c = queue.popleft()
        for _, (dr, dc) in VAULT_MOVES:  # the reverse of a move is a move: from (r - dr, c - dc) one lands on (r, c), which is open
            pr, pc = r - dr, c - dc
            if 0 <= pr < g and 0 <= pc < g and cells[pr][pc] == 0 and d[pr][pc] < 0:
                d[pr][pc] = d[r][c] + 1
                queue.append((pr, pc))
    return d


def vault_towards(d, p):
    """the lowest-numbered of 0, 1, 2, 3, 5, 6, 7, 8 whose landing cell has the minimum finite d; none: 4"""
    g = len(d)
    best, act = None, 4
    for k, (dr, dc) in VAULT_MOVES:
        r, c = int(p[0]) + dr, int(p[1]) + dc
        if 0 <= r < g and 0 <= c < g and d[r][c] >= 0 and (best is None or d[r][c] < best):
            best, act = d[r][c], k
    return act


def goal_cells(grid, pos, has_flag, teams, flag_pos, a, role):
    """-> (the goal set Q of agent ``a`` before any tile is asked for, or None when the agent is decided before the search: it stays)"""
    g = len(grid)
    t = teams[a]
    me = (int(pos[a][0]), int(pos[a][1]))
    window = lambda f: rr.dil([(int(f[0]), int(f[1]))], g)  # noqa: E731
    if has_flag[a]:
        return window(flag_pos[t])
    if role == rr.RUNNER:
        return window(flag_pos[1 - t])
    if role == rr.CHASER:
        s = rr.opponents(pos, teams, t, g)
    else:
        assert role == rr.GUARD
        s = rr.guard_set(pos, has_flag, teams, flag_pos, t, g)
        if not s:
            return None if rr.cheb(me, flag_pos[t]) <= 1 else window(flag_pos[t])
    zone = rr.dil([(int(pos[j][0]), int(pos[j][1])) for j in s], g)  # (no opponent in the grid: no goal cell, the search finds nothing)
    return None if me in zone else zone


def ability_action(grid, pos, has_flag, teams, flag_pos, a, role, cls):
    """the deterministic action of agent ``a`` in ``role``, moving as ``cls``"""
    if cls == WALKER:
        return rr.role_action(grid, pos, has_flag, teams, flag_pos, a, role)
    q = goal_cells(grid, pos, has_flag, teams, flag_pos, a, role)
    if q is None:
        return 4
    if cls == DIGGER:
        return dig_towards(grid, dig_distances(grid, q), pos[a])
    assert cls == VAULTER
    return vault_towards(vault_distances(grid, q), pos[a])


def scripted_abilities(grid, pos, hp, has_flag, teams, types, flag_pos, vault_cost, vault_min, agent_mask, roles, ability_mask, epsilon_q32=0, seed=0,
                       step=0, env=0, out=None):
    """One env -> int8 [N]: the actions of the agents of ``agent_mask``; every other entry of ``out`` is left as it is."""
    grid = np.asarray(grid)
    n = len(teams)
    out = np.zeros(n, np.int8) if out is None else out
    for a in range(n):
        if not (agent_mask >> a) & 1:
            continue
        assert grid[int(pos[a][0]), int(pos[a][1])] != 0, "an agent's cell holds its tile"
        cls = agent_class(types[a], hp[a], (ability_mask >> a) & 1, vault_cost, vault_min)
        act = ability_action(grid, pos, has_flag, teams, flag_pos, a, roles[a], cls)
        if epsilon_q32:
            w = ref.philox4x32_10((seed & ref.M32, (seed >> 32) & ref.M32), (env & ref.M32, step & ref.M32, a, ref.TAG))
            if w[0] < epsilon_q32:
                act = (w[1] * 5) >> 32
        out[a] = act
    return out


def cfg_types(cfg):
    return [int(cfg.agent_type[i]) for i in range(cfg.n_agents)]


def state_classes(cfg, state, ability_mask):
    return [agent_class(t, state["hp"][i], (ability_mask >> i) & 1, cfg.vault_hp_cost, cfg.vault_min_hp) for i, t in enumerate(cfg_types(cfg))]


def state_abilities(cfg, state, agent_mask, roles, ability_mask, **kw):
    """The same from a ctf_config and a dict of one env's arrays (grid, pos, hp, has_flag)."""
    teams, flags = rr.cfg_teams_flags(cfg)
    return scripted_abilities(state["grid"], state["pos"], state["hp"], state["has_flag"], teams, cfg_types(cfg), flags, float(cfg.vault_hp_cost),
                              float(cfg.vault_min_hp), agent_mask, roles, ability_mask, **kw)

"""An independent restatement of the scripted COSTS (include/ctf_env.h, ctf_scripted_costs): one agent at a time, from the helpers the
action restatements already have — the goal sets of tests/_scripted_abilities_ref.py (goal_cells), the queue breadth-first search of
tests/_scripted_roles_ref.py (distances_to), the heapq Dijkstra (dig_distances) and the eight-move queue search (vault_distances) —
no bit masks and no iteration counts.  What tests/test_scripted_costs_cpu.py holds csrc/ctf_scripted.h to, and
tests/test_gpu_scripted_costs.py the kernel."""
import numpy as np

import _scripted_abilities_ref as ar
import _scripted_ref as ref
import _scripted_roles_ref as rr

COST_NONE = -1


def agent_cost(grid, pos, has_flag, teams, flag_pos, a, role, cls):
    """the cost of agent ``a`` in ``role``, moving as ``cls``, of reaching its goal set Q"""
    cells = np.asarray(grid).tolist()
    g = len(cells)
    me = (int(pos[a][0]), int(pos[a][1]))
    if not (0 <= me[0] < g and 0 <= me[1] < g):
        return COST_NONE  # outside the grid (no valid state has one)
    q = ar.goal_cells(grid, pos, has_flag, teams, flag_pos, a, role)
    if q is None:
        return 0  # decided before the search
    if me in q:
        return 0  # it stands in the (uncut) goal set
    if cls == ar.WALKER:
        d, moves, entry = rr.distances_to(grid, q), tuple(enumerate(ref.DELTAS)), lambda r, c: 1
    elif cls == ar.DIGGER:
        d, moves, entry = ar.dig_distances(grid, q), tuple(enumerate(ref.DELTAS)), lambda r, c: ar.ENTRY_COST[cells[r][c]]
    else:
        assert cls == ar.VAULTER
        d, moves, entry = ar.vault_distances(grid, q), ar.VAULT_MOVES, lambda r, c: 1
    best = None
    for _, (dr, dc) in moves:
        r, c = me[0] + dr, me[1] + dc
        if 0 <= r < g and 0 <= c < g and d[r][c] >= 0:
            cost = entry(r, c) + d[r][c]
            best = cost if best is None or cost < best else best
    return COST_NONE if best is None else best


def scripted_costs(grid, pos, hp, has_flag, teams, types, flag_pos, vault_cost, vault_min, agent_mask, roles, ability_mask, out=None):
    """One env -> int16 [N]: the costs of the agents of ``agent_mask``; every other entry of ``out`` is left as it is."""
    grid = np.asarray(grid)
    n = len(teams)
    out = np.zeros(n, np.int16) if out is None else out
    for a in range(n):
        if (agent_mask >> a) & 1:
            cls = ar.agent_class(types[a], hp[a], (ability_mask >> a) & 1, vault_cost, vault_min)
            out[a] = agent_cost(grid, pos, has_flag, teams, flag_pos, a, roles[a], cls)
    return out


def state_costs(cfg, state, agent_mask, roles, ability_mask, out=None):
    """The same from a ctf_config and a dict of one env's arrays (grid, pos, hp, has_flag)."""
    teams, flags = rr.cfg_teams_flags(cfg)
    return scripted_costs(state["grid"], state["pos"], state["hp"], state["has_flag"], teams, ar.cfg_types(cfg), flags, float(cfg.vault_hp_cost),
                          float(cfg.vault_min_hp), agent_mask, roles, ability_mask, out=out)

"""An independent restatement of the scripted ROLES (include/ctf_env.h, ctf_scripted_roles): runner, chaser and guard, one agent at a
time, with a plain queue breadth-first search, Python sets of cells and explicit Chebyshev loops — no bit masks.  The runner, the
queue search's shape and the Philox exploration rule are those of tests/_scripted_ref.py.  What tests/test_scripted_roles_cpu.py
holds csrc/ctf_scripted.h to, and tests/test_gpu_scripted_roles.py the kernel."""
from collections import deque

import numpy as np

import _scripted_ref as ref

RUNNER, CHASER, GUARD = 0, 1, 2
ROLE_NAMES = {"runner": RUNNER, "chaser": CHASER, "guard": GUARD}
GUARD_ZONE = 3


def cheb(p, q):
    return max(abs(int(p[0]) - int(q[0])), abs(int(p[1]) - int(q[1])))


def distances_to(grid, goals):
    """ref.distances with any set of goal cells: d over the OPEN cells to the open cells of ``goals``; -1 = not reachable / a wall"""
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
        for dr, dc in ref.DELTAS:
            rr, cc = r + dr, c + dc
            if 0 <= rr < g and 0 <= cc < g and cells[rr][cc] == 0 and d[rr][cc] < 0:
                d[rr][cc] = d[r][c] + 1
                queue.append((rr, cc))
    return d


def step_towards(d, p):
    """the lowest-numbered action whose neighbour of ``p`` has the minimum finite d; none: 4"""
    g = len(d)
    best, act = None, 4
    for k, (dr, dc) in enumerate(ref.DELTAS):
        r, c = int(p[0]) + dr, int(p[1]) + dc
        if 0 <= r < g and 0 <= c < g and d[r][c] >= 0 and (best is None or d[r][c] < best):
            best, act = d[r][c], k
    return act


def opponents(pos, teams, t, g):
    """opp(t): every agent of the other team that stands inside the grid"""
    return [j for j in range(len(teams)) if teams[j] != t and 0 <= int(pos[j][0]) < g and 0 <= int(pos[j][1]) < g]


def dil(cells, g):
    """the cells inside the grid within Chebyshev distance 1 of some member of ``cells``"""
    out = set()
    for p in cells:
        for r in range(int(p[0]) - 1, int(p[0]) + 2):
            for c in range(int(p[1]) - 1, int(p[1]) + 2):
                if 0 <= r < g and 0 <= c < g and cheb((r, c), p) <= 1:
                    out.add((r, c))
    return out


def guard_set(pos, has_flag, teams, flag_pos, t, g):
    """the opponents a guard of team t goes for: the carriers; if nobody carries, those within GUARD_ZONE of flag_pos[t]"""
    opp = opponents(pos, teams, t, g)
    s = [j for j in opp if has_flag[j]]
    if not s:
        s = [j for j in opp if cheb(pos[j], flag_pos[t]) <= GUARD_ZONE]
    return s


def _cached(cache, key, make):
    if cache is None:
        return make()
    if key not in cache:
        cache[key] = make()
    return cache[key]


def chase(grid, pos, a, targets, cache=None):
    """the chaser's rule on the agents ``targets`` (not empty)"""
    g = len(grid)
    zone = dil([(int(pos[j][0]), int(pos[j][1])) for j in targets], g)
    me = (int(pos[a][0]), int(pos[a][1]))
    if me in zone:
        return 4
    return step_towards(_cached(cache, frozenset(zone), lambda: distances_to(grid, zone)), me)


def role_action(grid, pos, has_flag, teams, flag_pos, a, role, cache=None):
    """the deterministic action of agent ``a`` in ``role``.  ``cache``: a dict that keeps the distance maps between the agents of
    ONE state (a map depends on the grid and the goal cells alone)."""
    g = len(grid)
    t = teams[a]
    if has_flag[a] or role == RUNNER:
        return ref.runner_action(grid, pos, has_flag, teams, flag_pos, a, cache)
    if role == CHASER:
        s = opponents(pos, teams, t, g)
        return chase(grid, pos, a, s, cache) if s else 4  # nobody to go for: no goal cell
    assert role == GUARD
    s = guard_set(pos, has_flag, teams, flag_pos, t, g)
    if s:
        return chase(grid, pos, a, s, cache)
    own = (int(flag_pos[t][0]), int(flag_pos[t][1]))
    if cheb(pos[a], own) <= 1:
        return 4
    return step_towards(_cached(cache, own, lambda: ref.distances(grid, own)), pos[a])


def scripted_roles(grid, pos, has_flag, teams, flag_pos, agent_mask, roles, epsilon_q32=0, seed=0, step=0, env=0, out=None):
    """One env -> int8 [N]: the actions of the agents of ``agent_mask``, agent i in role ``roles[i]``; every other entry of ``out``
    is left as it is.  ``env`` is the env's global index."""
    grid = np.asarray(grid)
    n = len(teams)
    out = np.zeros(n, np.int8) if out is None else out
    cache = {}
    for a in range(n):
        if not (agent_mask >> a) & 1:
            continue
        assert grid[int(pos[a][0]), int(pos[a][1])] != 0, "an agent's cell holds its tile"
        act = role_action(grid, pos, has_flag, teams, flag_pos, a, roles[a], cache)
        if epsilon_q32:
            w = ref.philox4x32_10((seed & ref.M32, (seed >> 32) & ref.M32), (env & ref.M32, step & ref.M32, a, ref.TAG))
            if w[0] < epsilon_q32:
                act = (w[1] * 5) >> 32
        out[a] = act
    return out


def cfg_teams_flags(cfg):
    n = cfg.n_agents
    return [int(cfg.agent_team[i]) for i in range(n)], [(int(cfg.flag_pos[t][0]), int(cfg.flag_pos[t][1])) for t in range(2)]


def state_roles(cfg, state, agent_mask, roles, **kw):
    """The same from a ctf_config and a dict of one env's arrays (grid, pos, has_flag)."""
    teams, flags = cfg_teams_flags(cfg)
    return scripted_roles(state["grid"], state["pos"], state["has_flag"], teams, flags, agent_mask, roles, **kw)


def role_pack(roles):
    """nibble i = roles[i]"""
    return sum(int(r) << (4 * i) for i, r in enumerate(roles))

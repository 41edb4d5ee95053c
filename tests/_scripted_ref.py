"""An independent restatement of the scripted opponent CTF_SCRIPT_RUNNER (include/ctf_env.h, ctf_scripted_actions): a plain queue
breadth-first search over a 2-D array, one agent at a time, no bit masks, plus the Philox exploration rule in Python integers.
What tests/test_scripted_cpu.py holds csrc/ctf_scripted.h to, and tests/test_gpu_scripted.py the kernel."""
from collections import deque

import numpy as np

DELTAS = ((-1, 0), (1, 0), (0, 1), (0, -1))
TAG = 0x424F5431
M32 = 0xFFFFFFFF


def philox4x32_10(key, ctr):
    """Philox4x32-10 (Salmon et al. 2011): key (k0, k1), counter (c0, c1, c2, c3) -> four words."""
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def distances(grid, target):
    """d over the OPEN (0) cells of ``grid`` to the open cells within Chebyshev distance 1 of ``target``, as a list of rows; -1 = not
    reachable / a wall."""
    cells = np.asarray(grid).tolist()
    g = len(cells)
    d = [[-1] * g for _ in range(g)]
    queue = deque()
    for r in range(target[0] - 1, target[0] + 2):
        for c in range(target[1] - 1, target[1] + 2):
            if 0 <= r < g and 0 <= c < g and cells[r][c] == 0:
                d[r][c] = 0
                queue.append((r, c))
    while queue:
        r, c = queue.popleft()
        for dr, dc in DELTAS:
            rr, cc = r + dr, c + dc
            if 0 <= rr < g and 0 <= cc < g and cells[rr][cc] == 0 and d[rr][cc] < 0:
                d[rr][cc] = d[r][c] + 1
                queue.append((rr, cc))
    return d


def runner_action(grid, pos, has_flag, teams, flag_pos, a, fields=None):
    """The deterministic action of agent ``a``.  ``fields``: a dict that keeps the distances per target between the agents of one
    state (the grid is the same for all of them)."""
    g = len(grid)
    t = teams[a]
    target = flag_pos[t] if has_flag[a] else flag_pos[1 - t]
    target = (int(target[0]), int(target[1]))
    if fields is None or target not in fields:
        d = distances(grid, target)
        if fields is not None:
            fields[target] = d
    else:
        d = fields[target]
    best, act = None, 4
    for k, (dr, dc) in enumerate(DELTAS):
        r, c = int(pos[a][0]) + dr, int(pos[a][1]) + dc
        if 0 <= r < g and 0 <= c < g and d[r][c] >= 0 and (best is None or d[r][c] < best):
            best, act = d[r][c], k
    return act


def scripted_actions(grid, pos, has_flag, teams, flag_pos, agent_mask, epsilon_q32=0, seed=0, step=0, env=0, out=None):
    """One env -> int8 [N]: the actions of the agents of ``agent_mask``; every other entry of ``out`` is left as it is.
    ``env`` is the env's global index (env_offset + e).  Agents are tiles of the grid: a state whose agent stands on an OPEN cell is
    not one the env produces."""
    grid = np.asarray(grid)
    n = len(teams)
    out = np.zeros(n, np.int8) if out is None else out
    fields = {}
    for a in range(n):
        if not (agent_mask >> a) & 1:
            continue
        assert grid[int(pos[a][0]), int(pos[a][1])] != 0, "an agent's cell holds its tile"
        act = runner_action(grid, pos, has_flag, teams, flag_pos, a, fields)
        if epsilon_q32:
            w = philox4x32_10((seed & M32, (seed >> 32) & M32), (env & M32, step & M32, a, TAG))
            if w[0] < epsilon_q32:
                act = (w[1] * 5) >> 32
        out[a] = act
    return out


def state_actions(cfg, state, agent_mask, **kw):
    """The same from a ctf_config and a dict of one env's arrays (``_cases.view_arrays``' keys grid, pos, has_flag)."""
    n = cfg.n_agents
    teams = [int(cfg.agent_team[i]) for i in range(n)]
    flags = [(int(cfg.flag_pos[t][0]), int(cfg.flag_pos[t][1])) for t in range(2)]
    return scripted_actions(state["grid"], state["pos"], state["has_flag"], teams, flags, agent_mask, **kw)

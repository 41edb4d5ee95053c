"""The cases the scripted-ROLE tests share (tests/test_scripted_roles_cpu.py on the host form, tests/test_gpu_scripted_roles.py on the
kernel): planted scenes in the form of tests/_scripted_cases.py with a role per agent, seeded random role packs, and the behavioural
run (guards against runners) on the oracle."""
import numpy as np

import oracle
import _scripted_cases as sc
import _scripted_roles_ref as rr
from _cases import abi, view_arrays

R, C, G = rr.RUNNER, rr.CHASER, rr.GUARD


def random_roles(rng, n):
    return [int(v) for v in rng.integers(0, 3, n)]


def _open(g, blocks=()):
    rows = [["."] * g for _ in range(g)]
    for r, c in blocks:
        rows[r][c] = "#"
    return ["".join(r) for r in rows]


def _diagonal():
    """7 x 7: team 0's chaser at (3, 3) stands diagonal to the opponent at (4, 4): it tags already and stays"""
    return sc.scene(_open(7), {0: (0, 0), 1: (6, 6)}, [(3, 3, 0, 1), (4, 4, 1, 0)], {0: (1, 5), 1: (5, 1)}) + ([C, C],)


def _wall():
    """9 x 9, row 2 a wall with its one gap at column 8: the chaser at (3, 4) has opponent 1 at (0, 4) three cells away by Chebyshev
    distance but behind the wall (a path through the gap: first move east), opponent 2 at (3, 0) four cells away in the open (first
    move west)"""
    rows = _open(9, [(2, c) for c in range(8)])
    return sc.scene(rows, {0: (8, 0), 1: (8, 8)}, [(3, 4, 0, 1), (0, 4, 1, 0), (3, 0, 1, 0)], {0: (6, 2), 1: (6, 6)}) + ([C, R, R],)


def _equal():
    """7 x 7: opponents at (0, 3) and (6, 3), the chaser at (3, 3) between them: north and south are equally near, north (0) wins"""
    return sc.scene(_open(7), {0: (3, 0), 1: (3, 6)}, [(3, 3, 0, 1), (0, 3, 1, 0), (6, 3, 1, 0)], {0: (1, 1), 1: (5, 5)}) + ([C, R, R],)


def _enclosed():
    """9 x 9: opponent 1 at (1, 1) has blocks on all eight sides (nothing of its neighbourhood is a goal cell), opponent 2 at (6, 6)
    is in the open: the chaser at (1, 4), nearer to the first, goes for the second"""
    rows = _open(9, [(r, c) for r in range(3) for c in range(3) if (r, c) != (1, 1)])
    return sc.scene(rows, {0: (8, 0), 1: (0, 8)}, [(1, 4, 0, 1), (1, 1, 1, 0), (6, 6, 1, 0)], {0: (4, 1), 1: (3, 7)}) + ([C, R, R],)


def _unreachable():
    """7 x 7 cut in two by row 3: no way to the only opponent, both chasers stay"""
    rows = _open(7, [(3, c) for c in range(7)])
    return sc.scene(rows, {0: (0, 0), 1: (6, 6)}, [(1, 1, 0, 1), (5, 5, 1, 1)], {0: (1, 4), 1: (5, 2)}) + ([C, C],)


def _guard(guard_at, intruder_at, carriers=(), away=(), more=()):
    """11 x 11, flag 0 at (5, 5): team 0's guard, one opponent, and whoever else"""
    agents = [guard_at + (0, 1), intruder_at + (1, 0)] + list(more)
    return sc.scene(_open(11), {0: (5, 5), 1: (0, 10)}, agents, {0: (7, 3), 1: (2, 8)}, carriers=carriers, away=away) + ([G] + [R] * (len(agents) - 1),)


def _carrying():
    """11 x 11: a chaser and a guard of team 0 that both carry a flag (and a guard of team 1 that does): they act as runners"""
    agents = [(2, 2, 0, 1), (7, 8, 1, 1), (9, 3, 0, 0), (3, 7, 1, 0)]
    return sc.scene(_open(11, [(4, 4), (4, 5), (6, 6)]), {0: (5, 5), 1: (0, 10)}, agents, {0: (7, 3), 1: (2, 8)}, carriers=(0, 1, 2), away=(0, 1)) + ([C, G, G, C],)


def edges(g):
    """g x g: team 1 stands at row 0, row g - 1, column 0 and column g - 1.  Team 0's first two agents stand at the OTHER end of the two
    edge-row opponents' columns — (0, b) under nobody, (g - 1, a) over nobody — so a dilation that ran on past row g - 1 into the next
    env's row 0, or back past row 0, would make them stay; the third guards, the fourth chases along column g - 1."""
    a, b, h = g // 4, g - 1 - g // 4, g // 2
    agents = [(0, b, 0, 0), (0, a, 1, 0), (g - 1, a, 0, 1), (g - 1, b, 1, 1), (h, h, 0, 2), (h - 1, 0, 1, 2), (h - 1, g - 1, 0, 3), (h + 1, g - 1, 1, 3)]
    kw, edits = sc.scene(_open(g, [(1, 2), (g - 2, g - 3)]), {0: (h, 1), 1: (h, g - 2)}, agents, {0: (2, 3), 1: (g - 3, g - 4)})
    return kw, edits, [C, G, C, C, G, C, C, R]


def _sixteen():
    """tests/_scripted_cases.py's 12 x 12 map with sixteen agents, ten of team 0 and six of team 1, roles mixed inside both teams;
    three agents carry (one of each role), both flags are away"""
    kw, _ = sc.planted_scenes()["sixteen12"]
    kw = dict(kw, AGENT_CONFIG={i: {"team": 0 if i % 3 else 1, "type": i % 4} for i in range(16)})
    return kw, dict(carriers=(8, 9, 11), away=(0, 1)), [(i // 3 + i) % 3 for i in range(16)]


def scenes():
    """name -> (kwargs, edits, roles)"""
    return dict(diagonal7=_diagonal(), wall9=_wall(), equal7=_equal(), enclosed9=_enclosed(), unreachable7=_unreachable(),
                guard_far11=_guard((5, 0), (10, 10)), guard_adjacent11=_guard((4, 4), (10, 10)),
                intruder3_11=_guard((5, 4), (8, 8)), intruder4_11=_guard((5, 4), (9, 9)),
                carrier_outside11=_guard((4, 4), (10, 0), carriers=(1,), away=(0,), more=[(5, 7, 1, 0)]),
                carrying11=_carrying(), edges7=edges(7), edges16=edges(16), edges32=edges(32), sixteen12=_sixteen())


def masks(cfg):
    return [sc.all_mask(cfg)] + sc.team_masks(cfg) + [1 << i for i in range(cfg.n_agents)]


# ---- the behavioural run: guards against runners ---------------------------------------------------------------------------------
BEHAVIOUR_E, BEHAVIOUR_STEPS = 64, 500
DISPOSSESSIONS, RESPAWN_TAGS = abi.METRIC_NAMES.index("flag_dispossessions"), abi.METRIC_NAMES.index("respawn_tag_count")


def behaviour_cfg():
    return sc.build(sc.workloads()["arena"])[0]


def behaviour_roles(cfg, guards):
    """team 0 runs; team 1 runs as well (run A), or puts guards on its agents of type 1, the guardians (run B)"""
    n = cfg.n_agents
    return [G if guards and int(cfg.agent_team[i]) == 1 and int(cfg.agent_type[i]) == 1 else R for i in range(n)]


def behaviour_run(guards):
    """One 500-step episode of 64 arena envs (env e seeded (e, e)) on the oracle, every agent driven by the restatement ->
    (team 0's captures, team 1's flag_dispossessions + respawn_tag_count), summed over the envs"""
    cfg = behaviour_cfg()
    n, g = cfg.n_agents, cfg.grid_size
    roles = behaviour_roles(cfg, guards)
    team1 = [i for i in range(n) if int(cfg.agent_team[i]) == 1]
    caps = tags = 0
    for e in range(BEHAVIOUR_E):
        r = oracle.OracleEnv(cfg)
        r.seed(e, e)
        for t in range(BEHAVIOUR_STEPS):
            act = rr.state_roles(cfg, view_arrays(r.get_state(), n, g), sc.all_mask(cfg), roles)
            _, done, status = r.step(act)
            assert status == 0
        assert done
        st = view_arrays(r.get_state(), n, g)
        caps += int(st["team_captures"][0])
        tags += int(st["metrics"][DISPOSSESSIONS][team1].sum() + st["metrics"][RESPAWN_TAGS][team1].sum())
    return caps, tags

"""The states the scripted-opponent tests share (tests/test_scripted_cpu.py on the host form, tests/test_gpu_scripted.py on the
kernel): the three workloads and the agent-count sweep's configs with states from oracle play, and PLANTED scenes — a config drawn as
text plus the edits (who carries a flag, which flag is away) that turn its reset state into the case."""
import numpy as np

import oracle
from _cases import abi, cfgmod, pkg, view_arrays

PLAY_STEPS = (0, 1, 17, 499)
PLAY_SEED = 0x5C21
EPSILONS = (0, 1, 1 << 31, (1 << 32) - 1)


def workloads():
    return dict(arena=dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii),
                split=dict(pkg.configs.SPLIT_KWARGS, SCENARIO=pkg.CtfScenarios.arrow),
                arena20=dict(pkg.configs.ARENA20_KWARGS, SCENARIO=pkg.configs.arena20_scenario()))


def played_states(cfg, seed, steps=PLAY_STEPS, act_seed=PLAY_SEED, env_index=0):
    """One oracle env under the synthetic action stream (reset when an episode ends) -> {step: state dict} at ``steps``; the env is
    left at its first non-zero status (no respawn cell), so a late step may be missing."""
    r = oracle.OracleEnv(cfg)
    r.seed(int(seed), int(seed))
    n, g = cfg.n_agents, cfg.grid_size
    out = {}
    for t in range(max(steps) + 1):
        if t in steps:
            out[t] = view_arrays(r.get_state(), n, g)
        if r.get_state().done:
            r.reset()
        if r.step(oracle.philox_actions(n, act_seed, t, env_index))[2]:
            break
    return out


# ---- planted scenes -------------------------------------------------------------------------------------------------------------
def scene(rows, flags, agents, spawns, carriers=(), away=()):
    """rows: text, '#' block, 'd' destructible, anything else open.  flags {team: (r, c)}, agents [(r, c, team, type)], spawns {team: (r,
    c)}.  carriers: agents with has_flag set; away: teams whose flag tile is gone from its cell (carried: the cell is a block, as the
    pickup leaves it).  -> (kwargs, state edits)"""
    g = len(rows)
    assert all(len(r) == g for r in rows)
    blocks = [(r, c) for r in range(g) for c in range(g) if rows[r][c] == "#"]
    destr = [(r, c) for r in range(g) for c in range(g) if rows[r][c] == "d"]
    scen = dict(SCENARIO_NAME="Planted", GRID_SIZE=g, FLIP_AXIS=None, FLAG_POSITIONS=dict(flags), CAPTURE_POSITIONS=dict(flags),
                SPAWN_POSITIONS=dict(spawns), AGENT_STARTING_POSITIONS={i: (a[0], a[1]) for i, a in enumerate(agents)},
                BLOCK_TILE_SLICES=blocks, DESTRUCTIBLE_TILE_SLICES=destr)
    kw = dict(GRID_SIZE=g, AGENT_CONFIG={i: {"team": a[2], "type": a[3]} for i, a in enumerate(agents)}, GAME_STEPS=50,
              MAP_SYMMETRY_CHECK=False, SCENARIO=scen)
    return kw, dict(carriers=tuple(carriers), away=tuple(away))


def planted_state(cfg, derived, edits):
    """the reset state of the config with the edits applied -> state dict (grid, pos, has_flag)"""
    n = cfg.n_agents
    grid = derived["init_grid"].copy()
    pos = np.array([[cfg.start_pos[i][0], cfg.start_pos[i][1]] for i in range(n)], np.int8)
    has_flag = np.zeros(n, np.uint8)
    for a in edits["carriers"]:
        has_flag[a] = 1
    for t in edits["away"]:
        grid[cfg.flag_pos[t][0], cfg.flag_pos[t][1]] = 1
    return dict(grid=grid, pos=pos, has_flag=has_flag)


def _serpentine():
    """32 x 32: the odd rows are corridors, joined at alternating ends (column 31, column 0, ...): from row 1 to row 31 is one path of
    some 500 cells.  Team 0's agent stands in row 1 with a dead end behind it and the other flag at the far end of row 31; team 1's
    agent waits in an alcove off row 1 (its one goal cell, (1, 1), is that dead end: it stays)."""
    rows = []
    for r in range(32):
        if r % 2:
            rows.append("." * 32)
        elif r == 0:
            rows.append("#" * 5 + "." + "#" * 26)
        else:
            rows.append("#" * 31 + "." if r % 4 == 2 else "." + "#" * 31)
    return scene(rows, {0: (1, 0), 1: (31, 0)}, [(1, 2, 0, 0), (0, 5, 1, 0)], {0: (1, 10), 1: (31, 10)})


def _walled():
    """7 x 7: flag 1 is walled in on all eight sides (team 0 has no goal cell and stays); team 1's agent already stands next to flag 0."""
    rows = (".......",
            ".......",
            ".......",
            ".......",
            "....###",
            "....#.#",
            "....###")
    return scene(rows, {0: (0, 0), 1: (5, 5)}, [(3, 3, 0, 0), (1, 1, 1, 1)], {0: (2, 2), 1: (3, 5)})


def _edges():
    """8 x 8: flag 0 in the corner (0, 0), flag 1 on column 0; both goal windows are clipped."""
    rows = ("........",
            "..#.....",
            "........",
            "...d....",
            "........",
            ".#......",
            "........",
            "........")
    return scene(rows, {0: (0, 0), 1: (5, 0)}, [(7, 7, 0, 2), (3, 6, 1, 3), (6, 2, 0, 0), (2, 4, 1, 0)], {0: (2, 6), 1: (6, 5)})


def _edges_row0():
    """7 x 7: flag 1 on row 0, flag 0 in the far corner (6, 6)."""
    rows = (".......",
            ".......",
            "..##...",
            ".......",
            "...#...",
            ".......",
            ".......")
    return scene(rows, {0: (6, 6), 1: (0, 3)}, [(5, 1, 0, 0), (1, 5, 1, 0)], {0: (4, 5), 1: (2, 5)})


def _sixteen():
    """12 x 12, sixteen agents: team 0 has two carriers and six runners (two fields in one env), team 1 one carrier; flag 1 is away
    (carried) and so is flag 0."""
    rows = ("............",
            "..#....#....",
            "..#....#..d.",
            "......##....",
            "............",
            "...##.......",
            "....#...d...",
            "............",
            ".#......##..",
            ".#..........",
            "......#.....",
            "............")
    agents = [(0, 0, 0, 0), (11, 11, 1, 0), (0, 3, 0, 1), (11, 8, 1, 1), (2, 0, 0, 2), (9, 11, 1, 2), (4, 1, 0, 3), (7, 10, 1, 3),
              (4, 4, 0, 0), (7, 7, 1, 0), (6, 2, 0, 1), (5, 9, 1, 1), (9, 5, 0, 2), (2, 6, 1, 2), (10, 9, 0, 3), (1, 9, 1, 3)]
    return scene(rows, {0: (3, 1), 1: (9, 9)}, agents, {0: (5, 1), 1: (7, 5)}, carriers=(8, 14, 13), away=(0, 1))


def _tie():
    """9 x 9 (found by a random search): all four neighbours of team 0's agent at (4, 4) are open and five steps from the goal cells
    round flag 1: the lowest action wins.  (The test asserts the tie with the queue BFS before it relies on it.)"""
    rows = ("#........",
            "..#...#.#",
            "....#..#.",
            "..#..#...",
            "#.....#.#",
            "#........",
            ".#...#.#.",
            "#......##",
            "#..##.##.")
    return scene(rows, {0: (8, 8), 1: (2, 6)}, [(4, 4, 0, 0), (6, 8, 1, 0)], {0: (5, 1), 1: (5, 2)})


def planted_scenes():
    """name -> (kwargs, edits)"""
    return dict(serpentine32=_serpentine(), walled7=_walled(), tie9=_tie(), edges8=_edges(), row0_7=_edges_row0(), sixteen12=_sixteen())


def build(kwargs, **kw):
    return cfgmod.build_config(kwargs, **kw)


def all_mask(cfg):
    return (1 << cfg.n_agents) - 1


def team_masks(cfg):
    n = cfg.n_agents
    return [sum(1 << i for i in range(n) if cfg.agent_team[i] == t) for t in (0, 1)]

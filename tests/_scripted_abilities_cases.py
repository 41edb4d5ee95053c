"""The cases the scripted-ABILITY tests share (tests/test_scripted_abilities_cpu.py on the host form, tests/test_gpu_scripted_abilities.py
on the kernel): planted scenes in the form of tests/_scripted_roles_cases.py with a role and an ability bit per agent and, where a
scene needs them, cells of DESTRUCTIBLE_TILE2 and planted hp; the edge-jump states of one two-agent config; and the closed loop (jail,
fence) on the oracle."""
import numpy as np

import oracle
import _scripted_abilities_ref as ar
import _scripted_cases as sc
import _scripted_roles_cases as rc
import _scripted_roles_ref as rr
from _cases import abi, view_arrays

R, C, G = rr.RUNNER, rr.CHASER, rr.GUARD
BLOCK, TILE1, TILE2 = 1, 2, 3  # tile codes: BLOCK_TILE, DESTRUCTIBLE_TILE1 (two hits), DESTRUCTIBLE_TILE2 (one hit)


def scene(rows, flags, agents, spawns, roles, abilities=None, hp=None, **kw):
    """sc.scene plus: 't' in ``rows`` is a cell of DESTRUCTIBLE_TILE2 in the planted state (a 'd' that took one hit), ``hp`` {agent: hp}
    replaces the reset hp, ``abilities`` lists the agents whose bit is set (None: all) -> (kwargs, edits, roles, ability mask)"""
    g = len(rows)
    tile2 = tuple((r, c) for r in range(g) for c in range(g) if rows[r][c] == "t")
    kwargs, edits = sc.scene([row.replace("t", "d") for row in rows], flags, agents, spawns, **kw)
    n = len(agents)
    mask = (1 << n) - 1 if abilities is None else sum(1 << i for i in abilities)
    return kwargs, dict(edits, tile2=tile2, hp=dict(hp or {})), list(roles), mask


def planted_state(cfg, derived, edits):
    """sc.planted_state with hp (the reset value: the type's, unless planted) and the cells of DESTRUCTIBLE_TILE2"""
    st = sc.planted_state(cfg, derived, edits)
    st["hp"] = np.array([cfg.type_hp[int(cfg.agent_type[i])] for i in range(cfg.n_agents)], np.float64)
    for a, v in edits.get("hp", {}).items():
        st["hp"][a] = v
    for r, c in edits.get("tile2", ()):
        assert st["grid"][r, c] == TILE1
        st["grid"][r, c] = TILE2
    return st


def _carved(g, cells):
    """g x g of blocks with ``cells`` {(r, c): char} carved out"""
    rows = [["#"] * g for _ in range(g)]
    for (r, c), ch in cells.items():
        rows[r][c] = ch
    return ["".join(row) for row in rows]


# the two-route scenes: 11 x 11 of blocks, team 0's miner A at (6, 1), everything else in pockets of the bottom rows
_POCKETS = {(9, 1): ".", (9, 5): ".", (9, 7): ".", (9, 9): "."}


def _routes(cells, flag1):
    rows = _carved(11, {**_POCKETS, **cells, (6, 1): "."})
    return scene(rows, {0: (9, 9), 1: flag1}, [(6, 1, 0, 3), (9, 5, 1, 0)], {0: (9, 1), 1: (9, 7)}, [R, R])


def two_goals(direct, j):
    """East of A the cells ``direct`` ('.', 'd' or 't' each) lead to the goal cell X1 next to flag 1; north of A a walk of
    len(direct) + 1 + 2 j open cells leads to the goal cell X2 above X1 (j rows up and round).  -> scene; east costs the sum of the
    direct cells' entry costs + 1, north len(direct) + 2 + 2 j"""
    n = len(direct)
    cells = {(6, 2 + k): ch for k, ch in enumerate(direct)}
    cells[(6, 2 + n)] = cells[(5, 2 + n)] = "."  # X1, X2
    for r in range(5 - j, 6):
        cells[(r, 1)] = "."
    for c in range(1, 3 + n):
        cells[(5 - j, c)] = "."
    for r in range(5 - j, 5):
        cells[(r, 2 + n)] = "."
    return _routes(cells, (6, 3 + n))


def bypass(tile):
    """East of A the cell T (``tile``), the open cell J and the goal cell X next to flag 1; north of A three open cells lead round T
    into J.  -> scene; as far as J east costs w(T), north 3"""
    cells = {(6, 2): tile, (6, 3): ".", (6, 4): ".", (5, 1): ".", (5, 2): ".", (5, 3): "."}
    return _routes(cells, (6, 5))


def _ringed(bit):
    """9 x 9: team 0's miner at (3, 3) inside a ring of eight cells of DESTRUCTIBLE_TILE1"""
    rows = [".........",
            ".........",
            "..ddd....",
            "..d.d....",
            "..ddd....",
            ".........",
            ".........",
            ".........",
            "........."]
    return scene(rows, {0: (8, 0), 1: (0, 8)}, [(3, 3, 0, 3), (7, 7, 1, 0)], {0: (6, 1), 1: (1, 6)}, [R, R], abilities=(0,) if bit else ())


def _window():
    """7 x 7: all eight cells round flag 1 are destructible: no goal cell for a walker (agent 1, a scout), eight for the miner (agent 0),
    which stands next to one of them"""
    rows = [".......",
            ".......",
            "..ddd..",
            "..d.d..",
            "..ddd..",
            ".......",
            "......."]
    return scene(rows, {0: (6, 0), 1: (3, 3)}, [(3, 1, 0, 3), (5, 3, 0, 0), (6, 6, 1, 0)], {0: (5, 1), 1: (1, 5)}, [R, R, R])


def _serpentine():
    """sc's 32 x 32 serpentine with every corridor cell a DESTRUCTIBLE_TILE1: the way from row 1 to flag 1 costs three per cell, more
    than G G = 1024 in all"""
    kw, _ = sc.planted_scenes()["serpentine32"]
    scen = kw["SCENARIO"]
    keep = {(1, 2), (0, 5), (1, 0), (31, 0)}  # the agents and the flags
    rows = [["#"] * 32 for _ in range(32)]
    for r in range(32):
        for c in range(32):
            if (r, c) not in scen["BLOCK_TILE_SLICES"]:
                rows[r][c] = "." if (r, c) in keep else "d"
    return scene(["".join(r) for r in rows], {0: (1, 0), 1: (31, 0)}, [(1, 2, 0, 3), (0, 5, 1, 0)], {0: (1, 10), 1: (31, 10)}, [R, R])


def _fence(thick, hp=None, bit=True, other=(6, 6), gap=None):
    """7 x 7: a full-width row of blocks (``thick`` of them, from row 3 up) between team 0's vaulter at (4, 3) and flag 1 at (0, 3);
    ``other`` is where team 1's scout stands, ``gap`` a cell of the fence left open"""
    rows = [["."] * 7 for _ in range(7)]
    for k in range(thick):
        rows[3 - k] = ["#"] * 7
    if gap:
        rows[gap[0]][gap[1]] = "."
    return scene(["".join(r) for r in rows], {0: (6, 0), 1: (0, 3)}, [(4, 3, 0, 2), other + (1, 0)], {0: (5, 1), 1: (1, 5)}, [R, R],
                 abilities=(0,) if bit else (), hp=hp)


def _sixteen():
    """rc's 12 x 12 scene with sixteen agents (types i % 4, ten of team 0 and six of team 1, three carriers) and every ability bit
    set; roles chosen so that each team holds the three classes and the three roles, and every class occurs in every role"""
    kw, edits, _ = rc.scenes()["sixteen12"]
    roles = [(i // 4 + i) % 3 for i in range(16)]
    return kw, dict(edits, tile2=((6, 8),), hp={}), roles, 0xFFFF


def scenes():
    """name -> (kwargs, edits, roles, ability mask)"""
    out = dict(ringed9=_ringed(True), ringed9_no_bit=_ringed(False), window7=_window(), serpentine32=_serpentine(),
               tile3_beats_3=bypass("t"), tie_3_3=bypass("d"), detour_2_beats_tile2=two_goals("d", 0),
               six_vs_5=two_goals("dd", 1), six_vs_7=two_goals("dd", 2),
               fence1=_fence(1), fence1_no_bit=_fence(1, bit=False), fence2=_fence(2), walk_jump_tie=_fence(0),
               hp_edge=_fence(1, hp={0: 3.0}), hp_above=_fence(1, hp={0: 3.25}),
               landing_taken=_fence(1, other=(2, 3)), jumped_over_agent=_fence(1, other=(3, 3), gap=(3, 3)),
               sixteen12=_sixteen())
    return out


def build_scene(name):
    """-> (cfg, state, roles, ability mask)"""
    kw, edits, roles, mask = scenes()[name]
    cfg, derived = sc.build(kw)
    return cfg, planted_state(cfg, derived, edits), roles, mask


# ---- edge jumps: one config per grid size, the state differs from case to case -------------------------------------------------------
EDGE_SIZES = (7, 16, 17, 32)


def edge_cfg(g):
    """g x g, open: team 0's vaulter (agent 0) and team 1's scout (agent 1); flag 1 in the middle, flag 0 next to it"""
    h = g // 2
    rows = ["." * g] * g
    kw, _, roles, mask = scene(rows, {0: (h, h - 1), 1: (h, h)}, [(h + 2, h, 0, 2), (h - 2, h, 1, 0)], {0: (h + 1, h + 1), 1: (h - 1, h - 1)}, [R, R])
    cfg, derived = sc.build(kw)
    return kw, cfg, derived


def _edge_state(cfg, derived, at, blocks):
    """the reset state with the vaulter moved to ``at`` and ``blocks`` laid"""
    st = planted_state(cfg, derived, dict(carriers=(), away=()))
    r0, c0 = int(st["pos"][0][0]), int(st["pos"][0][1])
    tile = st["grid"][r0, c0]
    st["grid"][r0, c0] = 0
    for r, c in blocks:
        if st["grid"][r, c] == 0:  # (a flag or the scout is a wall as it is)
            st["grid"][r, c] = BLOCK
    assert st["grid"][at] == 0, at
    st["grid"][at] = tile
    st["pos"][0] = at
    return st


def edge_cases(g):
    """-> [(what, state, the vaulter's expected action)].  The vaulter stands with a block on every unit neighbour inside the grid and
    on every landing cell but one: it takes that jump (actions 5..8), taking off from or landing on rows and columns 0, 1, g - 2 and
    g - 1.  In the 'stuck' cases every landing cell inside the grid is blocked as well: it stays, whatever the rows of another env
    hold two lanes further on."""
    kw, cfg, derived = edge_cfg(g)
    h = g // 2
    inside = lambda p: 0 <= p[0] < g and 0 <= p[1] < g  # noqa: E731
    cases = []
    col = h + 3 if g > 7 else h + 2  # a column clear of the flags and the scout (and not the reset column of the vaulter)
    starts = []
    for a in (0, 1, g - 2, g - 1):  # take-offs from the edge rows / columns ...
        for act in ((6,) if a < 2 else (5,)):
            starts.append(((a, col), act))
        for act in ((7,) if a < 2 else (8,)):
            starts.append(((col, a), act))
    for a in (2, 3, g - 4, g - 3):  # ... and landings on them
        for act in ((5,) if a < 4 else (6,)):
            starts.append(((a, col), act))
        for act in ((8,) if a < 4 else (7,)):
            starts.append(((col, a), act))
    for at, act in starts:
        land = (at[0] + ar.JUMPS[act][0], at[1] + ar.JUMPS[act][1])
        assert inside(land)
        near = [(at[0] + d[0], at[1] + d[1]) for d in ar.ref.DELTAS]
        far = [(at[0] + d[0], at[1] + d[1]) for k, d in ar.JUMPS.items() if k != act]
        blocks = [p for p in near + far if inside(p)]
        cases.append((f"from {at} by {act}", _edge_state(cfg, derived, at, blocks), act))
    for at in ((0, col), (1, col), (g - 2, col), (g - 1, col), (0, h), (g - 1, h + 1)):
        near = [(at[0] + d[0], at[1] + d[1]) for d in ar.ref.DELTAS]
        far = [(at[0] + d[0], at[1] + d[1]) for d in ar.JUMPS.values()]
        cases.append((f"stuck at {at}", _edge_state(cfg, derived, at, [p for p in near + far if inside(p)]), 4))
    return kw, cfg, cases


# ---- the closed loop: a bot of team 0 alone against a walled-in opponent that is not asked --------------------------------------------
LOOP_STEPS = 120  # GAME_STEPS of the two scenes (<= 200)
# the step of team 0's first capture with abilities, as tests/test_scripted_abilities_cpu.py measures it on the restatement and the
# oracle (and asserts it): the GPU loop runs ten steps past it
LOOP_FIRST_CAPTURE = {"jail": 11, "fence": 8}
# team_flag_captures after the whole episode of the jail scene with the bot as team 1 (what batched_duel plays), measured and asserted there too
LOOP_DUEL_CAPTURES = [0, 7]


def loop_scene(name, bot_team=0):
    """jail: the bot team's miner (agent 0) inside a ring of DESTRUCTIBLE_TILE1; fence: its vaulter behind a one-thick row of blocks.
    The other team's scout (agent 1) stands in a cell walled off by blocks, where no move of a scout changes anything, and nobody
    is ever tagged.  ``bot_team`` = 1 gives the same map with the team labels swapped (a ScriptedPolicy opponent plays team 1).
    -> (kwargs, roles)"""
    top = ["........#.#",
           "........###",
           "..........."]
    if name == "jail":
        rows = top + ["...ddd.....",
                      "...d.d.....",
                      "...ddd.....",
                      "..........."] + ["..........."] * 4
        bot = (4, 4, bot_team, 3)
    else:
        assert name == "fence"
        rows = top + ["...........",
                      "###########",
                      "...........",
                      "..........."] + ["..........."] * 4
        bot = (7, 5, bot_team, 2)
    own, other = bot_team, 1 - bot_team
    kw, _, roles, _ = scene(rows, {own: (9, 1), other: (1, 5)}, [bot, (0, 9, other, 0)], {own: (7, 4), other: (2, 8)}, [R, R])
    return dict(kw, GAME_STEPS=LOOP_STEPS), roles


BLOCKS_MINED = abi.METRIC_NAMES.index("blocks_mined")
LOOP_SEED = 7


def loop_run(name, abilities, steps=LOOP_STEPS, bot_team=0):
    """The restatement drives agent 0 on the oracle for ``steps`` steps, agent 1 plays 4 -> dict(actions [steps] of agent 0, states
    [steps + 1] (before each step and after the last), first_capture (the step whose state first shows a capture of the bot's team,
    or None))"""
    kw, roles = loop_scene(name, bot_team)
    cfg, _ = sc.build(kw)
    n, g = cfg.n_agents, cfg.grid_size
    env = oracle.OracleEnv(cfg)
    env.seed(LOOP_SEED, LOOP_SEED)
    states, actions, first = [view_arrays(env.get_state(), n, g)], [], None
    for t in range(steps):
        act = np.full(n, 4, np.int8)
        ar.state_abilities(cfg, states[-1], 1, roles, 1 if abilities else 0, out=act)
        _, done, status = env.step(act)
        assert status == 0
        actions.append(int(act[0]))
        states.append(view_arrays(env.get_state(), n, g))
        if first is None and states[-1]["team_captures"][bot_team] > 0:
            first = t
        if done:
            break
    return dict(cfg=cfg, kw=kw, roles=roles, actions=actions, states=states, first_capture=first)

"""The states the action-effect tests share (tests/test_effects_cpu.py on the host form of csrc/ctf_effects.h,
tests/test_gpu_effects.py on the kernels): the recorded fixture (tests/golden/effects/reference.npz, made by
tests/golden/make_golden_effects.py from the reference's own ``act``), and CRAFTED edge states, grouped by the config they live on so
that a group is one batch of a VecGridworldCtf."""
import os

import numpy as np

import _rule_cases as rc
import _scripted_cases as sc
from _cases import GOLDEN, cfgmod

FIXTURE = os.path.join(GOLDEN, "effects", "reference.npz")
FIELDS = ("grid", "pos", "hp", "has_flag", "inv")
PLAYED = ("arena", "split")  # tests/_scripted_cases.workloads(): arena_iii (G = 15) and arrow (G = 11)
# effect byte -> count over the planted block (190 states, 14 310 triples), as the reference's act gave them when the fixture was made.
# Where a tagged-out agent respawns depends on the generators, so the split between 0 and 1 belongs to the seeds the generator uses
# (_rule_cases.seed_of(scenario, 0), both generators, seeded behind the planting as make_golden_rules does); the other nine do not move.
PLANTED_COUNTS = {0: 10799, 1: 3018, 3: 157, 5: 85, 7: 1, 9: 3, 11: 1, 13: 201, 16: 7, 48: 2, 64: 36}


def _kwargs(block, name):
    return rc.MAPS[name] if block == "planted" else sc.workloads()[name]


_configs = {}


def config(block, name):
    """-> (env kwargs, ctf_config) of a fixture entry"""
    if (block, name) not in _configs:
        kw = _kwargs(block, name)
        _configs[(block, name)] = (kw, cfgmod.build_config(kw)[0])
    return _configs[(block, name)]


def fixture_entries():
    """[(block, name, kwargs, cfg, [state dicts], effects uint8 [S, N, 9])]"""
    z = np.load(FIXTURE)
    out = []
    for block, names in (("planted", rc.MAP_NAMES), ("played", PLAYED)):
        for name in names:
            kw, cfg = config(block, name)
            arrays = {f: z[f"{block}_{name}_{f}"] for f in FIELDS}
            states = [{f: arrays[f][k] for f in FIELDS} for k in range(len(arrays["grid"]))]
            out.append((block, name, kw, cfg, states, z[f"{block}_{name}_effects"]))
    return out


# ---- crafted edge states -------------------------------------------------------------------------------------------------------------
def _open_map(g, flags, spawns, agents, **kw):
    """an open g x g map: agents [(team, type)], parked wherever ``place`` puts them"""
    starts = []
    for r in range(g):  # any distinct open cells away from the flags: every state places its agents itself
        for c in range(g):
            if len(starts) < len(agents) and (r, c) not in flags:
                starts.append((r, c))
    scen = dict(SCENARIO_NAME=f"Effects{g}", GRID_SIZE=g, FLIP_AXIS=None, FLAG_POSITIONS=dict(enumerate(flags)), CAPTURE_POSITIONS=dict(enumerate(flags)),
                SPAWN_POSITIONS=dict(enumerate(spawns)), AGENT_STARTING_POSITIONS=dict(enumerate(starts)), BLOCK_TILE_SLICES=[],
                DESTRUCTIBLE_TILE_SLICES=[])
    return dict(GRID_SIZE=g, AGENT_CONFIG={i: {"team": t, "type": ty} for i, (t, ty) in enumerate(agents)}, GAME_STEPS=50, MAP_SYMMETRY_CHECK=False,
                SCENARIO=scen, AGENT_TYPE_HP={0: 4, 1: 4, 2: 4, 3: 4}, VAULT_HP_COST=0.5, VAULT_MIN_HP=1.0, **kw)


def place(kw, pos, hp=None, inv=None, flag=(), tiles=None):
    """One state of the map ``kw``: the agents of ``pos`` {agent: (row, col)} where it says, every other agent on the free cell
    nearest the grid's middle (so that borders and corners stay clear), full hp unless ``hp`` says otherwise; ``flag``: carriers
    (the flag's home cell then holds the block tile); ``tiles`` {(row, col): code} painted last"""
    scen, g = kw["SCENARIO"], kw["GRID_SIZE"]
    n = len(kw["AGENT_CONFIG"])
    teams = [kw["AGENT_CONFIG"][i]["team"] for i in range(n)]
    types = [kw["AGENT_CONFIG"][i]["type"] for i in range(n)]
    grid = np.zeros((g, g), np.uint8)
    for cell in scen["BLOCK_TILE_SLICES"]:
        grid[cell] = 1
    for cell in scen["DESTRUCTIBLE_TILE_SLICES"]:
        grid[cell] = 2
    for t in (0, 1):
        grid[scen["FLAG_POSITIONS"][t]] = 12 + t
    where = dict(pos)
    taken = set(where.values()) | set((tiles or {}))
    middle = sorted(((r, c) for r in range(g) for c in range(g)), key=lambda p: (max(abs(2 * p[0] - g + 1), abs(2 * p[1] - g + 1)), p))
    for i in range(n):
        if i not in where:
            where[i] = next(p for p in middle if grid[p] == 0 and p not in taken)
            taken.add(where[i])
    assert len(set(where.values())) == n
    for i in range(n):
        assert grid[where[i]] == 0, (i, where[i])
        grid[where[i]] = 4 + types[i] + 4 * teams[i]
    for i in flag:
        grid[scen["FLAG_POSITIONS"][1 - teams[i]]] = 1
    for cell, code in (tiles or {}).items():
        grid[cell] = code
    hps = [float((hp or {}).get(i, kw["AGENT_TYPE_HP"][types[i]])) for i in range(n)]
    return dict(grid=grid, pos=np.array([where[i] for i in range(n)], np.int8), hp=np.array(hps, np.float64),
                has_flag=np.array([int(i in flag) for i in range(n)], np.uint8), inv=np.array([(inv or {}).get(i, 0) for i in range(n)], np.int32))


# agent 0 a vaulter, 1 a miner (other team), 2 a scout, 3 a guardian
_FOUR = [(0, 2), (1, 3), (0, 0), (1, 1)]
SMALL = _open_map(4, [(0, 3), (3, 0)], [(1, 1), (2, 2)], _FOUR, HOME_FLAG_CAPTURE=True)
LARGE = _open_map(32, [(0, 15), (31, 16)], [(8, 8), (23, 23)], _FOUR + [(i % 2, (i // 2) % 4) for i in range(12)])  # N = 16


def _border_states(kw):
    """the vaulter, the miner (one block) and the scout in turn on every cell within two of a border (for G = 4: every cell): corners,
    borders, one and two cells from each border"""
    g = kw["GRID_SIZE"]
    flags = set(kw["SCENARIO"]["FLAG_POSITIONS"].values())
    near = [r for r in range(g) if r < 3 or r >= g - 3]
    cells = [(r, c) for r in near for c in near if (r, c) not in flags]
    if g > 8:  # the rest of each border and of the two lines inside it, thinned
        cells += [(r, c) for r in near for c in range(3, g - 3, 5) if (r, c) not in flags] + [(r, c) for c in near for r in range(3, g - 3, 5) if (r, c) not in flags]
    out = []
    for k, cell in enumerate(cells):
        other = cells[(k + len(cells) // 2 + 1) % len(cells)]
        third = cells[(k + len(cells) // 3 + 2) % len(cells)]
        if len({cell, other, third}) == 3:
            out.append(place(kw, {0: cell, 1: other, 2: third}, inv={1: 1}))
            out.append(place(kw, {1: cell, 2: other, 0: third}, inv={1: 1}, hp={0: 1.5}))  # hp 1.5: 1.5 - 0.5 > 1.0 is false, no jump
    return out


def _rule_map_states():
    """on the maps of the rule table: {map: [states]}"""
    out = {"vault": [], "miner": [], "flags": []}
    # hp at the vault threshold and one ulp above it
    for hp in (rc.HP_EQ, rc.HP_UP):
        out["vault"].append(rc.state("vault", hp={0: hp, 1: hp}))
        out["vault"].append(rc.state("vault", pos={0: (2, 2), 1: (5, 5)}, hp={0: hp, 1: hp}))
    # a target cell holding each tile code: the vaulter 0 at (4, 4) lands on (2, 4) / (4, 6) and walks into (4, 5); the scout 0 of the
    # flags map at (1, 3) walks into (0, 3) / (1, 4)
    for code in range(1, 14):
        out["vault"].append(rc.state("vault", pos={2: (1, 1)}, tiles={(2, 4): code, (4, 6): (code % 13) + 1, (4, 5): code}))
        out["flags"].append(rc.state("flags", pos={1: (6, 6)}, tiles={(0, 3): code, (1, 4): (code % 13) + 1}))
    # inventory 0, 1 and 1000 in front of a tile 3 (and of a tile 2): miner 0 at (4, 4), miner 1 at (0, 4)
    for inv in (0, 1, 1000):
        out["miner"].append(rc.state("miner", inv={0: inv}, tiles={(4, 5): 3}))
        out["miner"].append(rc.state("miner", inv={0: inv, 1: inv}, tiles={(3, 4): 3, (4, 3): 2, (1, 4): 3}))
    for code in range(1, 14):  # ... and of every code, to mine (0..3) and to lay on (5..8)
        out["miner"].append(rc.state("miner", inv={0: 2}, tiles={(3, 4): code, (5, 4): (code % 13) + 1, (4, 3): (code + 5) % 13 + 1}))
    # a block laid into each spawn window, and just outside it, from every side: the miner acts at distance 1
    starts = {0: (4, 4), 1: (0, 4)}
    for team, (x, y) in enumerate([(2, 2), (6, 6)]):
        busy = {(0, 0), (8, 8), (4, 5), (8, 0), (0, 8), starts[1 - team]}
        for dr, dc in ((-1, 0), (1, 0), (0, 1), (0, -1)):
            for dist in (2, 3):  # the target is then 1 (inside the window) / 2 (outside) from the spawn cell
                for side in (-1, 0, 1):
                    cell = (x + dist * dr + side * dc, y + dist * dc + side * dr)
                    if 0 <= cell[0] < 9 and 0 <= cell[1] < 9 and cell not in busy:
                        for inv in (0, 3):
                            out["miner"].append(rc.state("miner", pos={team: cell}, inv={team: inv}))
    # the other flag already taken; HOME_FLAG_CAPTURE with the own flag away (flags map: (2, 3), (3, 3) and (4, 3) touch both flags)
    out["flags"].append(rc.state("flags", flag=(2,)))                                   # flag 1 is carried by a teammate: no pickup for agent 0
    out["flags"].append(rc.state("flags", flag=(2, 1)))                                  # ... and flag 0 is away as well
    out["flags"].append(rc.state("flags", pos={0: (1, 2), 1: (6, 6)}, flag=(0, 1)))      # a carrier whose own flag is away: no capture
    out["flags"].append(rc.state("flags", pos={0: (1, 2), 1: (6, 6)}, flag=(0,)))        # ... and at home: capture
    out["flags"].append(rc.state("flags", flag=(1,)))                                    # flag 0 away: agent 0's pickup without the capture
    out["flags"].append(rc.state("flags", pos={2: (1, 3), 0: (0, 0)}))                   # the vaulter two from (3, 3): a jump that picks up and captures
    out["flags"].append(rc.state("flags", pos={2: (0, 3), 0: (0, 0)}, hp={2: 0.5}))
    out["flags"].append(rc.state("flags", pos={2: (0, 3), 0: (0, 0)}))
    return {k: [{f: s[f] for f in FIELDS} for s in v] for k, v in out.items()}


_groups = {}


def edge_groups():
    """name -> (env kwargs, ctf_config, [state dicts]): the crafted states, a group per config"""
    if not _groups:
        for name, kw in (("small4", SMALL), ("large32", LARGE)):
            _groups[name] = (kw, cfgmod.build_config(kw)[0], _border_states(kw))
        for name, states in _rule_map_states().items():
            kw, cfg = config("planted", name)
            _groups["rule_" + name] = (kw, cfg, states)
    return _groups


def outside_states():
    """states whose agent 0 stands outside the grid (no valid state has one: for the host form only; set_states refuses them)"""
    kw, cfg, states = edge_groups()["small4"]
    out = []
    for where in ((-1, 0), (0, -1), (4, 1), (2, 4), (-2, -2), (127, 127), (-128, 0)):
        s = {f: np.array(v) for f, v in states[0].items()}
        s["pos"][0] = where
        out.append(s)
    return cfg, out

"""What each action does in the reference, recorded (effects/reference.npz): the fixture of the action-effect rule
(include/ctf_env.h, ctf_action_effects).

Runs where the reference is importable (through _refimport.py):

    python tests/golden/make_golden_effects.py

Two blocks of states.  PLANTED: for every scenario of tests/_rule_cases.py, replica 0, the planted state (make_golden_rules.plant)
and the state after each of its steps (a step on which the reference raises ends the scenario).  Random play never reaches a pickup
or a capture within a few games; the planted table does.  PLAYED: three games of random play on each of the two workloads
(arena_iii, G = 15, and arrow, G = 11), a state every seventh step.

For every recorded state, every agent i and every action a the reference env is deep-copied, ITS OWN act(i, a) is called on the
copy, and the flag byte is derived from the difference alone:
    position changed -> MOVES, by Chebyshev distance 2 -> JUMPS; agent_flag_pickups[i] rose -> PICKS_UP; team_flag_captures rose ->
    CAPTURES; one changed cell with the position unchanged: 0 -> 2 LAYS, 2 -> 3 MINES, 3 -> 0 MINES | BREAKS
and the generator asserts that nothing else changed: no other agent's position, hp or inventory, hp only on a jump (by the cost),
the inventory only on a lay or a break, has_flag only as pickup and capture say, and for effect 0 nothing at all.

One array per (block entry, field), written by make_golden_rules.save: running the script again gives the same bytes."""
import copy
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/ (_rule_cases, _scripted_cases)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository (the package, oracle)
OUT = os.path.join(HERE, "effects", "reference.npz")
FIELDS = ("grid", "pos", "hp", "has_flag", "inv")
MOVES, JUMPS, PICKS_UP, CAPTURES, MINES, BREAKS, LAYS = 1, 2, 4, 8, 16, 32, 64
PLAYED = ("arena", "split")  # tests/_scripted_cases.workloads(): arena_iii and arrow
PLAY_GAMES, PLAY_STEPS, PLAY_EVERY = 3, 105, 7


def read_state(env):
    n = env.N_AGENTS
    return dict(grid=np.array(env.grid, np.uint8), pos=np.array([list(env.agent_positions[i]) for i in range(n)], np.int8),
                hp=np.array([float(env.agent_hp[i]) for i in range(n)], np.float64), has_flag=np.array(env.has_flag, np.uint8),
                inv=np.array([env.block_inventory[i] for i in range(n)], np.int32))


def _counters(env):
    n = env.N_AGENTS
    agent = {k: [v.get(i, 0) for i in range(n)] for k, v in env.metrics.items() if k.startswith("agent_") and isinstance(v, dict)
             and k != "agent_visitation_maps"}
    return agent, [env.metrics["team_flag_captures"][t] for t in (0, 1)]


def effect_of(env, i, a):
    """the flag byte of act(i, a), from the difference between the env and a deep copy on which the reference's act ran"""
    after = copy.deepcopy(env)
    after.act(i, a)
    b, s = read_state(env), read_state(after)
    (agent_b, caps_b), (agent_s, caps_s) = _counters(env), _counters(after)
    n = env.N_AGENTS
    others = [j for j in range(n) if j != i]
    assert np.array_equal(b["pos"][others], s["pos"][others]) and np.array_equal(b["hp"][others], s["hp"][others])
    assert np.array_equal(b["inv"][others], s["inv"][others]) and np.array_equal(b["has_flag"][others], s["has_flag"][others])
    eff = 0
    moved = not np.array_equal(b["pos"][i], s["pos"][i])
    changed = np.argwhere(b["grid"] != s["grid"])
    if moved:
        eff |= MOVES
        dist = int(np.abs(s["pos"][i].astype(int) - b["pos"][i].astype(int)).max())
        assert dist in (1, 2)
        if dist == 2:
            eff |= JUMPS
        if agent_s["agent_flag_pickups"][i] > agent_b["agent_flag_pickups"][i]:
            eff |= PICKS_UP
        if sum(caps_s) > sum(caps_b):
            eff |= CAPTURES
        carried = (int(b["has_flag"][i]) or bool(eff & PICKS_UP)) and not eff & CAPTURES
        assert int(s["has_flag"][i]) == int(carried)
        assert s["inv"][i] == b["inv"][i]
    else:
        assert agent_s["agent_flag_pickups"] == agent_b["agent_flag_pickups"] and caps_s == caps_b and s["has_flag"][i] == b["has_flag"][i]
        if len(changed) == 1:
            cell = tuple(changed[0])
            step = (int(b["grid"][cell]), int(s["grid"][cell]))
            eff |= {(0, 2): LAYS, (2, 3): MINES, (3, 0): MINES | BREAKS}[step]
            gain = {LAYS: -1, MINES: 0, MINES | BREAKS: 1 if b["inv"][i] < env.MAX_AGENT_BLOCKS else 0}[eff]
            assert s["inv"][i] == b["inv"][i] + gain
        else:
            assert len(changed) == 0 and s["inv"][i] == b["inv"][i]
    if eff & JUMPS:
        assert s["hp"][i] == b["hp"][i] - env.VAULT_HP_COST
    else:
        assert s["hp"][i] == b["hp"][i]
    if eff == 0:
        assert all(np.array_equal(b[k], s[k]) for k in FIELDS) and agent_b == agent_s and caps_b == caps_s
    return eff


def effects_of(env):
    """-> uint8 [N, 9]"""
    return np.array([[effect_of(env, i, a) for a in range(9)] for i in range(env.N_AGENTS)], np.uint8)


def _stack(rows):
    return {f: np.stack([r[f] for r in rows]) for f in FIELDS + ("effects",)}


def _row(env):
    return dict(read_state(env), effects=effects_of(env))


def record_planted(Ref, rc, mgr, map_name):
    """-> {map_field: array}: the states of the map's scenarios in the table's order; ``scenario`` (index into rc.SCENARIOS) and
    ``step`` (0 = the planted state) say which"""
    rows, which = [], []
    for k, sc in enumerate(rc.SCENARIOS):
        if sc.map != map_name:
            continue
        env = Ref(**rc.MAPS[map_name])
        mgr.plant(env, rc, sc)
        random.seed(rc.seed_of(sc, 0))
        np.random.seed(rc.seed_of(sc, 0))
        rows.append(_row(env))
        which.append((k, 0))
        for t in range(len(sc.actions)):
            if sc.auto_reset and env.done:
                env.reset()
            try:
                env.step([int(a) for a in sc.actions[t]])
            except ValueError:  # the reference's own failure: no open cell round the spawn
                break
            rows.append(_row(env))
            which.append((k, t + 1))
    out = {f"planted_{map_name}_{f}": v for f, v in _stack(rows).items()}
    out[f"planted_{map_name}_scenario"] = np.array([w[0] for w in which], np.int32)
    out[f"planted_{map_name}_step"] = np.array([w[1] for w in which], np.int32)
    return out


def record_played(Ref, kw, name):
    rows = []
    for game in range(PLAY_GAMES):
        env = Ref(**kw)
        random.seed(1000 + game)
        np.random.seed(1000 + game)
        acts = np.random.RandomState(77 + game)  # its own stream: the env's draws do not move it
        for t in range(PLAY_STEPS):
            if t % PLAY_EVERY == 0:
                rows.append(_row(env))
            if env.done:
                env.reset()
            env.step([int(a) for a in acts.randint(0, 9, env.N_AGENTS)])
    return {f"played_{name}_{f}": v for f, v in _stack(rows).items()}


def record(Ref):
    import _rule_cases as rc
    import _scripted_cases as sc
    import make_golden_rules as mgr

    rec = {}
    for map_name in rc.MAP_NAMES:
        rec.update(record_planted(Ref, rc, mgr, map_name))
    for name in PLAYED:
        rec.update(record_played(Ref, sc.workloads()[name], name))
    return rec


def main():
    import _refimport
    import make_golden_rules as mgr

    cwd = os.getcwd()
    Ref, _ = _refimport.import_reference()  # (leaves cwd in the reference: its ctor opens cwd/img/*.png)
    rec = record(Ref)
    os.chdir(cwd)
    mgr.save(OUT, rec)
    eff = np.concatenate([v.reshape(-1) for k, v in rec.items() if k.endswith("_effects")])
    states = sum(len(v) for k, v in rec.items() if k.endswith("_grid"))
    print(f"wrote {OUT}: {states} states, {len(eff)} triples, {os.path.getsize(OUT)} bytes")
    for value, count in zip(*np.unique(eff, return_counts=True)):
        print(f"  effect {int(value):3d}: {int(count)}")


if __name__ == "__main__":
    main()

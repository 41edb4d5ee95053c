"""The reference on the planted scenarios of tests/_rule_cases.py, recorded (rules/reference.npz).

Runs where the reference is importable (through _refimport.py):

    python tests/golden/make_golden_rules.py

For every scenario and each of its R replicas the reference env is constructed, the scenario's six reward constants are set on the
instance (plain attributes its constructor sets), the state is planted by assigning the instance's own attributes (grid,
agent_positions, agent_hp, has_flag, block_inventory, _arr, env_step_count, done, metrics['team_flag_captures']), both generators are
seeded, and the scenario's action rows are stepped (a scenario with ``auto_reset`` resets a done env first).  After every step the
state is recorded in full — grid, positions, f64 hp, flags, inventory, `_arr`, step count, team captures, done, the agent-level
counters — with the f64 rewards in full and, of the generators, both positions and a 64-bit digest of both whole states.  A step on
which the reference raises (no open respawn cell) is recorded as such.

One array per (map, field), the records of a map stacked in the table's order (``records_of``), in a zip whose entries carry a fixed
date: running the script again gives the same bytes."""
import io
import os
import random
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/ (_rule_cases)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository (the package, oracle)
OUT = os.path.join(HERE, "rules", "reference.npz")
FIELDS = ("grid", "pos", "hp", "has_flag", "inv", "perm", "step_count", "team_captures", "done", "metrics", "r64", "done_out", "rng", "raised")


def records_of(rc, map_name):
    """[(scenario, replica, step)] of a map in the order the arrays hold them"""
    return [(sc, r, t) for sc, r in rc.rows_of(map_name) for t in range(len(sc.actions))]


def key(map_name, field):
    return f"{map_name}_{field}"


def plant(env, rc, sc):
    s = sc.state
    n = len(s["hp"])
    for field, attr in rc.REFERENCE_ATTRS.items():
        setattr(env, attr, rc.CONSTS[sc.consts][field])
    env.grid = s["grid"].copy()
    env.agent_positions = {i: (int(s["pos"][i][0]), int(s["pos"][i][1])) for i in range(n)}
    env.agent_hp = {i: float(s["hp"][i]) for i in range(n)}
    env.has_flag = s["has_flag"].copy()
    env.block_inventory = {i: int(s["inv"][i]) for i in range(n)}
    env._arr = [int(x) for x in s["perm"]]
    env.env_step_count = int(s["step_count"])
    env.done = bool(s["done"])
    env.metrics["team_flag_captures"] = {0: int(s["team_captures"][0]), 1: int(s["team_captures"][1])}


def read(env, rc, metric_names, rewards, done):
    n = env.N_AGENTS
    st = np.random.get_state()
    return dict(grid=np.array(env.grid, np.uint8), pos=np.array([list(env.agent_positions[i]) for i in range(n)], np.int8),
                hp=np.array([float(env.agent_hp[i]) for i in range(n)], np.float64), has_flag=np.array(env.has_flag, np.uint8),
                inv=np.array([env.block_inventory[i] for i in range(n)], np.int32), perm=np.array(list(env._arr), np.uint8),
                step_count=np.int32(env.env_step_count), team_captures=np.array([env.metrics["team_flag_captures"][t] for t in (0, 1)], np.int32),
                done=np.uint8(bool(env.done)), metrics=np.array([[env.metrics["agent_" + m].get(i, 0) for i in range(n)] for m in metric_names], np.int32),
                r64=np.array([float(x) for x in rewards], np.float64), done_out=np.uint8(bool(done)),
                rng=rc.rng_summary(np.array(random.getstate()[1], np.uint32), np.concatenate([st[1].astype(np.uint32), np.array([st[2]], np.uint32)])),
                raised=np.uint8(0))


def record_map(Ref, rc, map_name, metric_names):
    kw = rc.MAPS[map_name]
    rows, blank = [], None
    for sc, r in rc.rows_of(map_name):
        env = Ref(**kw)
        plant(env, rc, sc)
        random.seed(rc.seed_of(sc, r))
        np.random.seed(rc.seed_of(sc, r))
        raised = False
        for t in range(len(sc.actions)):
            if not raised:
                if sc.auto_reset and env.done:
                    env.reset()
                try:
                    _, rewards, done = env.step([int(a) for a in sc.actions[t]])
                except ValueError:  # the reference's own failure: no open cell round the spawn
                    raised = True
            if raised:
                rows.append(None)
            else:
                rows.append(read(env, rc, metric_names, rewards, done))
                blank = blank or {k: np.zeros_like(v) for k, v in rows[-1].items()}
    rows = [row if row is not None else dict(blank, raised=np.uint8(1)) for row in rows]
    return {key(map_name, f): np.stack([row[f] for row in rows]) for f in FIELDS}


def save(path, arrays):
    """an .npz whose bytes depend on the arrays alone (np.savez stamps every entry with the time of day)"""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    import _refimport
    import _rule_cases as rc

    cwd = os.getcwd()
    Ref, _ = _refimport.import_reference()  # (leaves cwd in the reference: its ctor opens cwd/img/*.png)
    rec = {}
    for map_name in rc.MAP_NAMES:
        rec.update(record_map(Ref, rc, map_name, rc.abi.METRIC_NAMES))
    os.chdir(cwd)
    save(OUT, rec)
    print(f"wrote {OUT}: {len(rec)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

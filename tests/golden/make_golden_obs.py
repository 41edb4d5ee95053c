"""The reference's renders on the planted states of tests/_obs_cases.py, recorded (obs/reference.npz).

Runs where the reference is importable (through _refimport.py):

    python tests/golden/make_golden_obs.py

For every map and each of the four FLIP_AXIS values one reference env is constructed; every case's state is planted into it by
assigning the instance's own attributes (make_golden_rules.plant), then ``get_env_metadata(i)`` (metadata cases) or
``standardise_state(i, reverse)`` for reverse = False and True (plane cases) is called for every agent i.  A reverse mask only
chooses between an agent's two views, so these are all the views the table's four masks show; the shift-by-one of the transition
sequence consists of plane cases and needs no record of its own.

Arrays: ``<map>_meta`` uint16 [metadata case, agent, 2N + 6] (the float16 elements' bits; FLIP_AXIS does not enter: asserted while
recording) and ``<map>_planes`` uint8 [flip axis, plane case, reverse, agent, ceil(C * G * G / 8)] (np.packbits of one view).  Written
with make_golden_rules.save: running the script again gives the same bytes."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/ (_obs_cases, _rule_cases)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository (the package, oracle)
OUT = os.path.join(HERE, "obs", "reference.npz")


def key(map_name, field):
    return f"{map_name}_{field}"


def pack(views):
    """uint8 0/1 [..., C, G, G] -> the bits of every view, packed [..., ceil(C * G * G / 8)]"""
    views = np.asarray(views, np.uint8)
    return np.packbits(views.reshape(views.shape[:-3] + (-1,)), axis=-1)


def unpack(packed, c, g):
    return np.unpackbits(packed, axis=-1)[..., :c * g * g].reshape(packed.shape[:-1] + (c, g, g))


def _plant(env, rc, mgr, state):
    mgr.plant(env, rc, types.SimpleNamespace(state=state, consts="REF"))


def record_map(Ref, oc, mgr, map_name):
    n, c, g, m = oc.shape(map_name)
    meta, planes = [], []
    for flip in oc.FLIPS:
        env = Ref(**oc.kwargs(map_name, flip))
        assert env.N_AGENTS == n and len(env.TILES_USED) + 1 == c and env.GRID_SIZE == g
        rows = []
        for case in oc.meta_cases(map_name):
            _plant(env, oc.rc, mgr, case.state)
            rows.append(np.stack([np.asarray(env.get_env_metadata(i), np.float16).reshape(m).view(np.uint16) for i in range(n)]))
        meta.append(np.stack(rows))
        if map_name in oc.PLANE_MAPS:
            views = []
            for case in oc.plane_cases(map_name):
                _plant(env, oc.rc, mgr, case.state)
                views.append([[np.asarray(env.standardise_state(i, reverse_grid=rev), np.uint8).reshape(c, g, g) for i in range(n)]
                              for rev in (False, True)])
            views = np.array(views, np.uint8)
            assert views.max() <= 1
            planes.append(pack(views))
    assert all(np.array_equal(meta[0], x) for x in meta[1:]), "the metadata depends on FLIP_AXIS"
    out = {key(map_name, "meta"): meta[0]}
    if planes:
        out[key(map_name, "planes")] = np.stack(planes)
    return out


def record(Ref, oc, mgr):
    rec = {}
    for map_name in oc.MAP_NAMES:
        rec.update(record_map(Ref, oc, mgr, map_name))
    return rec


def main():
    import _refimport
    import make_golden_rules as mgr
    import _obs_cases as oc

    cwd = os.getcwd()
    Ref, _ = _refimport.import_reference()  # (leaves cwd in the reference: its ctor opens cwd/img/*.png)
    rec = record(Ref, oc, mgr)
    os.chdir(cwd)
    mgr.save(OUT, rec)
    print(f"wrote {OUT}: {len(rec)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

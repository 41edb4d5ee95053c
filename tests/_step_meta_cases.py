"""What tests/test_step_meta_cpu.py and tests/test_gpu_step_meta.py share: the metadata cases of tests/_obs_cases.py as states to be
STEPPED, for the rows that k_step writes are made from the record AFTER the step.

``predecessors(name)``: the map's ``meta_cases`` with step_count lowered by one wherever it is at least one (a step adds one to it,
done or not), so that the step fraction after the step is the case's own; captures, hp and flags are planted as the case has them:
all agents stand at their starts and STAY, where nothing is captured and nobody is tagged, and healing moves only quotients below 1.
``stepped(name)``: the oracle planted with each predecessor, seeded as its env, stepped once with all STAY and no auto-reset -> the
states after the step and the metadata bits.  Computed once per map and left unchanged.
The CPU test asserts on the oracle alone that the values after the step still reach every class of the f64 -> binary16 conversion
and every hp and flag pattern; the GPU test then only compares."""
import numpy as np

import _obs_cases as oc
import oracle
from _cases import view_arrays
from _rule_cases import STAY, to_view


def seeds(n):
    return np.arange(n, dtype=np.uint64) * np.uint64(7919) + np.uint64(23)


def predecessors(name):
    out = []
    for case in oc.meta_cases(name):
        s = dict(case.state)
        step = int(s["step_count"])
        if step >= 1:
            s["step_count"] = step - 1
            s["done"] = int(step - 1 >= oc.game_steps(name))
        out.append(s)
    return out


def stay(name, n_envs):
    return np.full((n_envs, oc.shape(name)[0]), STAY, np.int8)


_stepped = {}


def stepped(name):
    """-> (the states after the step: [view_arrays dict], metadata bits uint16 [cases, N, M])"""
    if name not in _stepped:
        cfg, pre = oc.config(name), predecessors(name)
        n, _, g, _ = oc.shape(name)
        ref, sd, acts = oracle.OracleEnv(cfg), seeds(len(pre)), stay(name, len(pre))
        after, meta = [], []
        for e, s in enumerate(pre):
            ref.seed(int(sd[e]), int(sd[e]))
            ref.set_state(to_view(s))
            _, _, status = ref.step(acts[e])
            assert status == 0, (name, e)
            after.append(view_arrays(ref.get_state(), n, g))
            meta.append(ref.observe()[1].view(np.uint16).copy())
        meta = np.stack(meta)
        meta.setflags(write=False)
        _stepped[name] = (after, meta)
    return _stepped[name]

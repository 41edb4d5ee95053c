"""What the counter_direct tests share (tests/test_counter_direct_cpu.py, tests/test_gpu_counter_direct.py): the seeds, the window caps
as the step core defines them, and the planted 8 v 8 batch whose steps draw more words than either window holds — run once on the
oracle in counter mode, which reads the tape the mode under test must read."""
import functools
import os
import re

import numpy as np

import _rule_cases as rc
import oracle
from _cases import abi, cfgmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(ROOT, "marl-ctf-development_amd", "csrc", "ctf_step_core.h")


def seeds(n_envs):
    """any 64-bit values (the ones test_counter_rng_mode_matches_the_oracle_reading_the_same_tape uses)"""
    py = np.arange(n_envs, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(77)
    return py, py ^ np.uint64(0xABCDEF0123456789)


def window_caps():
    """(NP_DIRECT_BYTES, PY_DIRECT_BYTES) of the shipped build: the most words of either tape a step finds parked"""
    text = open(CORE).read()
    return tuple(int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) for name in ("NP_DIRECT_BYTES", "PY_DIRECT_BYTES"))


def counter_config(kwargs, log_metrics=True):
    return cfgmod.build_config(kwargs, log_metrics=log_metrics, rng_mode=abi.RNG_COUNTER)[0]


# ---- beyond the window: 16 agents, agent 0 inside a ring of its eight opponents, four of them one hit from a respawn -------------------
BEYOND_ENVS, BEYOND_STEPS = 24, 12  # (GAME_STEPS of the map is 20: no env ends)
BEYOND_KWARGS = rc.MAPS["tag16"]


def beyond_state():
    return rc._kill(8, 0)[1]


def beyond_actions(t, e):
    return oracle.philox_actions(16, 0xBE70, t, e)


@functools.lru_cache(maxsize=None)
def beyond_oracle():
    """-> per env the list of per-step (rewards f64, done, status, state view arrays, (py words, np words) consumed so far)"""
    cfg = counter_config(BEYOND_KWARGS)
    py, npz = seeds(BEYOND_ENVS)
    view = rc.to_view(beyond_state())
    out = []
    for e in range(BEYOND_ENVS):
        env = oracle.OracleEnv(cfg)
        env.seed(int(py[e]), int(npz[e]))
        env.set_state(view)
        rows = []
        for t in range(BEYOND_STEPS):
            rw, done, status = env.step(beyond_actions(t, e))
            rows.append((rw, done, status, rc.view_arrays(env.get_state(), env.n, env.g), env.get_rng_counters()))
        out.append(rows)
    return out


def beyond_fractions(runs):
    """the share of env-steps whose draw from the (`random`, np.random) tape exceeds the window's cap — whatever the offset of the
    first word in its block, such a step draws past what was parked"""
    np_cap, py_cap = window_caps()
    py_d, np_d = [], []
    for rows in runs:
        prev = (0, 0)
        for row in rows:
            py_d.append(row[4][0] - prev[0])
            np_d.append(row[4][1] - prev[1])
            prev = row[4]
    return float((np.array(py_d) > py_cap).mean()), float((np.array(np_d) > np_cap).mean())

"""The cases the scattered-reset tests share (tests/test_scatter_cpu.py on the host form of csrc/ctf_scatter.h, tests/test_gpu_scatter.py
on the kernel): the configs — the arena (G = 15, N = 8), the split map (G = 11, N = 4), sixteen agents on G = 32 and the 4 x 4 map of
tests/_effects_cases.py, every agent count 2..16 of tests/_agent_counts.py — and, per config, the argument combinations: radius 0, 1, 2
and G, with and without OWN_SIDE, all agents, each team, the first and the last agent alone, with round and episode offsets up to the
u32 wrap."""
import _agent_counts as ac
import _effects_cases as ec
import _scripted_cases as sc
from _cases import cfgmod

BATCHES = (1, 3, 67)
ENV_OFFSET = 0xFFFFFFF0  # + env index wraps inside the 67-env batch
# arena candidate counts of the eight agents with nothing taken (counted on the CPU, include/ctf_env.h has the rule)
ARENA_COUNTS = {1: [5, 5, 6, 6, 7, 7, 4, 4], 2: [18, 18, 12, 12, 13, 13, 11, 11]}
ARENA_WHOLE, ARENA_WHOLE_OWN_SIDE = 179, 97

_configs = {}


def configs():
    """name -> (env kwargs, ctf_config)"""
    if not _configs:
        named = dict(arena=sc.workloads()["arena"], split=sc.workloads()["split"], large32=ec.LARGE, small4=ec.SMALL)
        for c in ac.CONFIGS:
            named["count-" + ac.config_id(c)] = ac.config_kwargs(*c)
        for name, kw in named.items():
            _configs[name] = (kw, cfgmod.build_config(kw)[0])
    return _configs


def config_names():
    return ["arena", "split", "large32", "small4"] + ["count-" + ac.config_id(c) for c in ac.CONFIGS]


def agent_masks(cfg):
    n = cfg.n_agents
    return [sc.all_mask(cfg)] + sc.team_masks(cfg) + [1, 1 << (n - 1)]


def combos(cfg):
    """[(radius, own_side, agent_mask, seed, round, episode)]: every radius x flag x mask; the draws' offsets change from one to the
    next and reach the u32 wrap of round + episode"""
    offsets = [(0, 0), (5, 0), (0, 9), (0xFFFFFFFF, 1), (0xFFFFFFF0, 0x20), (0x80000000, 0x80000000), (3, 0xFFFFFFFF)]
    out = []
    for radius in (0, 1, 2, cfg.grid_size):
        for own_side in (False, True):
            for mask in agent_masks(cfg):
                k = len(out)
                rnd, ep = offsets[k % len(offsets)]
                out.append((radius, own_side, mask, 0x9E3779B97F4A7C15 * (k + 1) & 0xFFFFFFFFFFFFFFFF, rnd, ep))
    return out

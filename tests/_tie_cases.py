"""The tie cases of rng_mode="counter_direct" (tests/test_counter_direct_cpu.py asserts their conditions on the oracle alone,
tests/test_gpu_direct_edges.py runs them on the device, tests/hostsim/direct_main.cpp repeats the sweep under sanitizers).

``np.random.rand() < TAG_PROBABILITY`` compares the draw's 53-bit integer (w0 >> 5) << 26 | w1 >> 6 with ceil(p * 2**53).  A word of a
Philox tape cannot be chosen, the threshold can: for the draw that starts at tape word n*, X is that integer and the three VARIANTS
put the threshold at X (the draw misses on equality), at X + 1 (it hits through hi == th and lo < tl) and at the next multiple of
2**26 (it hits through hi < th, tl = 0).  All three are exact doubles.

The configuration: 16 agents of type 0 on the 4 x 4 block of cells (1..4, 1..4) of an open 7 x 7 map, team = (row + col) % 2, hp 20,
damage 1: a step draws 16 * 8 pairs = 256 np.random words and nobody is put out.  Env k of a handle starts its np.random tape at word
n* - 2 k, so that the step's k-th rand() is the draw at n*; byte b = ((n* - 2 k) & 3) + 2 k of the step's window holds its first word
(b = n* mod 4).  A draw is DECIDING where the oracle's hp after the step differs between the tie and the tie+1 variant: only those
k are worth an env."""
import functools

import numpy as np

import _philox
import _rule_cases as rc
import oracle
from _cases import abi, cfgmod

PY_SEED = 77
NP_SEED = 77 ^ 0xABCDEF0123456789
PY_COUNTER = 3
# a second position of the `random` tape, for the host program alone: the shuffle it gives puts tagging pairs first, so that the
# step's draws 0, 2 and 3 decide.  With PY_COUNTER the first deciding draw is k = 5 (b >= 10): past a window shrunk to 8 bytes.
EARLY_PY_COUNTER = 20
N_STAR = 2000            # + r, r in RESIDUES: the tape word the deciding draw starts at (2000 % 4 == 0: r is its word in the block)
RESIDUES = (0, 1, 2, 3)  # r = 3: the draw's two words lie in different blocks
VARIANTS = ("tie", "tie+1", "next-hi")
N_AGENTS, PAIRS = 16, 128
FOLLOW_SEED = 0x71E5     # the action stream of the steps after the first
STAY = np.full(N_AGENTS, 4, np.int8)
CTR_TAG = 0x43544631     # ctf_mt.h CTF_CTR_TAG


def kwargs(tag_probability):
    cells = [(r, c) for r in range(1, 5) for c in range(1, 5)]
    return rc._map("Tie16", rc.OPEN7, flags=[(0, 6), (6, 0)], spawns=[(0, 0), (6, 6)], teams=[(r + c) % 2 for r, c in cells], types=[0] * 16,
                   starts=cells, GAME_STEPS=20, TAG_PROBABILITY=tag_probability, AGENT_TYPE_HP={t: 20 for t in range(4)},
                   AGENT_TYPE_DAMAGE={t: 1 for t in range(4)})


def config(tag_probability):
    return cfgmod.build_config(kwargs(tag_probability), log_metrics=True, rng_mode=abi.RNG_COUNTER)[0]


def tape_word(seed, n, stream=1):
    """word n of a counter tape (ctf_mt.h ctr_block): stream 1 is np.random's, 0 is `random`'s"""
    blk = n >> 2
    out = _philox.philox4x32_10((blk & 0xFFFFFFFF, blk >> 32, stream, CTR_TAG), (seed & 0xFFFFFFFF, seed >> 32))
    return int(out[n & 3])


def draw_integer(n):
    """X of the rand() that starts at word n of the np.random tape"""
    return (tape_word(NP_SEED, n) >> 5) << 26 | tape_word(NP_SEED, n + 1) >> 6


def probability(r, variant):
    x = draw_integer(N_STAR + r)
    thr = {"tie": x, "tie+1": x + 1, "next-hi": ((x >> 26) + 1) << 26}[variant]
    p = thr / 2.0 ** 53
    assert 0.0 <= p <= 1.0 and int(p * 2.0 ** 53) == thr  # exact
    return p


def np_counter(r, k):
    return N_STAR + r - 2 * k


def window_byte(r, k):
    """b: the byte of the step's np.random window that holds the first word of env k's draw at n*"""
    return (np_counter(r, k) & 3) + 2 * k


def position_class(b, fill):
    """where the draw's two bytes lie: both parked / the first parked and the second not / neither"""
    return "inside" if b + 1 < fill else "edge" if b == fill - 1 else "beyond"


def parking_lane(b, lanes):
    """the lane of the env's group that parks byte b: block t of the list is lane t % W's, and the np.random blocks come first"""
    return (b >> 2) % lanes


def twin(cfg, r, k, py_counter=PY_COUNTER):
    env = oracle.OracleEnv(cfg)
    env.seed(PY_SEED, NP_SEED)
    env.set_rng_counters(py_counter, np_counter(r, k))
    return env


def actions(t, e):
    return STAY if t == 0 else oracle.philox_actions(N_AGENTS, FOLLOW_SEED, t, e)


def twin_step(env, acts):
    """one step of an oracle twin -> its outputs in rc.compare's form"""
    rw, done, status = env.step(acts)
    out = rc.snapshot(env, counter=True)
    out.update(r64=rw, r32=rw.astype(np.float32), done_out=int(done), status=int(status))
    return out


@functools.lru_cache(maxsize=None)
def first_step(r, py_counter=PY_COUNTER):
    """-> {variant: [per k (hp after the step, words consumed, status, tag_count sum)]} of the oracle alone, every k"""
    out = {}
    for v in VARIANTS:
        cfg = config(probability(r, v))
        rows = []
        for k in range(PAIRS):
            env = twin(cfg, r, k, py_counter)
            o = twin_step(env, STAY)
            rows.append((o["hp"].copy(), tuple(int(x) for x in o["rng"]), o["status"], int(o["metrics"][rc.M["tag_count"]].sum())))
        out[v] = rows
    return out


@functools.lru_cache(maxsize=None)
def deciding(r, py_counter=PY_COUNTER):
    """the k whose draw at n* decides an agent's hp: the oracle's hp differs between the tie and the tie+1 variant"""
    rows = first_step(r, py_counter)
    return tuple(k for k in range(PAIRS) if not np.array_equal(rows["tie"][k][0], rows["tie+1"][k][0]))

"""The table of the observation suite (tests/test_obs_cases_cpu.py, tests/test_gpu_obs_cases.py, tests/golden/make_golden_obs.py): the
renders' whole input space reached from PLANTED states instead of by random play, which shows them a capture ratio in [1/9, 9], hp
elements 0..2 and the few tile changes a move, a tag or a respawn makes.

Maps (layout, agents and ``state()`` are those of tests/_rule_cases.py; a flip axis is a copy of the kwargs with FLIP_AXIS replaced):
  term16   16 agents, 8 x 8, both teams own all four types: all 14 tile codes are in the reference's domain.  11 264-byte blocks
  tag16    16 scouts, 9 x 9
  tag      6 agents, 9 x 9: 4 860-byte blocks, no multiple of 16
  flags    4 agents, 7 x 7, the smallest
  wide16   term16 with GAME_STEPS = 2**26 and four different AGENT_TYPE_HP: step fractions below 2**-14 (the halves' subnormals can
           be reached through element 0 with no smaller divisor) and an hp element that shows which type's hp it was divided by

METADATA CASES (``meta_cases``): a state at the map's start grid with step_count, team_captures, hp and has_flag planted.
  ratio-*   team_captures (a, b): element 1 is (a + 1) / (b + 1) for team 0's viewers and its inverse for team 1's, one case at least
            for every class of the f64 -> binary16 conversion (``half_of`` names the classes by the exact rational value)
  step-*    the same classes through element 0 = step_count / GAME_STEPS; a step_count of GAME_STEPS or more comes with done = 1
  hp-r      agents 0..3 carry pairwise distinct quotients of HP_QUOTIENTS times their own type's AGENT_TYPE_HP, rotated over four
            cases: every hp element then shows which agent it was read from (and on wide16 which type's hp divided it)
  flag-k    has_flag[i] = bit k of i, and a last case of all ones: every flag element then shows which agent it was read from
Domain, as the reference accepts it (asserted by tests/test_obs_cases_cpu.py): team_captures in [0, 2**31 - 2] (the device adds 1 in
int32; -1 divides by zero), 0 <= step_count < 2**28 (set_state's rule), agent types < N wherever metadata is read (the reference
indexes agent_hp by the type id).  Every hp quotient the metadata shows lies in [0, 256): the reference casts it to uint8 with NumPy,
which is undefined in C and platform-dependent outside that range, so negative quotients and quotients >= 256 are left out.

PLANE CASES (``plane_cases``): grid k of a map holds code CODES[(stride * c + k) mod K] in cell c, k = 0..K-1, so every code stands in
every cell once (term16: K = 14, stride 5: code (5c + k) mod 14; the stride is 3 where 5 divides K).  CODES are open, block, both
destructibles, both flags and the tiles of the map's own agents: the reference relabels a grid by the tiles of the agents that exist,
so the tile of a (team, type) no agent has is outside its domain and is left out.  A code without a channel of its own (1, 2, 3 on
these maps) shows in no plane.  Viewers' positions do not follow the grid: drawn uniformly (two viewers on a cell, a viewer on a
cell that holds another tile), plus cases with all N on one cell and with the viewers in the four corners.  The agents of a plane
case carry 25 times their full hp, so that a step from it tags nobody out.  Every case runs under
FLIP_AXIS None, 0, 1, 2 and the reverse masks none, all, the default and the per-team alternating one (``masks``).

TRANSITION SEQUENCE (``transition_states``): K envs, env e holding grid e, then shifted by s = 1, 2 .. K-1 grids from one render to the
next: each shift puts every ordered pair (old code, old code + s) into some cell, all of them together every ordered pair of different
codes.  Positions are redrawn for every render; those of renders 0 and 1 are the plane cases', so the recorded reference covers the
shift by one.  One further env keeps grid 0 and its positions throughout.

``compare`` is the one comparison the CPU test's wrong-input checks and the GPU test share: bytes of the planes, bits of the metadata."""
import math
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np

import _rule_cases as rc
from _cases import abi, cfgmod

FLIPS = (None, 0, 1, 2)
MAX_ENVS = 128  # per handle
WIDE_STEPS = 1 << 26
MAPS = {  # name -> (the map of _rule_cases it is, kwargs replaced)
    "term16": ("term16", {}), "tag16": ("tag16", {}), "tag": ("tag", {}), "flags": ("flags", {}),
    "wide16": ("term16", dict(GAME_STEPS=WIDE_STEPS, AGENT_TYPE_HP={0: 2, 1: 3, 2: 5, 3: 7})),
}
MAP_NAMES = tuple(MAPS)
HP_QUOTIENTS = (0, 0.999, 1, 2.5, 37.2, 200, 255, 255.99)
CAPS_MAX, STEP_LIMIT = 2 ** 31 - 2, 1 << 28


# ---- maps and configs ------------------------------------------------------------------------------------------------------------------
def kwargs(name, flip="own"):
    base, over = MAPS[name]
    kw = dict(rc.MAPS[base], **over)
    if flip != "own":
        kw["SCENARIO"] = dict(kw["SCENARIO"], FLIP_AXIS=flip)
    return kw


_configs = {}


def config(name, flip="own", log_metrics=True):
    key = (name, flip, log_metrics)
    if key not in _configs:
        _configs[key] = cfgmod.build_config(kwargs(name, flip), log_metrics=log_metrics)[0]
    return _configs[key]


def teams(name):
    ac = kwargs(name)["AGENT_CONFIG"]
    return [ac[i]["team"] for i in range(len(ac))]


def types(name):
    ac = kwargs(name)["AGENT_CONFIG"]
    return [ac[i]["type"] for i in range(len(ac))]


def type_hp(name):
    return kwargs(name)["AGENT_TYPE_HP"]


def game_steps(name):
    return kwargs(name)["GAME_STEPS"]


def shape(name):
    """-> (N, C, G, M)"""
    cfg = config(name)
    return cfg.n_agents, cfg.n_channels, cfg.grid_size, 2 * cfg.n_agents + 6


def masks(name):
    """[none, all, the default (None: team 1 reversed), every other agent of each team]"""
    seen, alt = [0, 0], 0
    for i, t in enumerate(teams(name)):
        alt |= (seen[t] & 1) << i
        seen[t] += 1
    return [0, (1 << len(teams(name))) - 1, None, alt]


def reversed_views(name, mask):
    """-> [is agent i's view reversed under ``mask``]"""
    return [bool(t == 1 if mask is None else (mask >> i) & 1) for i, t in enumerate(teams(name))]


# ---- the conversion's classes, by the exact value --------------------------------------------------------------------------------------
CLASSES = ("zero", "exact normal", "normal rounded down", "normal rounded up", "normal tie, even mantissa", "normal tie, odd mantissa",
           "carry into the exponent", "largest finite", "overflow by rounding", "overflow", "subnormal", "subnormal tie, even", "subnormal tie, odd",
           "subnormal carrying into the smallest normal", "underflow")


def half_of(q):
    """The binary16 nearest to the rational q >= 0, ties to even -> (its bits, the class of the rounding).  Integer and Fraction
    arithmetic only."""
    q = Fraction(q)
    assert q >= 0
    if q == 0:
        return 0, "zero"
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    scaled = q / Fraction(2) ** (max(e, -14) - 10)  # in units of the last place
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    odd, tie, up = n & 1, rem == Fraction(1, 2), rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1)
    n += int(up)
    if e < -14:  # below the smallest normal: n units of 2**-24
        assert 0 <= n <= 1024
        cls = ("subnormal carrying into the smallest normal" if n == 1024 else f"subnormal tie, {'odd' if odd else 'even'}" if tie else
               "underflow" if n == 0 else "subnormal")
        return n, cls
    assert 1024 <= n <= 2048
    if e > 15:
        return 0x7C00, "overflow"
    bits = ((e + 15) << 10) + (n - 1024)  # (n == 2048 carries into the exponent field by itself)
    if bits == 0x7C00:
        return bits, "overflow by rounding"
    if bits == 0x7BFF:
        return bits, "largest finite"
    if n == 2048:
        return bits, "carry into the exponent"
    if tie:
        return bits, f"normal tie, {'odd' if odd else 'even'} mantissa"
    return bits, "exact normal" if rem == 0 else "normal rounded up" if up else "normal rounded down"


# ---- metadata cases ----------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name map state")

RATIOS = [(2, 1), (0, 2), (2, 4), (8, 0), (12, 6), (2048, 0), (2050, 0), (4094, 1), (65518, 0), (65503, 0), (65519, 0), (CAPS_MAX, 0), (CAPS_MAX, CAPS_MAX),
          (0, 19999), (0, 2 ** 25 - 1), (2, 2 ** 25 - 1), (4094, 2 ** 26 - 1), (0, 2 ** 26 - 1), (2, 2 ** 26 - 1), (6, 2 ** 26 - 1), (CAPS_MAX, 2 ** 16)]


def step_counts(name):
    gs = game_steps(name)
    if gs == WIDE_STEPS:  # multiples of 2**-26: 2**-24 is the last place of a subnormal half
        steps = [0, 1, 2, 3, 6, 7, 4095, 4096, 5 << 12, gs - 1, gs, gs + 1, STEP_LIMIT - 1]
    else:
        steps = [0, 1, gs - 1, gs, gs + 1, 65520 * gs, STEP_LIMIT - 1, gs // 2, 2049 * gs, 2051 * gs, 2047 * gs + gs // 2, 65504 * gs, 65519 * gs,
                 3 * gs + 7]
    assert all(0 <= s < STEP_LIMIT for s in steps) and len(set(steps)) == len(steps)
    return steps


def _meta_state(name, step=0, caps=(0, 0), hp=None, flags=None):
    s = rc.state(MAPS[name][0], step=step, caps=caps, done=int(step >= game_steps(name)))
    t, full = types(name), type_hp(name)
    s["hp"] = np.array([float((hp or {}).get(i, full[t[i]])) for i in range(len(t))], np.float64)
    if flags is not None:
        s["has_flag"] = np.array(flags, np.uint8)
    return s


def hp_planted(name, r):
    """{agent: hp} of rotation r: agent i of 0..3 carries quotient (i + 2r) mod 8 of its own type's full hp"""
    t, full = types(name), type_hp(name)
    return {i: HP_QUOTIENTS[(i + 2 * r) % 8] * full[t[i]] for i in range(4)}


def flag_case_count(name):
    return math.ceil(math.log2(len(teams(name)))) + 1


def flags_planted(name, k):
    n = len(teams(name))
    return [1] * n if k == flag_case_count(name) - 1 else [(i >> k) & 1 for i in range(n)]


_meta = {}


def meta_cases(name):
    if name not in _meta:
        out = [Case(f"ratio-{a}-{b}", name, _meta_state(name, step=k % game_steps(name), caps=(a, b))) for k, (a, b) in enumerate(RATIOS)]
        out += [Case(f"step-{s}", name, _meta_state(name, step=s, caps=(k % 3, k % 2))) for k, s in enumerate(step_counts(name))]
        out += [Case(f"hp-{r}", name, _meta_state(name, step=r, hp=hp_planted(name, r))) for r in range(4)]
        out += [Case(f"flag-{k}", name, _meta_state(name, step=k, caps=(1, 1), flags=flags_planted(name, k))) for k in range(flag_case_count(name))]
        assert len(out) <= MAX_ENVS
        _meta[name] = out
    return _meta[name]


def meta_case(name, case_name):
    return next(c for c in meta_cases(name) if c.name == case_name)


# ---- plane cases -------------------------------------------------------------------------------------------------------------------------
def codes(name):
    """the tile codes of the reference's domain on this map, ascending"""
    return sorted({0, 1, 2, 3, 12, 13} | {4 + ty + 4 * te for te, ty in zip(teams(name), types(name))})


def grid(name, k):
    cs, g = codes(name), shape(name)[2]
    stride = 5 if math.gcd(5, len(cs)) == 1 else 3
    assert math.gcd(stride, len(cs)) == 1
    return np.array([cs[(stride * c + k) % len(cs)] for c in range(g * g)], np.uint8).reshape(g, g)


def positions(name, kind, *key):
    """int8 [N, 2]: "random" (uniform over the grid), "cell" (all N on one drawn cell) or "corners" (agent i in corner i mod 4)"""
    n, _, g, _ = shape(name)
    rng = np.random.default_rng([zlib.crc32(name.encode()), zlib.crc32(kind.encode())] + [int(x) for x in key])
    if kind == "random":
        return rng.integers(0, g, (n, 2)).astype(np.int8)
    if kind == "cell":
        return np.repeat(rng.integers(0, g, (1, 2)), n, axis=0).astype(np.int8)
    corners = [(0, 0), (0, g - 1), (g - 1, 0), (g - 1, g - 1)]
    return np.array([corners[i % 4] for i in range(n)], np.int8)


def _plane_state(name, k, pos):
    s = rc.state(MAPS[name][0])
    s["grid"], s["pos"] = grid(name, k), pos
    s["hp"] = 25 * s["hp"]  # nobody is tagged out when a plane case is stepped: these grids may hold no open respawn cell
    return s


_planes = {}


def plane_cases(name):
    if name not in _planes:
        K = len(codes(name))
        out = [Case(f"grid{k}-random", name, _plane_state(name, k, positions(name, "random", k))) for k in range(K)]
        out += [Case(f"grid{k}-cell", name, _plane_state(name, k, positions(name, "cell", k))) for k in (1, K // 2)]
        out += [Case("grid2-corners", name, _plane_state(name, 2, positions(name, "corners")))]
        _planes[name] = out
    return _planes[name]


PLANE_MAPS = ("term16", "tag16", "tag", "flags")  # (wide16's planes are term16's)


def transition_renders(name):
    return len(codes(name))  # render 0 and one per shift s = 1 .. K-1


def transition_grids(name, r):
    """the grid index env e = 0..K-1 holds at render r: e + 1 + 2 + .. + r"""
    K = len(codes(name))
    return [(e + r * (r + 1) // 2) % K for e in range(K)]


def transition_states(name, r):
    """the K + 1 states of render r: env e holds its grid of that render, env K keeps grid 0 and its positions"""
    ks = transition_grids(name, r)
    pos = lambda k: positions(name, "random", k) if r < 2 else positions(name, "random", k, r)
    return [_plane_state(name, k, pos(k)) for k in ks] + [_plane_state(name, 0, positions(name, "random", 0))]


# ---- states as set_states takes them, the oracle on a state, the comparison ----------------------------------------------------------------
SET_FIELDS = dict(grid=("grid", np.uint8), pos=("pos", np.int8), hp=("hp", np.float64), has_flag=("has_flag", np.uint8), inventory=("inv", np.int32),
                  perm=("perm", np.uint8), step_count=("step_count", np.int32), team_captures=("team_captures", np.int32), done=("done", np.uint8))


def stacked(states):
    """[state] -> {set_states field: numpy array [n, ...]}"""
    return {f: np.stack([np.asarray(s[k]) for s in states]).astype(dt) for f, (k, dt) in SET_FIELDS.items()}


def oracle_observe(cfg, states, mask, env=None):
    """-> (planes uint8 [n, N, C, G, G], metadata bits uint16 [n, N, M]) of the oracle planted with each state in turn"""
    import oracle

    env = env or oracle.OracleEnv(cfg)
    obs, meta = [], []
    for s in states:
        env.set_state(rc.to_view(s))
        o, m = env.observe(abi.REVERSE_DEFAULT if mask is None else int(mask))
        obs.append(o)
        meta.append(m.view(np.uint16))
    return np.stack(obs), np.stack(meta)


def compare(got_obs, got_meta, want_obs, want_meta):
    """What the thing under test wrote against what is expected, exactly: the planes' bytes (uint8 [..., N, C, G, G]) and the metadata's
    bits (uint16 or float16 [..., N, M]); either pair may be None -> the list of what differs (empty: equal), the first index of each."""
    bad = []
    for what, got, want in (("planes", got_obs, want_obs), ("metadata", got_meta, want_meta)):
        if got is None and want is None:
            continue
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        if what == "metadata":
            got, want = got.view(np.uint16), want.view(np.uint16)
        if got.shape != want.shape or got.dtype != want.dtype:
            bad.append(f"{what}: shape {got.shape} {got.dtype}, expected {want.shape} {want.dtype}")
        elif not np.array_equal(got, want):
            at = tuple(int(x) for x in np.argwhere(got != want)[0])
            bad.append(f"{what}: {int((got != want).sum())} elements differ, the first at {at}: {int(got[at]):#x} != {int(want[at]):#x}")
    return bad

"""The observation suite without a GPU (tests/_obs_cases.py is the table): the oracle, planted with ``set_state``, renders what the
reference rendered from the same planted state (tests/golden/obs/reference.npz, recorded by tests/golden/make_golden_obs.py) on every
case, under every flip axis and mask; the table stays inside the domain its docstring states; a classifier in exact rational arithmetic
finds every class of the f64 -> binary16 conversion through element 0 and through element 1 and gives the recorded bits; the recorded
hp and flag elements each show which agent they were read from; the transition sequence holds every ordered pair of codes; and the
shared compare function reports each of four deliberately wrong inputs.

tests/test_gpu_obs_cases.py relies on this: it compares the kernels with the oracle and does not measure its own inputs."""
import math
import os
import sys
from fractions import Fraction as F

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import _refimport  # noqa: E402
import make_golden_obs as mgo  # noqa: E402
import make_golden_rules as mgr  # noqa: E402

import _obs_cases as oc  # noqa: E402
from _cases import abi  # noqa: E402

ONE = 0x3C00  # 1.0 as a half


def _load():
    with np.load(mgo.OUT) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def record():
    rec = _load()
    assert sorted(rec) == sorted([mgo.key(m, "meta") for m in oc.MAP_NAMES] + [mgo.key(m, "planes") for m in oc.PLANE_MAPS])
    return rec


def recorded_planes(rec, name, flip, mask):
    """-> uint8 [plane case, N, C, G, G]: every agent's view under ``mask`` as the reference rendered it"""
    n, c, g, _ = oc.shape(name)
    views = mgo.unpack(rec[mgo.key(name, "planes")][oc.FLIPS.index(flip)], c, g)
    rev = oc.reversed_views(name, mask)
    return np.stack([views[:, int(rev[i]), i] for i in range(n)], axis=1)


def _states(cases):
    return [c.state for c in cases]


def _oracle_against(rec, name):
    """-> rows compared; raises on the first case that differs"""
    rows = 0
    meta_want = rec[mgo.key(name, "meta")]
    assert len(meta_want) == len(oc.meta_cases(name))
    for flip in oc.FLIPS:
        cfg = oc.config(name, flip)
        _, meta = oc.oracle_observe(cfg, _states(oc.meta_cases(name)), None)
        for k, case in enumerate(oc.meta_cases(name)):
            bad = oc.compare(None, meta[k], None, meta_want[k])
            assert not bad, f"{name} flip {flip} {case.name}: " + "; ".join(bad)
            rows += meta[k].shape[0]
        if name not in oc.PLANE_MAPS:
            continue
        assert rec[mgo.key(name, "planes")].shape[:2] == (4, len(oc.plane_cases(name)))
        for mask in oc.masks(name):
            obs, _ = oc.oracle_observe(cfg, _states(oc.plane_cases(name)), mask)
            want = recorded_planes(rec, name, flip, mask)
            for k, case in enumerate(oc.plane_cases(name)):
                bad = oc.compare(obs[k], None, want[k], None)
                assert not bad, f"{name} flip {flip} mask {mask} {case.name}: " + "; ".join(bad)
                rows += obs[k].shape[0]
    return rows


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def test_the_table_stays_inside_its_domain():
    assert set(oc.PLANE_MAPS) | {"wide16"} == set(oc.MAP_NAMES) and {"term16", "tag16", "tag", "flags"} <= set(oc.MAP_NAMES)
    assert [oc.shape(m)[0] for m in ("term16", "tag16", "tag", "flags")] == [16, 16, 6, 4]
    n, c, g, _ = oc.shape("term16")
    assert n * c * g * g == 11264 and oc.codes("term16") == list(range(14))
    n, c, g, _ = oc.shape("tag")
    assert n * c * g * g == 4860 and 4860 % 16 != 0
    for name in oc.MAP_NAMES:
        n, c, g, m = oc.shape(name)
        ty, full, cs = oc.types(name), oc.type_hp(name), set(oc.codes(name))
        assert all(t < n for t in ty), "the reference indexes agent_hp by the type id"
        assert sorted(oc.teams(name)).count(0) == n // 2  # (the metadata order below assumes even teams)
        cases = oc.meta_cases(name) + oc.plane_cases(name)
        assert len(cases) <= oc.MAX_ENVS and len({x.name for x in cases}) == len(cases)
        for case in cases:
            s = case.state
            assert all(0 <= int(x) <= 2 ** 31 - 2 for x in s["team_captures"]), case.name
            assert 0 <= s["step_count"] < 2 ** 28, case.name
            assert s["grid"].shape == (g, g) and set(s["grid"].reshape(-1).tolist()) <= cs, case.name
            assert s["pos"].shape == (n, 2) and s["pos"].min() >= 0 and s["pos"].max() < g, case.name
            for j in range(n):  # the quotient element hp(j) shows, as the double division gives it
                q = float(s["hp"][ty[j]]) / float(full[ty[j]])
                assert 0 <= q < 256, (case.name, j, q)
        # every quotient of the list is planted (times the agent's own type's full hp), pairwise distinct within a case
        seen = set()
        for r in range(4):
            hp = oc.meta_case(name, f"hp-{r}").state["hp"]
            qs = [oc.HP_QUOTIENTS.index(next(q for q in oc.HP_QUOTIENTS if q * full[ty[i]] == hp[i])) for i in range(4)]
            assert len(set(qs)) == 4
            seen |= set(qs)
        assert seen == set(range(8))
    assert oc.masks("term16") == [0, 0xFFFF, None, 0xCCCC]  # teams alternate with the index: every other agent of each team is ..1100
    for name in oc.PLANE_MAPS:
        for mask in oc.masks(name)[3:]:
            assert {2 * t + int(r) for t, r in zip(oc.teams(name), oc.reversed_views(name, mask))} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", oc.PLANE_MAPS)
def test_every_code_stands_in_every_cell_and_viewers_do_not_follow_the_grid(name):
    K, (n, _, g, _) = len(oc.codes(name)), oc.shape(name)
    grids = np.stack([oc.grid(name, k) for k in range(K)])
    assert all(sorted(grids[:, r, c].tolist()) == oc.codes(name) for r in range(g) for c in range(g))
    cases = oc.plane_cases(name)
    assert [np.array_equal(cases[k].state["grid"], grids[k]) for k in range(K)] == [True] * K
    shared = foreign = 0
    for case in cases:
        pos, gr = case.state["pos"], case.state["grid"]
        shared += len({tuple(p) for p in pos.tolist()}) < n
        own = [4 + ty + 4 * te for te, ty in zip(oc.teams(name), oc.types(name))]
        foreign += sum(int(gr[tuple(pos[i])]) != own[i] for i in range(n))
    assert shared >= (3 if n == 16 else 2) and foreign >= n * len(cases) // 2
    assert sum(len({tuple(p) for p in c.state["pos"].tolist()}) == 1 for c in cases) == 2  # all N on one cell
    corners = {(0, 0), (0, g - 1), (g - 1, 0), (g - 1, g - 1)}
    assert sum({tuple(p) for p in c.state["pos"].tolist()} == corners for c in cases) >= 1


# ---- the oracle against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.MAP_NAMES)
def test_the_oracle_equals_the_recorded_reference(record, name):
    n = oc.shape(name)[0]
    planes = len(oc.plane_cases(name)) * 4 if name in oc.PLANE_MAPS else 0
    assert _oracle_against(record, name) == 4 * n * (len(oc.meta_cases(name)) + planes)  # no row left out


@pytest.fixture
def reference():
    cwd = os.getcwd()
    before = set(sys.modules)
    Ref, _ = _refimport.import_reference()  # (leaves cwd in the reference: its ctor opens cwd/img/*.png)
    stubs = [m for m in ("IPython", "IPython.display", "seaborn", "imageio", "wandb", "ray") if m not in before]
    yield Ref
    for m in stubs:  # (later test modules must not find the stand-ins: matplotlib asks a loaded IPython for its shell)
        sys.modules.pop(m, None)
    os.chdir(cwd)


@pytest.mark.skipif(not _refimport.available(), reason="the reference is present in the build container only")
@pytest.mark.filterwarnings("ignore:overflow encountered in cast")
def test_the_oracle_equals_the_live_reference_and_recording_again_gives_the_committed_bytes(reference, tmp_path):
    live = mgo.record(reference, oc, mgr)
    for name in oc.MAP_NAMES:
        _oracle_against(live, name)
    again = str(tmp_path / "reference.npz")
    mgr.save(again, live)
    assert open(again, "rb").read() == open(mgo.OUT, "rb").read()


# ---- the conversion's classes --------------------------------------------------------------------------------------------------------------
def _element_values(name, case):
    """-> [(element, viewers' team, the exact value the element holds)] of a metadata case"""
    s = case.state
    a, b = (int(x) for x in s["team_captures"])
    return [(0, None, F(int(s["step_count"]), oc.game_steps(name))), (1, 0, F(a + 1, b + 1)), (1, 1, F(b + 1, a + 1))]


def test_half_of_on_values_worked_by_hand():
    for q, bits, cls in ((F(3, 2), 0x3E00, "exact normal"), (2049, 0x6800, "normal tie, even mantissa"), (2051, 0x6802, "normal tie, odd mantissa"),
                         (F(4095, 2), 0x6800, "carry into the exponent"), (65519, 0x7BFF, "largest finite"), (65504, 0x7BFF, "largest finite"),
                         (65520, 0x7C00, "overflow by rounding"), (2 ** 31 - 1, 0x7C00, "overflow"), (F(1, 2 ** 25), 0, "subnormal tie, even"),
                         (F(3, 2 ** 25), 2, "subnormal tie, odd"), (F(4095, 2 ** 26), 0x0400, "subnormal carrying into the smallest normal"),
                         (F(1, 2 ** 26), 0, "underflow"), (F(3, 2 ** 26), 1, "subnormal"), (F(1, 20000), 0x0347, "subnormal"), (0, 0, "zero"),
                         (F(1, 3), 0x3555, "normal rounded down"), (F(3, 5), 0x38CD, "normal rounded up"), (F(1, 2 ** 14), 0x0400, "exact normal")):
        assert oc.half_of(q) == (bits, cls), q


def test_every_class_occurs_through_both_elements_and_the_classifier_gives_the_recorded_bits(record):
    seen = {0: set(), 1: set()}
    for name in oc.MAP_NAMES:
        meta = record[mgo.key(name, "meta")]
        tm = oc.teams(name)
        for k, case in enumerate(oc.meta_cases(name)):
            for element, team, q in _element_values(name, case):
                bits, cls = oc.half_of(q)
                seen[element].add(cls)
                # the reference (and the device) round twice, to a double and then to a half: on this table that changes nothing
                if q.denominator & (q.denominator - 1):
                    assert oc.half_of(F(q.numerator / q.denominator)) == (bits, cls), (name, case.name, element)
                for i in range(len(tm)):
                    if team in (None, tm[i]):
                        assert int(meta[k, i, element]) == bits, (name, case.name, element, i, cls)
    assert seen[0] == set(oc.CLASSES), set(oc.CLASSES) - seen[0]
    assert seen[1] == set(oc.CLASSES) - {"zero"}, set(oc.CLASSES) - seen[1]  # (a ratio of two positive counts is not zero)


# ---- every hp and flag element shows its agent ---------------------------------------------------------------------------------------------
def metadata_order(name, viewer):
    """The agents whose (hp, flag) pairs fill elements 6.. of ``viewer``'s row, in order (gridworld_ctf.py:1044-1067): itself, its
    team-mates and then its opponents, both in index order and cut to N // 2."""
    tm = oc.teams(name)
    half = len(tm) // 2
    mates = [i for i in range(len(tm)) if tm[i] == tm[viewer]][:half]
    opponents = [i for i in range(len(tm)) if tm[i] != tm[viewer]][:half]
    return [viewer] + [i for i in mates if i != viewer] + opponents


@pytest.mark.parametrize("name", oc.MAP_NAMES)
def test_every_flag_element_shows_one_agent(record, name):
    meta, n, nb = record[mgo.key(name, "meta")], oc.shape(name)[0], oc.flag_case_count(name)
    rows = [meta[[c.name for c in oc.meta_cases(name)].index(f"flag-{k}")] for k in range(nb)]
    for viewer in range(n):
        order = metadata_order(name, viewer)
        assert sorted(order) == list(range(n))
        for slot, agent in enumerate(order):
            seq = [int(rows[k][viewer, 7 + 2 * slot]) for k in range(nb)]
            assert set(seq) <= {0, ONE} and seq[-1] == ONE
            assert sum((seq[k] == ONE) << k for k in range(nb - 1)) == agent, (viewer, slot)


@pytest.mark.parametrize("name", oc.MAP_NAMES)
def test_every_hp_element_shows_one_agent_and_its_divisor(record, name):
    meta, n = record[mgo.key(name, "meta")], oc.shape(name)[0]
    ty, full = oc.types(name), oc.type_hp(name)
    rows = [meta[[c.name for c in oc.meta_cases(name)].index(f"hp-{r}")] for r in range(4)]
    planted = [oc.hp_planted(name, r) for r in range(4)]
    divisors = sorted({full[t] for t in ty})
    shown = lambda v, d: [oc.half_of(math.floor(F(planted[r][v]) / F(d)))[0] for r in range(4)]
    candidates = {(v, d): shown(v, d) for v in range(4) for d in divisors}
    assert len({tuple(s) for s in candidates.values()}) == len(candidates)  # no two (source agent, divisor) look alike
    sources = set()
    for viewer in range(n):
        for slot, agent in enumerate(metadata_order(name, viewer)):
            seq = [int(rows[r][viewer, 6 + 2 * slot]) for r in range(4)]
            # the quirk: the hp of the agent whose INDEX is type(agent), over the full hp of type(agent)
            assert [k for k, s in candidates.items() if s == seq] == [(ty[agent], full[ty[agent]])], (viewer, slot, seq)
            sources.add(ty[agent])
    assert sources == set(ty)
    if name in ("term16", "wide16", "tag"):
        assert sources == {0, 1, 2, 3}
    if name == "wide16":
        assert len(divisors) == 4
    assert max(int(r.max()) for r in rows) >= oc.half_of(255)[0]


# ---- the transition sequence -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.PLANE_MAPS)
def test_the_transition_sequence_holds_every_ordered_pair_of_codes(name):
    cs = oc.codes(name)
    K = len(cs)
    assert oc.transition_renders(name) == K
    pairs, before = set(), oc.transition_states(name, 0)
    assert len(before) == K + 1
    for r in range(1, K):
        after = oc.transition_states(name, r)
        this = set()
        for e in range(K):
            this |= set(zip(before[e]["grid"].reshape(-1).tolist(), after[e]["grid"].reshape(-1).tolist()))
            assert not np.array_equal(before[e]["pos"], after[e]["pos"])  # redrawn
        assert this == {(cs[k], cs[(k + r) % K]) for k in range(K)}  # the shift by r
        assert np.array_equal(before[K]["grid"], after[K]["grid"]) and np.array_equal(before[K]["pos"], after[K]["pos"])
        pairs |= this
        before = after
    assert pairs == {(a, b) for a in cs for b in cs if a != b} and (name != "term16" or len(pairs) == 182)
    # the shift by one consists of plane cases: the record covers it
    cases = oc.plane_cases(name)
    for r in (0, 1):
        for e, s in enumerate(oc.transition_states(name, r)[:K]):
            k = oc.transition_grids(name, r)[e]
            assert k == (e + r) % K and np.array_equal(s["grid"], cases[k].state["grid"]) and np.array_equal(s["pos"], cases[k].state["pos"])


# ---- the compare function reports what is wrong ------------------------------------------------------------------------------------------------
def test_compare_accepts_the_oracle_itself(record):
    cfg = oc.config("term16", 1)
    obs, _ = oc.oracle_observe(cfg, _states(oc.plane_cases("term16")), 0xCCCC)
    _, meta = oc.oracle_observe(cfg, _states(oc.meta_cases("term16")), None)
    assert oc.compare(obs, meta, obs.copy(), meta.copy()) == []
    assert oc.compare(obs, meta.view(np.float16), recorded_planes(record, "term16", 1, 0xCCCC), record[mgo.key("term16", "meta")]) == []


def test_wrong_input_one_metadata_bit_flipped(record):
    want = record[mgo.key("tag", "meta")]
    got = want.copy()
    got[17, 3, 1] ^= 1  # the last place of one capture ratio
    bad = oc.compare(None, got, None, want)
    assert [b.split(":")[0] for b in bad] == ["metadata"] and "(17, 3, 1)" in bad[0], bad


def test_wrong_input_two_agents_hp_swapped(record):
    name = "term16"
    k = [c.name for c in oc.meta_cases(name)].index("hp-1")
    s = dict(oc.meta_cases(name)[k].state)
    s["hp"] = s["hp"].copy()
    s["hp"][[0, 1]] = s["hp"][[1, 0]]
    obs, meta = oc.oracle_observe(oc.config(name), [s], None)
    want_obs, _ = oc.oracle_observe(oc.config(name), [oc.meta_cases(name)[k].state], None)
    bad = oc.compare(obs[0], meta[0], want_obs[0], record[mgo.key(name, "meta")][k])
    assert [b.split(":")[0] for b in bad] == ["metadata"], bad


def test_wrong_input_one_plane_bit_moved_by_one_cell(record):
    want = recorded_planes(record, "flags", None, None)
    got = want.copy()
    case, agent, plane, r, c = (int(x) for x in np.argwhere(want[:, :, :, :, :-1] == 1)[5])
    assert got[case, agent, plane, r, c + 1] == 0 or plane > 0
    got[case, agent, plane, r, c], got[case, agent, plane, r, c + 1] = got[case, agent, plane, r, c + 1], 1
    bad = oc.compare(got, None, want, None)
    assert [b.split(":")[0] for b in bad] == ["planes"], bad


def test_wrong_input_a_view_flipped_on_the_wrong_axis(record):
    name = "tag"
    every = oc.masks(name)[1]
    obs, meta = oc.oracle_observe(oc.config(name, 0), _states(oc.plane_cases(name)), every)
    assert oc.compare(obs, None, recorded_planes(record, name, 0, every), None) == []
    for other in (None, 1, 2):
        bad = oc.compare(obs, None, recorded_planes(record, name, other, every), None)
        assert [b.split(":")[0] for b in bad] == ["planes"], (other, bad)
    assert oc.compare(obs, None, recorded_planes(record, name, 1, 0), None) != []  # nor is it the view that is not reversed
    assert abi.REVERSE_DEFAULT not in oc.masks(name)  # (the default is None in the table; oracle_observe translates it)

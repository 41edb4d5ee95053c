"""The rule suite without a GPU (tests/_rule_cases.py is the table): the oracle, planted with ``set_state`` and seeded as each replica,
equals what the reference did from the same planted state (tests/golden/rules/reference.npz, recorded by
tests/golden/make_golden_rules.py) at every step; every scenario's event takes place in at least half of its replicas; at each of the
step's three multiply-then-add sites some recorded result differs between two roundings and one; and the shared compare function reports
each of four deliberately wrong "things under test".

tests/test_gpu_rules.py relies on the first two: it compares the kernels with the oracle and does not measure its own inputs."""
import os
import sys
from fractions import Fraction as F

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import _refimport  # noqa: E402
import make_golden_rules as mgr  # noqa: E402

import _rule_cases as rc  # noqa: E402
from _cases import abi  # noqa: E402


@pytest.fixture(scope="module")
def record():
    """(scenario name, replica, step) -> the reference's outputs of that step in the compare function's form"""
    with np.load(mgr.OUT) as z:
        assert sorted(z.files) == sorted(mgr.key(m, f) for m in rc.MAP_NAMES for f in mgr.FIELDS)
        out = {}
        for m in rc.MAP_NAMES:
            recs = mgr.records_of(rc, m)
            arrs = {f: z[mgr.key(m, f)] for f in mgr.FIELDS}
            assert all(len(a) == len(recs) for a in arrs.values()), m
            for k, (sc, r, t) in enumerate(recs):
                row = {f: arrs[f][k] for f in mgr.FIELDS}
                row["team_captures"] = row["team_captures"].tolist()
                out[sc.name, r, t] = row
    return out


@pytest.fixture(scope="module")
def runs():
    """(scenario name, replica) -> (state before, the oracle's outputs of every step)"""
    return {(sc.name, r): rc.run_oracle(sc, r) for sc in rc.SCENARIOS for r in range(rc.R)}


def _summarised(out):
    """an oracle step's outputs with the generators in the record's form"""
    o = dict(out, rng=rc.rng_summary(out["py"], out["np"]))
    del o["py"], o["np"]
    return o


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def test_the_table_is_what_the_suites_assume():
    assert rc.R == 8 and len({s.name for s in rc.SCENARIOS}) == len(rc.SCENARIOS) >= 60
    for name, kw in rc.MAPS.items():
        n, g = len(kw["AGENT_CONFIG"]), kw["GRID_SIZE"]
        assert 7 <= g <= 9 and (2 <= n <= 8 or (name in ("tag16", "term16") and n == 16))
    assert {kw["TAG_PROBABILITY"] for kw in rc.MAPS.values()} == {0.5, 1.0}
    for consts in ("REF", "VIS"):
        cfg, _ = rc.build("term", consts)
        assert [getattr(cfg, f) for f in rc.CONSTS[consts]] == list(rc.CONSTS[consts].values())
    untouched, _ = rc.cfgmod.build_config(rc.MAPS["term"])
    assert [getattr(untouched, f) for f in rc.REF] == list(rc.REF.values())  # REF is what build_config hard-codes
    vis = list(rc.VIS.values())
    assert len(set(vis)) == 6 and all(v != 0 and F(v).denominator > 2 ** 20 for v in vis)  # non-zero, pairwise distinct, non-dyadic
    assert all(F(v).denominator > 2 ** 20 for v in (rc.DMG_G, rc.DMG_S, rc.MULT, rc.COST, rc.VMIN, rc.HEAL_T))
    assert rc.handles() == [("flags", "VIS"), ("miner", "VIS"), ("tag", "VIS"), ("tag16", "VIS"), ("term", "REF"), ("term", "VIS"), ("term16", "REF"),
                            ("term16", "VIS"), ("vault", "VIS")]
    assert all(len(rc.rows_of(m, c)) <= 200 for m, c in rc.handles())
    seeds = [rc.seed_of(sc, r) for sc in rc.SCENARIOS for r in range(rc.R)]
    assert len(set(seeds)) == len(seeds) and max(seeds) < 2 ** 31


# ---- replay and coverage ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("map_name", rc.MAP_NAMES)
def test_the_oracle_equals_the_recorded_reference(record, runs, map_name):
    for sc, r in rc.rows_of(map_name):
        _, outs = runs[sc.name, r]
        for t, out in enumerate(outs):
            want = record[sc.name, r, t]
            ctx = f"{sc.name} replica {r} step {t}"
            if want["raised"]:  # the reference's own failure: no open cell round the spawn
                assert sc.status_only and out["status"] & abi.ST_NO_RESPAWN, ctx
                continue
            assert out["status"] == 0 and not sc.status_only, ctx
            bad = rc.compare(_summarised(out), want)
            assert not bad, f"{ctx}: " + "; ".join(bad)


@pytest.mark.parametrize("sc", rc.SCENARIOS, ids=[s.name for s in rc.SCENARIOS])
def test_the_event_takes_place_in_at_least_half_of_the_replicas(runs, sc):
    if sc.status_only:
        assert all(outs[-1]["status"] == abi.ST_NO_RESPAWN for _, outs in (runs[sc.name, r] for r in range(rc.R)))
        return
    hits = sum(rc.event(sc, *runs[sc.name, r]) for r in range(rc.R))
    assert 2 * hits >= rc.R, f"{sc.name}: the event takes place in {hits} of {rc.R} replicas"


@pytest.mark.parametrize("k", range(1, 9))
def test_the_multi_kill_rows_put_k_opponents_out_in_one_turn(runs, k):
    """... in EVERY replica, whatever the shuffled order, and the k respawns land on k different cells of the window"""
    sc = rc.BY_NAME[f"one_tagger_{k}_out_in_one_turn"]
    for r in range(rc.R):
        before, outs = runs[sc.name, r]
        moved = [i for i in range(16) if not np.array_equal(before["pos"][i], outs[0]["pos"][i])]
        assert len(moved) == k and all(i % 2 == 1 and rc._in_window("tag16", outs[0], i) for i in moved)
        assert len({tuple(outs[0]["pos"][i]) for i in moved}) == k and int(outs[0]["metrics"][rc.M["respawn_tag_count"]][0]) == k


# ---- the three multiply-then-add sites ---------------------------------------------------------------------------------------------------
def _once(r, a, b, sign):
    """r + sign * a * b rounded once, as a contracted multiply-add gives it"""
    return float(F(r) + sign * F(a) * F(b))


def _differs(twice, r, a, b, sign):
    """``twice`` (a recorded value) is r + sign * (a * b) with the product rounded first, and a single rounding gives another double"""
    assert twice == r + sign * (a * b)
    return twice != _once(r, a, b, sign)


def test_each_multiply_add_site_has_a_result_that_one_rounding_would_change(record):
    v = rc.VIS
    # hp - damage * multiplier (the guardian inside its zone)
    hp = float(record["guardian_three_from_its_flag_multiplied", 0, 0]["hp"][1])
    assert _differs(hp, 2.0, rc.DMG_G, rc.MULT, -1)
    # ... and where two roundings leave exactly 0 (a respawn), one leaves a positive remainder (none)
    assert rc.HIT3 - rc.DMG_G * rc.MULT == 0.0 and _once(rc.HIT3, rc.DMG_G, rc.MULT, -1) > 0
    assert rc._in_window("tag", record["hit_to_exactly_zero_respawns", 0, 0], 1)
    # r - x * capture * punishment: the capturer's and the bystander's reward when both teams capture
    rw = record["both_teams_capture_in_one_step", 0, 0]["r64"]
    assert _differs(float(rw[0]), rc.V_RCAP, 1.0 * v["reward_capture"], v["opp_capture_punishment"], -1)
    assert _differs(float(rw[2]), rc.V_STEP, 1.0 * v["reward_capture"], v["opp_capture_punishment"], -1)
    # r +- margin * scalar, VIS: a win by three
    rw = record["last_step_5_to_2_VIS", 0, 0]["r64"]
    assert _differs(float(rw[0]), rc.V_STEP, 3, v["win_margin_scalar"], +1)
    # ... and with the reference's own constants: -0.5 + 3 * 0.1, a three-capture win on a step where the other side captures
    rw = record["three_ahead_while_the_other_side_captures_REF", 0, 0]["r64"]
    assert float(rw[0]) == -0.5 + 3 * 0.1 and _differs(float(rw[0]), -0.5, 3, 0.1, +1)


# ---- the compare function reports what is wrong ------------------------------------------------------------------------------------------
def test_compare_accepts_the_oracle_itself(runs, record):
    for name in ("both_teams_capture_in_one_step", "carrier_tagged_out_drops_the_flag", "last_step_5_to_2_VIS", "one_tagger_8_out_in_one_turn"):
        _, outs = runs[name, 3]
        for t, out in enumerate(outs):
            assert rc.compare(out, out) == [] and rc.compare(_summarised(out), record[name, 3, t]) == []


def test_compare_reports_a_status_bit(runs):
    _, outs = runs["spawn_window_full", 0]
    assert outs[0]["status"] == abi.ST_NO_RESPAWN
    assert rc.compare(outs[0], outs[0], state=False) == []
    bad = rc.compare(dict(outs[0], status=0), outs[0], state=False)
    assert [b.split(":")[0] for b in bad] == ["status"], bad


def test_mutation_ref_constants_against_a_vis_record(record):
    sc = rc.BY_NAME["both_teams_capture_in_one_step"]
    _, outs = rc.run_oracle(sc, 0, cfg=rc.build(sc.map, "REF")[0])
    bad = rc.compare(_summarised(outs[0]), record[sc.name, 0, 0])
    assert [b.split(":")[0] for b in bad] == ["r64", "r32"], bad  # the rules are the same: only the rewards differ


def test_mutation_tag_reward_credited_to_the_victim(runs, record):
    sc = rc.BY_NAME["carrier_tagged_out_drops_the_flag"]
    _, outs = runs[sc.name, 0]
    wrong = _summarised(outs[0])
    r = wrong["r64"].copy()
    assert r[0] == rc.V_STEP + rc.V_TAG and r[1] == rc.V_STEP
    r[0], r[1] = r[1], r[0]  # (what a wrong bit in the mask of taggers gives)
    wrong.update(r64=r, r32=r.astype(np.float32))
    bad = rc.compare(wrong, record[sc.name, 0, 0])
    assert [b.split(":")[0] for b in bad] == ["r64", "r32"], bad


def test_mutation_losers_terminal_term_dropped(runs, record):
    sc = rc.BY_NAME["last_step_5_to_2_VIS"]
    _, outs = runs[sc.name, 0]
    wrong = _summarised(outs[0])
    r = wrong["r64"].copy()
    r[1] = r[3] = rc.V_STEP
    assert r[1] != outs[0]["r64"][1]
    wrong.update(r64=r, r32=r.astype(np.float32))
    bad = rc.compare(wrong, record[sc.name, 0, 0])
    assert [b.split(":")[0] for b in bad] == ["r64", "r32"], bad


def test_mutation_rewards_with_one_rounding(runs, record):
    """in float64 alone: the float32 rewards are too coarse to see one rounding, the float64 ones must"""
    v = rc.VIS
    for name, fused in (("last_step_5_to_2_VIS", lambda r: [_once(rc.V_STEP, 3, v["win_margin_scalar"], +1), r[1]] * 2),
                        ("both_teams_capture_in_one_step", lambda r: [_once(rc.V_RCAP, 1.0 * v["reward_capture"], v["opp_capture_punishment"], -1)] * 2
                         + [_once(rc.V_STEP, 1.0 * v["reward_capture"], v["opp_capture_punishment"], -1)] * 2)):
        _, outs = runs[name, 0]
        wrong = _summarised(outs[0])
        r = np.array(fused(wrong["r64"]), np.float64)
        wrong.update(r64=r, r32=r.astype(np.float32))
        bad = rc.compare(wrong, record[name, 0, 0])
        assert [b.split(":")[0] for b in bad] == ["r64"], bad
    # ... and the hp: a fused hit is a state mismatch
    _, outs = runs["guardian_three_from_its_flag_multiplied", 0]
    wrong = _summarised(outs[0])
    wrong["hp"] = wrong["hp"].copy()
    wrong["hp"][1] = _once(2.0, rc.DMG_G, rc.MULT, -1)
    bad = rc.compare(wrong, record["guardian_three_from_its_flag_multiplied", 0, 0])
    assert [b.split(":")[0] for b in bad] == ["hp"], bad


# ---- the record is what the recorder writes ----------------------------------------------------------------------------------------------
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
def test_recording_again_gives_the_committed_bytes(reference, tmp_path):
    rec = {}
    for map_name in rc.MAP_NAMES:
        rec.update(mgr.record_map(reference, rc, map_name, abi.METRIC_NAMES))
    again = str(tmp_path / "reference.npz")
    mgr.save(again, rec)
    assert open(again, "rb").read() == open(mgr.OUT, "rb").read()

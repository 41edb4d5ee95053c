"""k_step's rules from planted states, every reward term visible (tests/_rule_cases.py is the table, tests/test_rules_cpu.py shows that
the oracle equals the recorded reference on every row of it and that every row's event takes place; nothing of that is measured here).

One handle per (map, constant set): env k runs row k of ``rows_of`` — a scenario and one of its 8 replicas — seeded as its oracle twin
and planted, all rows at once, with one ``set_states`` call.  After every step each env's state arrays, float64 and float32 rewards,
done and both generators' whole states are compared with the twin's by the table's compare function, and the handle's status with the
OR of the twins' statuses.  A row whose scenario is over keeps stepping with nobody moving, twin and env alike.

The whole table also runs in rng_mode="counter_direct" against counter-mode twins; tests/test_counter_direct_cpu.py shows with the
oracle alone that every row's event takes place on that tape too."""
import numpy as np
import pytest

import _rule_cases as rc
from _cases import abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GET_TO_COMPARE = dict(inventory="inv")  # get_states' names -> the compare function's


def _planted(rows, device, fields):
    stack = lambda f, dtype: torch.from_numpy(np.stack([np.asarray(sc.state[f]) for sc, _ in rows]).astype(dtype)).to(device)
    dtypes = dict(grid=np.uint8, pos=np.int8, hp=np.float64, has_flag=np.uint8, inv=np.int32, perm=np.uint8, step_count=np.int32,
                  team_captures=np.int32, done=np.uint8)
    return {f: stack(GET_TO_COMPARE.get(f, f), dtypes[GET_TO_COMPARE.get(f, f)]) for f in fields}


def _outputs(vec, counter):
    """every env's outputs of the last step -> [dict in the compare function's form]"""
    st = {GET_TO_COMPARE.get(f, f): t.cpu().numpy() for f, t in vec.get_states().items()}
    r64, r32, done = vec.rewards64.cpu().numpy(), vec.rewards.cpu().numpy(), vec.done.cpu().numpy()
    if counter:
        gens = dict(rng=vec.get_rng_counters().cpu().numpy())
    else:
        py, npw = vec.get_rng_states()
        gens = dict(py=py.cpu().numpy().view(np.uint32), np=npw.cpu().numpy().view(np.uint32))
    outs = []
    for e in range(vec.n_envs):
        o = {k: v[e] for k, v in st.items()}
        o.update(team_captures=o["team_captures"].tolist(), r64=r64[e], r32=r32[e], done_out=int(done[e]))
        o.update({k: v[e] for k, v in gens.items()})
        outs.append(o)
    return outs


def _run(monkeypatch, map_name, consts, log_metrics=True, lanes=None, observe=False, mode="mt19937", auto_reset=None, one_launch=False,
         launches=None):
    """``mode``: the handle's rng_mode; the twins of both counter modes are counter-mode oracles seeded (s, s ^ 0x5DEECE66D).
    ``auto_reset`` None: one pass per value the map's scenarios ask for, each comparing the rows that ask for it; True / False: one
    pass with that flag in which every twin follows it.  ``observe``: through step_observe, as one launch with ``one_launch``
    (``launches``: how many the handle then takes, where the mode does not follow the switch)."""
    if observe:
        monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", "1" if one_launch else "0")  # read at every call
    if lanes is not None:
        monkeypatch.setenv("CTF_STEP_W", str(lanes))  # read when the handle is created
    counter = mode != "mt19937"
    rows = rc.rows_of(map_name, consts)
    n_envs = len(rows)
    assert 0 < n_envs <= 200
    seeds = np.array([rc.seed_of(sc, r) for sc, r in rows], np.uint64)
    np_seeds = np.array([rc.counter_seeds(sc, r)[1] for sc, r in rows], np.uint64) if counter else seeds
    vec = rc.open_vec(monkeypatch, map_name, consts, n_envs, device=0, py_seeds=seeds, np_seeds=np_seeds, log_metrics=log_metrics,
                      rng_mode=mode)
    assert not observe or vec.step_observe_launches() == (launches or (1 if one_launch else 2))
    cfg = rc.build(map_name, consts, log_metrics=log_metrics, counter=counter)[0]
    steps = max(len(sc.actions) for sc, _ in rows)
    planted = _planted(rows, vec.device, [f for f in abi.STATE_FIELDS[:-2]])
    passes = sorted({sc.auto_reset for sc, _ in rows}) if auto_reset is None else [auto_reset]
    for flag in passes:
        vec.seed(seeds, np_seeds)
        vec.set_states(planted)
        twins = [rc.oracle_env(sc, r, cfg, seeds=(int(seeds[e]), int(np_seeds[e]))) for e, (sc, r) in enumerate(rows)]
        defined = np.ones(n_envs, bool)  # (False from the step on at which the twin reports a status: no respawn cell)
        for t in range(steps):
            acts = torch.from_numpy(np.stack([rc.actions_at(sc, t) for sc, _ in rows])).to(vec.device)
            if observe:
                vec.step_observe(acts, auto_reset=flag, want_f64=True)
            else:
                vec.step(acts, auto_reset=flag, want_f64=True)
            got = _outputs(vec, counter)
            status = 0
            for e, (sc, r) in enumerate(rows):
                want = rc.oracle_step(twins[e], sc, t, counter=counter, auto_reset=flag)
                status |= want["status"]
                defined[e] &= want["status"] == 0
                if auto_reset is None and sc.auto_reset != flag:
                    continue
                bad = rc.compare(got[e], want, metrics=log_metrics, state=bool(defined[e]))
                assert not bad, f"{mode} {map_name} {consts} W={lanes} auto_reset={flag}: {sc.name} replica {r} step {t}: " + "; ".join(bad)
            assert vec.status() == status, f"{mode} {map_name} {consts} W={lanes} auto_reset={flag} step {t}: status"
        assert defined.sum() >= n_envs - rc.R * sum(sc.status_only for sc in rc.SCENARIOS if sc.map == map_name)
    vec.close()


@pytest.mark.parametrize("map_name,consts", rc.handles(), ids=[f"{m}-{c}" for m, c in rc.handles()])
def test_planted_rules_match_the_oracle(map_name, consts, monkeypatch):
    _run(monkeypatch, map_name, consts)


@pytest.mark.parametrize("map_name", rc.LANE_MAPS)
@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_the_tagging_rows_at_every_lane_width(map_name, lanes, monkeypatch):
    """one tagger putting 1..8 opponents out in one turn, with W lanes per env: several tagging passes per turn (W < opponents) or idle
    lanes (W > opponents), the respawn draws in between"""
    _run(monkeypatch, map_name, "VIS", lanes=lanes)


def test_the_tagging_rows_without_counters(monkeypatch):
    """k_step<METRICS = false>: everything but the counters"""
    _run(monkeypatch, "tag", "VIS", log_metrics=False)


@pytest.mark.parametrize("map_name,one_launch", [("term", False), ("term16", False), ("term16", True)])
@pytest.mark.parametrize("consts", ["REF", "VIS"])
def test_the_terminal_rows_through_step_observe(map_name, one_launch, consts, monkeypatch):
    """step_observe(auto_reset=True): every done env is reset first, the rows planted as done included.  The 16-agent map's observation
    block is one the tile render takes: there also as ONE launch (k_step_observe)."""
    _run(monkeypatch, map_name, consts, observe=True, auto_reset=True, one_launch=one_launch)


def test_the_flag_rows_in_counter_mode(monkeypatch):
    """rng_mode="counter" against the oracle reading the same tape; the generators' states are the words consumed"""
    _run(monkeypatch, "flags", "VIS", mode="counter")


# ---- rng_mode="counter_direct": the whole table -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("map_name,consts", rc.handles(), ids=[f"{m}-{c}" for m, c in rc.handles()])
def test_planted_rules_in_counter_direct(map_name, consts, monkeypatch):
    """every row of the table with the Philox tape drawn inside the step: the tag compare at TAG_PROBABILITY 0.5 and 1, the respawn
    draws of 1..8 victims of one turn (16 agents: past the np.random window), the shuffles"""
    _run(monkeypatch, map_name, consts, mode="counter_direct")


@pytest.mark.parametrize("map_name", rc.LANE_MAPS)
@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_the_tagging_rows_at_every_lane_width_in_counter_direct(map_name, lanes, monkeypatch):
    """... with the windows' blocks spread over W lanes per env"""
    _run(monkeypatch, map_name, "VIS", lanes=lanes, mode="counter_direct")


@pytest.mark.parametrize("consts", ["REF", "VIS"])
def test_the_terminal_rows_through_step_observe_in_counter_direct(consts, monkeypatch):
    """step_observe(auto_reset=True) on the 16-agent map, whose observation block the tile render takes: with the one-launch switch on
    the mode still takes two launches (its step kernel is its own)"""
    _run(monkeypatch, "term16", consts, observe=True, auto_reset=True, mode="counter_direct", one_launch=True, launches=2)

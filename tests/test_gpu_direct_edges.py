"""rng_mode="counter_direct" at the edges of its tag compare (tests/_tie_cases.py): ``np.random.rand() < TAG_PROBABILITY`` where
the draw's 53-bit integer EQUALS the threshold, is one below it, or differs from it in the high 27 bits alone — the threshold chosen
from the tape, since a tape word cannot be — for draws whose two bytes are both parked, parked by different lanes, half parked
(the window's last byte) and not parked (computed on demand, with a second block when the draw starts at a block's last word); and
TAG_PROBABILITY at both ends of its range.  Every env has an oracle twin in counter mode, which reads the same tape with its own
float64 compare; everything is compared bit for bit after every step.  tests/test_counter_direct_cpu.py asserts on the oracle alone
that the envs run here are the deciding ones and cover those positions: nothing of that is measured here."""
import numpy as np
import pytest

import _counter_direct_cases as cd
import _rule_cases as rc
import _tie_cases as tc
import oracle
from _cases import abi, pkg
from test_gpu_rules import _outputs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MODE = "counter_direct"
TIE_STEPS = 3


def _open(n_envs, p, mode, py, npz):
    return pkg.VecGridworldCtf(n_envs, device=0, py_seeds=py, np_seeds=npz, rng_mode=mode, log_metrics=True, tune_placement=False, **tc.kwargs(p))


def _compare_step(vec, twins, acts, ctx, allowed=0):
    """one step of every env and its twin; ``allowed``: the status bits a twin may report (the handle's are then the OR of the twins')"""
    vec.step(torch.from_numpy(acts).to(vec.device), want_f64=True)
    got = _outputs(vec, True)
    status = 0
    for e, env in enumerate(twins):
        want = tc.twin_step(env, acts[e])
        assert want["status"] & ~allowed == 0, ctx
        status |= want["status"]
        bad = rc.compare(got[e], want)
        assert not bad, f"{ctx} env {e}: " + "; ".join(bad)
    assert vec.status() == status, ctx


def _tie_run(mode, r, variants, lanes=None):
    ks = tc.deciding(r)
    E = len(ks)
    for v in variants:
        p = tc.probability(r, v)
        vec = _open(E, p, mode, [tc.PY_SEED] * E, [tc.NP_SEED] * E)
        ctr = np.array([[tc.PY_COUNTER, tc.np_counter(r, k)] for k in ks], np.int64)
        vec.set_rng_counters(torch.from_numpy(ctr).to(vec.device))
        cfg = tc.config(p)
        twins = [tc.twin(cfg, r, k) for k in ks]
        for t in range(TIE_STEPS):
            acts = np.stack([tc.actions(t, e) for e in range(E)])
            _compare_step(vec, twins, acts, f"{mode} W={lanes} n* = {tc.N_STAR + r} {v} step {t} (env e: k = deciding[e])")
        vec.close()


@pytest.mark.parametrize("r", tc.RESIDUES)
@pytest.mark.parametrize("mode", [MODE, "counter"])
def test_a_draw_at_the_threshold_misses_and_one_below_it_hits(mode, r):
    """Per residue of n* one handle per variant, env e the e-th deciding k: the step's k-th rand() is the draw at n*.  One step with
    nobody moving, then two more on random actions along the tapes that have diverged between the variants.  `counter` runs the same
    cases through the ring digests."""
    _tie_run(mode, r, tc.VARIANTS)


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_the_straddling_tie_at_every_lane_width(lanes, monkeypatch):
    """n* = 3 mod 4: the draw's two words lie in different blocks, so its two bytes sit in different dwords of the window, and with
    W >= 2 lanes per env different lanes have parked them (asserted from the byte -> lane map of group_rng_setup's loop, block t is
    lane t % W's).  W = 1 cannot have that: one lane parks every block."""
    r = 3
    fill = cd.window_caps()[0]
    inside = [tc.window_byte(r, k) for k in tc.deciding(r) if tc.position_class(tc.window_byte(r, k), fill) == "inside"]
    assert inside and all(b % 4 == 3 for b in inside)
    if lanes > 1:
        assert any(tc.parking_lane(b, lanes) != tc.parking_lane(b + 1, lanes) for b in inside)
    monkeypatch.setenv("CTF_STEP_W", str(lanes))  # read when the handle is created
    _tie_run(MODE, r, ("tie", "tie+1"), lanes=lanes)


ENDS = {"0": 0.0, "2^-53": 2.0 ** -53, "1-2^-53": 1.0 - 2.0 ** -53, "1": 1.0}


@pytest.mark.parametrize("end", sorted(ENDS))
def test_the_ends_of_the_threshold(end):
    """TAG_PROBABILITY 0 (threshold 0: nothing is below it), 2**-53 (threshold 1: only the all-zero draw), 1 - 2**-53 (th = 2**27 - 1,
    tl = 2**26 - 1: every draw but the largest) and 1 (th = 2**27, which no 27-bit value reaches).  The map's spawns lie in two
    corners: at the upper end a respawn of the last steps may land past row / column 0 (CTF_ST_SPAWN_EDGE), which the oracle reports
    and places as the step does: the handle's status is the OR of the twins', and at the lower end it is 0."""
    p = ENDS[end]
    E, steps = 16, 6
    py, npz = cd.seeds(E)
    vec = _open(E, p, MODE, py, npz)
    cfg = tc.config(p)
    twins = [oracle.OracleEnv(cfg) for _ in range(E)]
    for e, env in enumerate(twins):
        env.seed(int(py[e]), int(npz[e]))
    for t in range(steps):
        acts = np.stack([oracle.philox_actions(tc.N_AGENTS, tc.FOLLOW_SEED, t, e) for e in range(E)])
        _compare_step(vec, twins, acts, f"TAG_PROBABILITY {end} step {t}", allowed=abi.ST_SPAWN_EDGE if p > 0.5 else 0)
    vec.close()

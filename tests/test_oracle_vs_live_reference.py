"""The C oracle against the reference on random configurations: the fuzz the round-4 review ran by hand (120 configs, 0 mismatches)
kept as a test.  The configurations and action tapes are drawn from fixed seeds (tests/golden/make_golden_live.py draw_trials); what the
reference did on each — per step grid, positions, f64 hp, flags, inventory, `_arr`, f64 rewards, done, both MT positions, all N
observations and metadata rows; at the end counters, visitation maps and both generators' full states — is recorded in
tests/golden/live/reference.npz (per-step 64-bit digests, end-of-trial arrays in full; re-recorded from the reference by that script).
A config on which the reference itself raises (no open respawn cell: ValueError from np.random.randint(0)) must make the oracle
report CTF_ST_NO_RESPAWN at the same step."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_live as live  # noqa: E402

import oracle  # noqa: E402
from _cases import abi, cfgmod, view_arrays  # noqa: E402


@pytest.fixture(scope="module")
def ref():
    with np.load(live.OUT) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("block", live.BLOCKS)
def test_oracle_equals_the_live_reference_on_random_configurations(ref, block):
    """Blocks 0-11: capture-dense small maps in the style of the committed fuzz fixtures.  Blocks wild0-11: configurations outside what the
    shipped maps use (tests/_cases.py wild_config: unequal teams, capture cells away from the flags, no-damage types, TAG_PROBABILITY 0,
    healing past the cap, 4x4 grids with eight agents ...): 10 of each per block."""
    wild = isinstance(block, str)
    captures = raised = 0
    trials = live.draw_trials(block)
    assert {k for k in ref if k.startswith(f"b{block}_")} == {live.key(block, tr[0], w) for tr in trials for w in ("tiles_used", "raised", "states", "views")} | {
        live.key(block, tr[0], w) for tr in trials if int(ref[live.key(block, tr[0], "raised")]) < 0 for w in ("metrics", "visitation", "team_captures", "rng_states")}
    for trial, scen, kw, seed, actions in trials:
        rec = lambda what: ref[live.key(block, trial, what)]
        n, T = len(kw["AGENT_CONFIG"]), len(actions)
        cfg, derived = cfgmod.build_config(dict(kw, SCENARIO=scen), log_metrics=True)
        assert derived["tiles_used"] == rec("tiles_used").tolist()
        o = oracle.OracleEnv(cfg)
        o.seed(seed, seed)
        g = kw["GRID_SIZE"]
        ctx = f"block {block} trial {trial} seed {seed}"
        stop, states, views = int(rec("raised")), rec("states"), rec("views")
        assert len(states) == (stop if stop >= 0 else T), ctx
        v = 0
        for t in range(T):
            if t == stop:  # the reference's own failure: no open cell round the spawn
                _, _, status = o.step(actions[t])
                assert status & abi.ST_NO_RESPAWN, ctx
                raised += 1
                break
            rw, dn, status = o.step(actions[t])
            assert status == 0, (ctx, t, status)
            s = view_arrays(o.get_state(), n, g)
            py, npw = o.get_rng_state()
            got = live.state_digest(s["grid"], s["pos"], s["hp"], s["has_flag"], s["inv"], s["perm"], rw, dn, py[624], npw[624])
            assert got == states[t], f"{ctx} step {t}: grid / positions / hp / flags / inventory / _arr / rewards / done / MT positions"
            if live.observed(t, T):
                obs, meta = o.observe()
                assert live.obs_digest(obs, meta) == views[v], f"{ctx} step {t}: observations / metadata"
                v += 1
        else:
            assert v == len(views), ctx
            s = view_arrays(o.get_state(), n, g)
            assert np.array_equal(s["metrics"], rec("metrics")), ctx
            assert np.array_equal(s["visitation"], rec("visitation")), ctx
            assert s["team_captures"] == rec("team_captures").tolist(), ctx
            py, npw = o.get_rng_state()
            assert live.rng_digest(py, npw[:624], npw[624]) == rec("rng_states")[0], ctx
            captures += sum(s["team_captures"])
    assert wild or captures + raised > 0  # (a capture-dense block without a single capture or respawn failure would not be testing much)

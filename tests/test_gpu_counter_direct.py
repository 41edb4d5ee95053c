"""rng_mode="counter_direct" (include/ctf_env.h CTF_RNG_COUNTER_DIRECT) on the GPU: the Philox tape of rng_mode="counter" drawn
inside the step kernel, nothing stored.  Same seeds, same actions -> the trajectory of "counter" and of the oracle reading that tape,
bit for bit, words consumed included; at every lane width; with draws far beyond the windows; on the reference's own recordings;
through every carrier of env state (counters as the checkpoint, snapshot records, hipGraph replays)."""
import glob
import json
import os
import types

import numpy as np
import pytest

import _counter_direct_cases as cd
import _rule_cases as rc
import oracle
from _cases import GOLDEN, Case, abi, cfgmod, kwargs_from_json, pkg, view_arrays
from test_gpu_parity import _run_against_oracle, _state_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODE = "counter_direct"


def _vec(n_envs, kwargs, mode=MODE, seeds=None, log_metrics=True):
    py, npz = seeds if seeds is not None else cd.seeds(n_envs)
    return pkg.VecGridworldCtf(n_envs, device=0, py_seeds=py, np_seeds=npz, rng_mode=mode, log_metrics=log_metrics, tune_placement=False, **kwargs)


def _same_tensors(a, b, ctx):
    assert sorted(a) == sorted(b), ctx
    for k in a:
        assert torch.equal(a[k], b[k]), f"{ctx}: {k}"


class _Pair:
    """A `counter` and a `counter_direct` handle stepped as one, for _run_against_oracle: every call goes to both, what they
    answer is compared bit for bit, and the oracle's compare then sees the counter_direct handle's answers."""

    def __init__(self, n_envs, kwargs):
        self.a, self.b = _vec(n_envs, kwargs, "counter"), _vec(n_envs, kwargs)
        self.n_envs, self.device, self.t = n_envs, self.b.device, 0

    def random_actions(self, out, **kw):
        return self.b.random_actions(out, **kw)

    def step(self, acts, **kw):
        ctx = f"counter vs counter_direct step {self.t}"
        if self.t % 2:  # the rewards and done alone in one half of the steps, with the observations in the other
            for v in (self.a, self.b):
                v.step(acts, **kw)
        else:
            for v in (self.a, self.b):
                v.step_observe(acts, **kw)
        for name in ("rewards", "rewards64", "done"):
            assert torch.equal(getattr(self.a, name), getattr(self.b, name)), f"{ctx}: {name}"
        if self.t % 20 == 19:
            _same_tensors(self.a.get_states(), self.b.get_states(), ctx + ": get_states")
            assert torch.equal(self.a.get_rng_counters(), self.b.get_rng_counters()), ctx + ": words consumed"
            for x, y in zip(self.a.counters(), self.b.counters()):
                assert torch.equal(x, y), ctx + ": counters()"
            (oa, ma), (ob, mb) = self.a.observe(), self.b.observe()
            assert torch.equal(oa, ob) and torch.equal(ma.view(torch.int16), mb.view(torch.int16)), ctx + ": observations"
        self.t += 1
        self.rewards64, self.done = self.b.rewards64, self.b.done

    def get_rng_counters(self):
        return self.b.get_rng_counters()

    def get_state(self, e):
        return self.b.get_state(e)

    def close(self):
        assert self.a.status() == 0 and self.b.status() == 0
        self.a.close()
        self.b.close()


# ---- 1. equals `counter`, bit for bit, and both equal the oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["arena_random", "split_random", "arena_stress"])
def test_counter_direct_equals_counter_and_the_oracle(name):
    case = Case(name)
    n_envs = 140
    py, npz = cd.seeds(n_envs)
    pair = _Pair(n_envs, case.kwargs)  # (without the feature: ValueError, rng_mode must be 'mt19937' or 'counter')
    alive = _run_against_oracle(pair, cd.counter_config(case.kwargs), case, py, 200, f"counter_direct {name}", np_seeds=npz, counters=True)
    assert alive.sum() >= n_envs // 2
    pair.close()


# ---- 2. every lane width ----------------------------------------------------------------------------------------------------------------
LANE_CONFIGS = {"4v4": lambda: Case("arena_stress").kwargs, "8v8": lambda: cd.BEYOND_KWARGS}


@pytest.mark.parametrize("config", sorted(LANE_CONFIGS))
@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_every_lane_width_matches_the_oracle(config, lanes, monkeypatch):
    monkeypatch.setenv("CTF_STEP_W", str(lanes))
    kwargs = LANE_CONFIGS[config]()
    n_envs = 64
    py, npz = cd.seeds(n_envs)
    vec = _vec(n_envs, kwargs)
    shape = types.SimpleNamespace(n=vec.N_AGENTS, g=vec.GRID_SIZE)
    alive = _run_against_oracle(vec, cd.counter_config(kwargs), shape, py, 60, f"counter_direct {config} W={lanes}", np_seeds=npz, counters=True)
    assert alive.sum() >= n_envs // 2 and vec.status() == 0
    vec.close()


# ---- 3. beyond the window ----------------------------------------------------------------------------------------------------------------
def test_draws_beyond_both_windows_match_the_oracle():
    """16 agents, 8 v 8 in tagging range from a planted state: every step draws 256 np.random words (the window holds at most 68)
    and 36 .. 70 `random` words (at most 44)."""
    runs = cd.beyond_oracle()
    py_share, np_share = cd.beyond_fractions(runs)
    assert py_share >= 0.25 and np_share >= 0.25, (py_share, np_share)
    E, T = cd.BEYOND_ENVS, cd.BEYOND_STEPS
    vec = _vec(E, cd.BEYOND_KWARGS)
    view = rc.to_view(cd.beyond_state())
    for e in range(E):
        vec.set_state(e, view)
    n, g = vec.N_AGENTS, vec.GRID_SIZE
    for t in range(T):
        acts = torch.from_numpy(np.stack([cd.beyond_actions(t, e) for e in range(E)])).to(vec.device)
        vec.step(acts, want_f64=True)
        r64, done, ctr = vec.rewards64.cpu().numpy(), vec.done.cpu().numpy(), vec.get_rng_counters().cpu().numpy()
        for e in range(E):
            rw, dn, status, state, words = runs[e][t]
            ctx = f"beyond the window env {e} step {t}"
            assert status == 0
            assert np.array_equal(r64[e], rw) and int(done[e]) == int(dn), ctx
            assert tuple(int(x) for x in ctr[e]) == words, ctx + ": words consumed"
            if t % 3 == 2 or t == T - 1:
                _state_equal(view_arrays(vec.get_state(e), n, g), state, ctx)
    assert vec.status() == 0
    vec.close()


# ---- 4. the reference's own recording ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "counter_*.npz"))), ids=lambda p: os.path.basename(p)[:-4])
def test_the_patched_reference_recording_replays(path):
    z = np.load(path)
    meta = json.loads(bytes(z["case_json"]).decode())
    kw = kwargs_from_json(meta)
    vec = _vec(2, kw, seeds=([meta["py_seed"], 1], [meta["np_seed"], 2]))
    n, g, T = meta["n"], meta["g"], meta["T"]
    acts = torch.zeros((2, n), dtype=torch.int8, device=vec.device)
    rows, ctrs = [], []
    for t in range(T):
        acts[0] = torch.from_numpy(z["actions"][t])
        acts[1] = torch.from_numpy(z["actions"][(t * 7 + 3) % T])
        vec.step(acts, auto_reset=True, want_f64=True)  # (the recording resets an env that is done before its next step)
        rows.append((vec.rewards64[0].clone(), vec.done[0].clone()))
        ctrs.append(vec.get_rng_counters()[0].clone())
        if t % 20 == 19 or t == T - 1:
            s = view_arrays(vec.get_state(0), n, g)
            for k in ("grid", "pos", "hp", "has_flag", "inv", "perm"):
                assert np.array_equal(s[k], z[k][t]), f"{meta['name']} step {t}: {k}"
    r64 = torch.stack([r for r, _ in rows]).cpu().numpy()
    done = torch.stack([d for _, d in rows]).cpu().numpy()
    ctr = torch.stack(ctrs).cpu().numpy()
    assert np.array_equal(r64, z["rewards"]) and np.array_equal(done.astype(bool), z["done"].astype(bool))
    assert np.array_equal(ctr[:, 0], z["py_n"].astype(np.int64)) and np.array_equal(ctr[:, 1], z["np_n"].astype(np.int64)), "words consumed"
    assert vec.status() == 0
    vec.close()


# ---- 5. counters as the checkpoint -----------------------------------------------------------------------------------------------------------
def _run(vec, acts, t0, steps):
    rows = []
    for t in range(t0, t0 + steps):
        vec.random_actions(acts, seed=0xABC, step=t)
        vec.step(acts, auto_reset=True, want_f64=True)
        rows.append(torch.cat([vec.rewards64.view(torch.int64).flatten(), vec.rewards.view(torch.int32).flatten().long(), vec.done.flatten().long()]))
    return torch.stack(rows), vec.get_rng_counters().clone(), vec.get_states()


def _restore(vec, seeds, ctr, states):
    vec.seed(*seeds)
    vec.set_rng_counters(ctr)
    vec.set_states(states)


def _same_run(a, b, ctx):
    assert torch.equal(a[0], b[0]), ctx + ": rewards / done"
    assert torch.equal(a[1], b[1]), ctx + ": words consumed"
    _same_tensors(a[2], b[2], ctx + ": states")


def test_counters_are_the_checkpoint_within_the_mode_and_across_the_two_counter_modes():
    case = Case("arena_stress")
    E = 96
    seeds = cd.seeds(E)
    direct, ring = _vec(E, case.kwargs), _vec(E, case.kwargs, "counter")
    acts = torch.empty((E, case.n), dtype=torch.int8, device=direct.device)
    _run(direct, acts, 0, 30)
    ctr, states = direct.get_rng_counters().clone(), {k: v.clone() for k, v in direct.get_states().items()}
    first = _run(direct, acts, 30, 30)
    _restore(direct, seeds, ctr, states)
    _same_run(_run(direct, acts, 30, 30), first, "counter_direct restored from its own counters")
    # the hand-over: the checkpoint of one counter mode is the other's
    _restore(ring, seeds, ctr, states)
    second = _run(ring, acts, 30, 30)
    _same_run(second, first, "counter continued from counter_direct's checkpoint")
    _restore(direct, seeds, second[1], second[2])
    back = _run(direct, acts, 60, 20)
    _same_run(_run(ring, acts, 60, 20), back, "counter_direct continued from counter's checkpoint")
    assert direct.status() == 0 and ring.status() == 0
    direct.close()
    ring.close()


def test_counts_above_two_to_the_32_reach_the_high_counter_word():
    case = Case("arena_stress")
    E = 40
    py, npz = cd.seeds(E)
    vec = _vec(E, case.kwargs)
    cfg = cd.counter_config(case.kwargs)
    e_ = np.arange(E, dtype=np.int64)
    # just below, at and far above 2**32 words (block index 2**30: the low counter word wraps into the high one during the run)
    far = np.stack([(1 << 32) - 40 + 3 * e_, (1 << 32) - 70 + 5 * e_], axis=1)
    far[E // 2:] += (1 << 45) + 1
    vec.set_rng_counters(torch.from_numpy(far).to(vec.device))
    refs = [oracle.OracleEnv(cfg) for _ in range(E)]
    for e, r in enumerate(refs):
        r.seed(int(py[e]), int(npz[e]))
        r.set_rng_counters(int(far[e, 0]), int(far[e, 1]))
    acts = torch.empty((E, case.n), dtype=torch.int8, device=vec.device)
    for t in range(12):
        vec.random_actions(acts, seed=0xFA5, step=t)
        vec.step(acts, want_f64=True)
        a, r64, ctr = acts.cpu().numpy(), vec.rewards64.cpu().numpy(), vec.get_rng_counters().cpu().numpy()
        for e, r in enumerate(refs):
            rw, _, status = r.step(a[e])
            assert status == 0 and np.array_equal(r64[e], rw), f"env {e} step {t}"
            assert tuple(int(x) for x in ctr[e]) == r.get_rng_counters(), f"env {e} step {t}: words consumed"
    for e in range(0, E, 3):
        _state_equal(view_arrays(vec.get_state(e), case.n, case.g), view_arrays(refs[e].get_state(), case.n, case.g), f"env {e}")
    assert vec.status() == 0
    vec.close()


# ---- 6. snapshot records ---------------------------------------------------------------------------------------------------------------------
def _up(x, a):
    return (x + a - 1) // a * a


def test_snapshot_records_carry_32_bytes_of_rng_and_continue_bit_for_bit():
    case = Case("arena_random")
    E = 48
    seeds = cd.seeds(E)
    a, b, ring = _vec(E, case.kwargs), _vec(E, case.kwargs, seeds=(seeds[0] + np.uint64(5), seeds[1])), _vec(4, case.kwargs, "counter")
    acts = torch.empty((E, case.n), dtype=torch.int8, device=a.device)
    _run(a, acts, 0, 25)
    recs = a.save_states()
    ref_ctr_at_save = a.get_rng_counters().cpu().numpy()
    ref = _run(a, acts, 25, 25)
    # into other slots of the same handle (reversed), and into another handle whose own seeds differ
    perm = torch.arange(E - 1, -1, -1, device=a.device)
    a.load_states(recs, perm)
    acts_rev = torch.empty_like(acts)
    rows = []
    for t in range(25, 50):
        a.random_actions(acts, seed=0xABC, step=t)
        acts_rev.copy_(acts.flip(0))
        a.step(acts_rev, auto_reset=True, want_f64=True)
        rows.append(torch.cat([a.rewards64.flip(0).contiguous().view(torch.int64).flatten(), a.rewards.flip(0).contiguous().view(torch.int32).flatten().long(),
                               a.done.flip(0).flatten().long()]))
    assert torch.equal(torch.stack(rows), ref[0]), "continuation in other slots"
    assert torch.equal(a.get_rng_counters().flip(0), ref[1])
    b.load_states(recs)
    _same_run(_run(b, acts, 25, 25), ref, "continuation in another handle")
    # the record: the mode-1 record minus its ring, digest and ring-position segments, with rngctr 32 bytes in place of 48
    shared = _record_bytes(a) - 32
    assert shared == _record_bytes(ring) - RING_SEGMENTS - 48, "the segments the two modes share"
    assert a.snapshot_bytes == _up(64 + shared + 32, 256) and ring.snapshot_bytes == _up(64 + shared + RING_SEGMENTS + 48, 256)
    rec = recs[5].cpu().numpy()
    assert np.array_equal(rec[64 + shared - _tail(a):][:32].view(np.int64)[:2], ref_ctr_at_save[5]), "the RNG segment is rngctr"
    # a mode-1 record is refused and leaves the target env's bytes alone
    before = (a.get_states(), a.get_rng_counters().clone())
    foreign = ring.save_states()[:1, :a.snapshot_bytes].contiguous()
    assert a.fingerprint != ring.fingerprint
    a.load_states(foreign, torch.tensor([3], device=a.device))
    assert a.status() == abi.ST_BAD_SNAPSHOT
    _same_tensors(a.get_states(), before[0], "a refused record")
    assert torch.equal(a.get_rng_counters(), before[1])
    for v in (a, b, ring):
        assert v.status() == 0
        v.close()


RING_SEGMENTS = 2 * 4992 + 1408 + 208 + 736 + 16  # both streams' rings, the three digests, the positions / flags / ages


def _tail(vec):
    """bytes of a record's segments behind its RNG segment: metrics, visitation base maps and log (ctf_snapshot.h)"""
    N, GS = vec.N_AGENTS, _up(vec.GRID_SIZE ** 2, 16)
    return _up(52 * N, 16) + 4 * N * GS + 1024 * N


def _record_bytes(vec):
    """bytes of a record's segments (header and final padding apart), ctf_snapshot.h"""
    N, GS = vec.N_AGENTS, _up(vec.GRID_SIZE ** 2, 16)
    rng = {"counter": RING_SEGMENTS + 48, MODE: 32}[vec.rng_mode]
    return _up(_up(14 * N, 4) + 16, 16) + GS + rng + _tail(vec)


# ---- 7. hipGraph -----------------------------------------------------------------------------------------------------------------------------
def test_a_captured_step_observe_replays_to_the_oracles_results():
    kw = dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii, GAME_STEPS=25)
    E = 16
    py, npz = cd.seeds(E)
    vec = _vec(E, kw)
    cfg = cd.counter_config(kw)
    n, dev = vec.N_AGENTS, vec.device
    table = torch.zeros((E, n), dtype=torch.int8, device=dev)
    vec.obs  # (allocated before the capture)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph, stream=side):  # capture only: nothing runs
        vec.step_observe(table, auto_reset=True, want_f64=True)
    torch.cuda.synchronize(dev)
    refs = [oracle.OracleEnv(cfg) for _ in range(E)]
    for e, r in enumerate(refs):
        r.seed(int(py[e]), int(npz[e]))
    rng = np.random.default_rng(9)
    for rep in range(40):
        acts = rng.integers(0, 9, (E, n)).astype(np.int8)
        table.copy_(torch.from_numpy(acts).to(dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        r64, d, o, m = vec.rewards64.cpu().numpy(), vec.done.cpu().numpy(), vec.obs.cpu().numpy(), vec.meta.cpu().numpy().view(np.uint16)
        for e, r in enumerate(refs):
            if r.get_state().done:
                r.reset()
            rw, dn, status = r.step(acts[e])
            ro, rm = r.observe()
            ctx = f"replay {rep} env {e}"
            assert status == 0 and np.array_equal(r64[e], rw) and int(d[e]) == int(dn), ctx
            assert np.array_equal(o[e], ro) and np.array_equal(m[e], rm.view(np.uint16)), ctx
    ctr = vec.get_rng_counters().cpu().numpy()
    assert all(tuple(int(x) for x in ctr[e]) == refs[e].get_rng_counters() for e in range(E))
    assert vec.status() == 0
    vec.close()


# ---- 8. what refuses, refuses ------------------------------------------------------------------------------------------------------------------
def test_the_mt_state_entry_points_refuse_and_step_observe_stays_two_launches(monkeypatch):
    monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", "1")
    case = Case("arena_random")
    vec, ring = _vec(64, case.kwargs), _vec(64, case.kwargs, "counter")
    vec.obs, ring.obs
    assert ring.observe_kernel() == "k_observe_tiles" and ring.step_observe_launches() == 1  # the switch is on, and mode 1 takes it
    assert vec.observe_kernel() == "k_observe_tiles" and vec.step_observe_launches() == 2
    state = np.zeros(625, np.uint32)
    dev_states = torch.zeros((64, 625), dtype=torch.int32, device=vec.device)
    for call in (lambda: vec.get_rng_state(0), lambda: vec.set_rng_state(0, state, state), lambda: vec.get_rng_states(),
                 lambda: vec.set_rng_states(dev_states, dev_states)):
        with pytest.raises(abi.CtfLibraryError, match="counter-direct"):
            call()
    one = pkg.VecGridworldCtf(1, device=0, py_seeds=[5], np_seeds=[6], rng_mode=MODE, tune_placement=False, **case.kwargs)
    with pytest.raises(abi.CtfLibraryError, match="counter-direct"):
        one.host_step(np.zeros(case.n, np.int8), rng_out=True)
    # ... and ctf_host_step without generator states simply works: one step against the oracle
    ref = oracle.OracleEnv(cd.counter_config(case.kwargs))
    ref.seed(5, 6)
    a = np.array([t % 9 for t in range(case.n)], np.int8)
    rewards, done, status, view, _, _ = one.host_step(a)
    rw, dn, _ = ref.step(a)
    assert status == 0 and np.array_equal(rewards, rw) and done == dn
    _state_equal(view_arrays(view, case.n, case.g), view_arrays(ref.get_state(), case.n, case.g), "host_step")
    mt = _vec(2, case.kwargs, "mt19937", seeds=([1, 2], [1, 2]))
    with pytest.raises(abi.CtfLibraryError, match="MT19937"):
        mt.get_rng_counters()  # (the error names the handle's actual mode)
    for v in (vec, ring, one, mt):
        assert v.status() == 0
        v.close()


# ---- 9. memory ---------------------------------------------------------------------------------------------------------------------------------
def test_a_handle_is_12000_bytes_per_env_smaller_than_a_counter_handle():
    case = Case("arena_random")
    E = 4096
    used = {}
    for mode in ("counter", MODE):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free0 = torch.cuda.mem_get_info(0)[0]
        vec = _vec(E, case.kwargs, mode, log_metrics=False)
        torch.cuda.synchronize()
        used[mode] = free0 - torch.cuda.mem_get_info(0)[0]
        assert vec.status() == 0
        vec.close()
        del vec
    assert used["counter"] - used[MODE] >= 12000 * E, used

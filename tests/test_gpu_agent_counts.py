"""The env path at every agent count, 2 to 16 (tests/_agent_counts.py: 29 configurations, even and lopsided teams, grid sizes whose
16-byte pads differ): the step and both renders, the snapshot kernels, the two harvests and the bulk state export / import, each
against one CPU oracle env per device env.  What the sweep pins beyond the fixed-shape tests: the snapshot's word path of the
counters segment (N no multiple of 4) and every row width of its visitation-log column (N = 16; 4, 12; 2, 6, 10, 14; odd N), decoded
on the host from the documented record layout and moved between two handles at different index lists; k_harvest_1 .. 4 with ragged
last waves, group changes inside a batch and the hand-over from batches of eight to single envs; odd N above 8 and opponent lists of
different lengths in the step, the renders and the forced lane widths.  77 envs: 2 * 32 + 13 = 64 + 13.  An env is dropped only
where the oracle itself reports a non-zero status (no respawn cell); tests/test_agent_counts_cpu.py asserts with the oracle alone
that this leaves every run enough envs, episode ends, captures and non-zero last counter words.  Every comparison is exact."""
import numpy as np
import pytest

import oracle
import _agent_counts as ac
from _cases import abi, cfgmod, pkg, view_arrays
from test_gpu_harvest import _row
from test_gpu_snapshot import _layout
from test_gpu_states import EXPORTED, _assert_record_is_view, _bits, _host
from test_gpu_visitation import Tracked, _i64

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

IDS = [ac.config_id(c) for c in ac.CONFIGS]
E = ac.E
OTHER_SEED = 77         # action stream of the second handle before it takes the first one's envs
POISON = 0x5A5A5A5A5A5A5A5A
VIEW_FIELDS = ("grid", "pos", "has_flag", "inv", "perm", "metrics", "visitation", "step_count", "done", "team_captures")


def _make(config, seeds, log_metrics=True, rng_mode="mt19937"):
    return pkg.VecGridworldCtf(len(seeds), device=0, py_seeds=seeds, np_seeds=seeds, log_metrics=log_metrics, tune_placement=False,
                               rng_mode=rng_mode, **ac.config_kwargs(*config))


def _other_seeds():
    return np.arange(E, dtype=np.uint64) * 7919 + 11


def _acts(vec):
    return torch.empty((vec.n_envs, vec.N_AGENTS), dtype=torch.int8, device=vec.device)


class Follower(Tracked):
    """Tracked (one oracle env and the test's own true visit counts) for auto-reset runs in which the oracle may drop the env."""

    def __init__(self, cfg, seed):
        super().__init__(cfg, seed)
        self.alive = True

    def step(self, actions):
        """one auto-reset step -> (rewards, done), or None once the oracle has reported a non-zero status"""
        if not self.alive:
            return None
        if self.done():
            self.reset()
        rewards, done, status = self.env.step(actions)
        if status:
            self.alive = False
            return None
        self._mark()
        return rewards, done

    def arrays(self):
        return view_arrays(self.env.get_state(), self.n, self.g)

    def cells(self):
        """every agent's cell as the visitation log has it: row * G + column"""
        v = self.env.get_state()
        return [int(v.pos[i][0]) * self.g + int(v.pos[i][1]) for i in range(self.n)]


def _followers(cfg, seeds):
    return [Follower(cfg, s) for s in seeds]


def _alive(followers):
    return np.array([f.alive for f in followers], bool)


def _same_view(got, want, ctx):
    for k in VIEW_FIELDS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), f"{ctx}: {k}"
    assert np.array_equal(_bits(got["hp"]), _bits(want["hp"])), f"{ctx}: hp"


def _check_outputs(vec, e_dev, follower, out, reverse_mask, host, ctx):
    """the outputs of device env e_dev (host copies: rewards64, done, obs, meta) against what the follower's step returned"""
    r64, d, o, m = host
    rewards, done = out
    assert np.array_equal(_bits(r64[e_dev]), _bits(rewards)) and int(d[e_dev]) == int(done), ctx
    ro, rm = follower.env.observe() if reverse_mask is None else follower.env.observe(reverse_mask=reverse_mask)
    assert np.array_equal(o[e_dev], ro), ctx + ": observations"
    assert np.array_equal(m[e_dev], rm.view(np.uint16)), ctx + ": metadata"


def _host_outputs(vec):
    return vec.rewards64.cpu().numpy(), vec.done.cpu().numpy(), vec.obs.cpu().numpy(), vec.meta.cpu().numpy().view(np.uint16)


def _status_ok(vec, followers, ctx=""):
    """no status bit but CTF_ST_NO_RESPAWN, and that one only where the oracle has dropped an env for it: at most a quarter of them"""
    dropped = int((~_alive(followers)).sum())
    assert 4 * dropped <= len(followers), (ctx, dropped)
    st = vec.status()
    assert st & ~abi.ST_NO_RESPAWN == 0 and (dropped or st == 0), (ctx, st)


# ---- (a) the step, the render, the compact render --------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ac.CONFIGS, ids=IDS)
def test_step_and_both_renders_match_the_oracle(config):
    """70 step_observe(auto_reset, want_f64) calls: every step f64 rewards, done, all observations and metadata rows; every fifth
    step the compact render; every 16th step a reversal mask other than the default; at the end the full state views and both
    generators' states of every env still followed."""
    n = config[0]
    seeds = ac.seeds()
    vec = _make(config, seeds)
    g = vec.GRID_SIZE
    followers = _followers(vec.cfg, seeds)
    acts = _acts(vec)
    every = (1 << n) - 1
    masks = {0: 0, 16: every, 32: 0x9A65 & every, 48: 0x65A6 & every, 64: 1}
    for t in range(ac.STEPS):
        vec.random_actions(acts, seed=ac.ACT_SEED, step=t)
        mask = masks.get(t)
        _, _, obs, meta = vec.step_observe(acts, auto_reset=True, want_f64=True, reverse_mask=mask)
        host = _host_outputs(vec)
        if t % 5 == 0:
            meta_planes = meta.clone()  # (observe_codes writes the same metadata buffer)
            codes, meta_c = vec.observe_codes(reverse_mask=mask)
            assert torch.equal(pkg.expand_codes(codes, vec.N_CHANNELS), obs) and torch.equal(meta_c.view(torch.int16), meta_planes.view(torch.int16)), t
        a = acts.cpu().numpy()
        for e, f in enumerate(followers):
            out = f.step(a[e])
            if out is not None:
                _check_outputs(vec, e, f, out, mask, host, f"{ac.config_id(config)} env {e} step {t}")
    alive = _alive(followers)
    py, npw = (x.cpu().numpy().view(np.uint32) for x in vec.get_rng_states())
    for e in np.flatnonzero(alive):
        ctx = f"{ac.config_id(config)} env {e} final"
        _same_view(view_arrays(vec.get_state(int(e)), n, g), followers[e].arrays(), ctx)
        rpy, rnp = followers[e].env.get_rng_state()
        assert np.array_equal(py[e], rpy) and np.array_equal(npw[e], rnp), ctx + ": generators"
    _status_ok(vec, followers)
    vec.close()


class _SweepCase:
    """what test_gpu_parity._lane_width_against_oracle reads of a golden Case, for a config of the sweep"""

    def __init__(self, config):
        self.kwargs = ac.config_kwargs(*config)
        self.n, self.g = config[0], ac.grid_size(*config)

    def config(self, log_metrics=True):
        return cfgmod.build_config(self.kwargs, log_metrics=log_metrics)


@pytest.mark.parametrize("lanes", [1, 2, 4])
@pytest.mark.parametrize("config", ac.LANE_CONFIGS, ids=[ac.config_id(c) for c in ac.LANE_CONFIGS])
def test_forced_lane_widths_at_odd_and_lopsided_counts(config, lanes, monkeypatch):
    """The lopsided configs of ten agents and more (opponent lists of different lengths, agents in no list) and 9-, 13- and 15-even
    under CTF_STEP_W = 1, 2, 4: the step alone, by the helper of test_every_step_lane_width_matches_the_oracle."""
    import test_gpu_parity as parity

    monkeypatch.setattr(parity, "Case", _SweepCase)
    parity._lane_width_against_oracle(config, lanes, ac.LANE_E, ac.LANE_STEPS, True, monkeypatch)


# ---- (b) the snapshot ----------------------------------------------------------------------------------------------------------------
def _segments(vec):
    """record segments restated from ctf_snapshot.h: name -> (offset, bytes in use); -> (segments, end of the last one)"""
    N, G = vec.N_AGENTS, vec.GRID_SIZE
    up = lambda x, a=16: (x + a - 1) // a * a
    GS, RS = up(G * G), up(up(14 * N, 4) + 16)
    segs = [("rec", RS), ("grid", GS), ("mt_py", 2 * 624 * 4), ("mt_np", 2 * 624 * 4), ("py_top", 2 * 176 * 4), ("np_hit", 2 * 26 * 4),
            ("np_nib", 2 * 92 * 4), ("rng", 16)]
    if vec.rng_mode == "counter":
        segs.append(("ctr", 6 * 8))
    if vec.cfg.log_metrics:
        segs += [("metrics", 13 * N * 4), ("vis", 4 * N * GS), ("vislog", 512 * N * 2)]
    out, off = {}, 64
    for name, size in segs:
        out[name] = (off, size)
        off += up(size)
    assert up(off, 256) == vec.snapshot_bytes
    if vec.cfg.log_metrics:
        assert {k: v[0] for k, v in out.items()} == {k: v[0] for k, v in _layout(vec).items()}
    return out, off


def _check_records(recs, src, vec, followers, log, handed, ctx):
    """Records ``recs`` (host, uint8 [n, S]) saved from envs ``src`` of ``vec``, decoded from the documented layout."""
    n_rec, S = recs.shape
    N, G = vec.N_AGENTS, vec.GRID_SIZE
    GG, GS = G * G, (G * G + 15) // 16 * 16
    segs, end = _segments(vec)
    assert S % 256 == 0 and S == vec.snapshot_bytes
    head = recs[:, :64].copy().view(np.uint32)
    fp = vec.fingerprint
    want_head = np.zeros(16, np.uint32)
    want_head[:6] = [0x53465443, 1, fp & 0xFFFFFFFF, (fp >> 32) & 0xFFFFFFFF, S, N]
    assert np.array_equal(head, np.broadcast_to(want_head, head.shape)), ctx + ": header"
    assert not recs[:, end:].any(), ctx + ": bytes after the last segment"

    def seg(name, dtype, lo=0, count=None):
        o, size = segs[name]
        hi = size if count is None else lo + count * np.dtype(dtype).itemsize
        return recs[:, o + lo:o + hi].copy().view(dtype)

    states = _host(vec.get_states(src.tolist()))
    off_misc = (14 * N + 3) // 4 * 4
    assert np.array_equal(seg("rec", np.uint64, 0, N), _bits(states["hp"])), ctx + ": hp"
    assert np.array_equal(seg("rec", np.int8, 8 * N, 2 * N).reshape(n_rec, N, 2), states["pos"]), ctx + ": pos"
    assert np.array_equal(seg("rec", np.uint8, 10 * N, N), states["has_flag"]), ctx + ": has_flag"
    assert np.array_equal(seg("rec", np.uint8, 11 * N, N), states["perm"]), ctx + ": perm"
    assert np.array_equal(seg("rec", np.int16, 12 * N, N).astype(np.int32), states["inventory"]), ctx + ": inventory"
    misc = seg("rec", np.int32, off_misc, 4)
    assert np.array_equal(misc[:, 0], states["step_count"]) and np.array_equal(misc[:, 1:3], states["team_captures"]), ctx + ": step / captures"
    assert np.array_equal(misc[:, 3] & 1, states["done"]), ctx + ": done"
    grid = seg("grid", np.uint8)
    assert np.array_equal(grid[:, :GG].reshape(n_rec, G, G), states["grid"]) and not grid[:, GG:].any(), ctx + ": grid"
    rng = seg("rng", np.uint32)
    assert not rng[:, 3].any()
    if vec.rng_mode == "mt19937":
        py, npw = (x.cpu().numpy().view(np.uint32) for x in vec.get_rng_states())
        assert np.array_equal(rng[:, 0] & 0xFFFF, py[src, 624]) and np.array_equal(rng[:, 1] & 0xFFFF, npw[src, 624]), ctx + ": generator positions"
    met, caps, steps = (x.cpu().numpy() for x in vec.counters())
    assert np.array_equal(misc[:, 0], steps[src]) and np.array_equal(misc[:, 1:3], caps[src])
    if not vec.cfg.log_metrics:
        return
    o, size = segs["metrics"]
    assert np.array_equal(seg("metrics", np.int32).reshape(n_rec, 13, N), met[src]), ctx + ": counters"
    assert not recs[:, o + size:segs["vis"][0]].any(), ctx + ": the pad of the counters"
    vis = seg("vis", np.uint32).reshape(n_rec, N, GS)
    rows = seg("vislog", np.uint16).reshape(n_rec, 512, N)
    for k, e in enumerate(src):
        if e in handed:  # base maps handed in with set_states: the segment carries them, pads zero
            assert np.array_equal(vis[k, :, :GG], handed[e].reshape(N, GG)) and not vis[k, :, GG:].any(), f"{ctx}: base maps of env {e}"
        if followers[e].alive:  # the log since the env's last reset: row (t & 511) = the cells after step t
            for t in range(1, len(log) + 1):
                assert np.array_equal(rows[k, t & 511], log[t - 1][e]), f"{ctx}: visitation log of env {e}, step {t}"


def _snapshot(config, rng_mode, log_metrics):
    n = config[0]
    name = f"{ac.config_id(config)} {rng_mode}" + ("" if log_metrics else " bare")
    seeds, seeds_b = ac.seeds(), _other_seeds()
    A, B, twin = (_make(config, s, log_metrics, rng_mode) for s in (seeds, seeds_b, seeds_b))
    g, dev = A.GRID_SIZE, A.device
    assert A.fingerprint == B.fingerprint and A.snapshot_bytes == B.snapshot_bytes
    # a handle does not clear, when it is created, the storage that nothing has written yet (log slots of steps not yet made, base
    # maps that are implicitly zero): B starts from the twin's bytes, so that whole records of the two can be compared at the end
    B.load_states(twin.save_states())
    followers = _followers(A.cfg, seeds)
    xa, xb = _acts(A), _acts(B)
    rng = np.random.default_rng(1000 * n + config[1])
    log, handed = [], {}

    def step_a(t):
        A.random_actions(xa, seed=ac.ACT_SEED, step=t)
        A.step_observe(xa, auto_reset=True, want_f64=True)
        a = xa.cpu().numpy()
        return [f.step(a[e]) for e, f in enumerate(followers)]

    for t in range(25):
        step_a(t)
        log.append(np.array([f.cells() for f in followers], np.uint16))
        if t == 9 and log_metrics:  # non-trivial base maps for the even-numbered envs: CTF_F_BASE_ZERO goes, the vis segment carries data
            even = [e for e in range(0, E, 2) if followers[e].alive]
            st = A.get_states(even)
            maps = rng.integers(0, 256, (len(even), n, g, g)).astype(np.uint8)
            maps[:, :, ::3, 1] = 0
            st["visitation"] = torch.from_numpy(maps).to(dev)
            A.set_states(st, idx=even)
            for k, e in enumerate(even):
                view = followers[e].env.get_state()
                for i in range(n):
                    np.frombuffer(view.visitation[i], np.uint8)[:g * g] = maps[k, i].reshape(-1)
                followers[e].env.set_state(view)
                followers[e].counts[:] = maps[k]
                handed[e] = maps[k]
    for t in range(7):
        B.random_actions(xb, seed=OTHER_SEED, step=t)
        B.step_observe(xb, auto_reset=True, want_f64=True)
        twin.step_observe(xb, auto_reset=True, want_f64=True)
    assert not log_metrics or bool(A.counters()[0].any())
    saved = {}
    for count in (1, 63, 65, 77):
        src = rng.permutation(E)[:count]
        saved[count] = (src, A.save_states(torch.from_numpy(src).to(dev)))
        _check_records(saved[count][1].cpu().numpy(), src, A, followers, log, handed, f"{name}, {count} records")
    src, recs = saved[65]
    dst = rng.permutation(E)[:65]
    assert not np.array_equal(dst, src) and not np.array_equal(dst, np.arange(65))
    B.load_states(recs, torch.from_numpy(dst).to(dev))
    B.observe()
    src_d, dst_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    ends = 0
    for t in range(25, ac.STEPS):
        B.random_actions(xb, seed=OTHER_SEED, step=t)
        outs = step_a(t)  # (fills xa)
        xb[dst_d] = xa[src_d]
        B.step_observe(xb, auto_reset=True, want_f64=True)
        twin.step_observe(xb, auto_reset=True, want_f64=True)
        host = _host_outputs(B)
        for k in range(65):
            if outs[src[k]] is not None:
                _check_outputs(B, dst[k], followers[src[k]], outs[src[k]], None, host, f"{name} step {t}: env {dst[k]} loaded from {src[k]}")
                ends += int(outs[src[k]][1])
    assert ends > 0, "the run crosses no episode end"
    met, caps, steps = (x.cpu().numpy() for x in B.counters())
    if rng_mode == "mt19937":
        py, npw = (x.cpu().numpy().view(np.uint32) for x in B.get_rng_states())
    else:
        ctr = B.get_rng_counters().cpu().numpy()
    vis = _i64(B.visitation()).cpu().numpy() if log_metrics else None
    for k in range(65):
        f, e = followers[src[k]], int(dst[k])
        if not f.alive:
            continue
        ctx = f"{name} final: env {e} loaded from {src[k]}"
        want = f.arrays()
        _same_view(view_arrays(B.get_state(e), n, g), want, ctx)
        if rng_mode == "mt19937":
            rpy, rnp = f.env.get_rng_state()
            assert np.array_equal(py[e], rpy) and np.array_equal(npw[e], rnp), ctx + ": generators"
        else:
            assert tuple(int(x) for x in ctr[e]) == f.env.get_rng_counters(), ctx + ": words consumed"
        assert int(steps[e]) == want["step_count"] and caps[e].tolist() == want["team_captures"], ctx + ": counters()"
        if log_metrics:
            assert np.array_equal(met[e], want["metrics"]), ctx + ": counters()"
            assert np.array_equal(vis[e], f.checked()), ctx + ": visitation()"
    rest = torch.from_numpy(np.setdiff1d(np.arange(E), dst)).to(dev)
    assert rest.numel() == E - 65 and torch.equal(B.save_states()[rest], twin.save_states()[rest]), f"{name}: an env that was not listed changed"
    _status_ok(A, followers, name)
    for v in (B, twin):
        assert v.status() & ~abi.ST_NO_RESPAWN == 0
        v.close()
    A.close()


@pytest.mark.parametrize("config", ac.CONFIGS, ids=IDS)
def test_snapshot_records_decode_and_move_between_handles(config):
    """Handle A runs 25 steps (the oracle follows; at step 10 the even-numbered envs are given base maps); 1, 63, 65 and 77 records
    are saved at shuffled index lists and decoded on the host: header, S, the rec and grid segments against get_states, the
    generators' positions, the counters segment against counters() with its pad, the handed-in base maps, every row of the
    visitation log since the last reset against the oracle's positions, the zero tail.  The 65 records go into handle B (other
    seeds, 7 steps of another action stream) at another shuffled list; for 45 steps, across two episode ends, B's loaded envs give
    the oracle's rewards, done, observations and metadata of the env they came from, at the end its state view, generators,
    counters() and visitation(); B's other envs stay bit-identical to a twin that never loaded a record of A."""
    _snapshot(config, "mt19937", True)


@pytest.mark.parametrize("config", [c for c in ac.CONFIGS if c[0] in ac.COUNTER_N], ids=lambda c: ac.config_id(c))
def test_snapshot_in_counter_mode(config):
    _snapshot(config, "counter", True)


@pytest.mark.parametrize("config", [c for c in ac.CONFIGS if c[0] in ac.BARE_N], ids=lambda c: ac.config_id(c))
def test_snapshot_without_metrics(config):
    _snapshot(config, "mt19937", False)


# ---- (c) the episode harvest ---------------------------------------------------------------------------------------------------------
def _guarded(shape, dev):
    """a zeroed table with one extra row on either side of it, filled with a pattern -> (whole allocation, the table)"""
    big = torch.full((shape[0] + 2,) + tuple(shape[1:]), POISON, dtype=torch.int64, device=dev)
    table = big[1:-1]
    table.zero_()
    return big, table


def _guards_kept(big):
    return bool((big[0] == POISON).all()) and bool((big[-1] == POISON).all())


@pytest.mark.parametrize("config", ac.CONFIGS, ids=IDS)
def test_harvests_of_a_staggered_run_equal_the_oracle(config):
    """77 envs staggered as bench.stagger_phases does it, 5 groups by a fixed permutation, 70 step(auto_reset) calls with both
    harvests after every step.  Expected: the oracle envs' rows and the tracked visit counts read just before they reset.  The
    kernel is k_harvest_NR, NR = ceil(13 N / 64) counter words per lane: 1 up to N = 4, 2 up to 9, 3 up to 14, 4 at 15 and 16 (there
    and at N = 10 the last round is partial)."""
    import bench

    n = config[0]
    seeds, G = ac.seeds(), 5
    vec = _make(config, seeds)
    g, gs, dev = vec.GRID_SIZE, int(vec.cfg.game_steps), vec.device
    followers = _followers(vec.cfg, seeds)
    groups_h = np.random.default_rng(1).permutation(E) % G
    groups = torch.from_numpy(groups_h.astype(np.int32)).to(dev)
    bench.stagger_phases(vec, torch, 0, gs)
    for s in range(gs):  # the same steps and resets on the CPU
        for e, f in enumerate(followers):
            f.step(oracle.philox_actions(n, ac.STAGGER_SEED, s, e))
            if e % gs == s and f.alive:
                f.reset()
    acts = _acts(vec)
    big, acc = _guarded((G, vec.harvest_words), dev)
    big_v, table = _guarded((G, n, g, g), dev)
    want, want_v = np.zeros((G, vec.harvest_words), np.int64), np.zeros((G, n, g, g), np.int64)
    alive = _alive(followers)
    mask = torch.from_numpy(alive.astype(np.uint8)).to(dev)
    for t in range(ac.STEPS):
        vec.random_actions(acts, seed=ac.ACT_SEED, step=t)
        vec.step(acts, auto_reset=True)
        for e, f in enumerate(followers):
            out = f.step(oracle.philox_actions(n, ac.ACT_SEED, t, e))
            if out is not None and out[1]:
                v = f.env.get_state()
                assert v.step_count == gs
                want[groups_h[e]] += _row(v, n, g)
                want_v[groups_h[e]] += f.checked()
        if not np.array_equal(alive, _alive(followers)):
            alive = _alive(followers)
            mask = torch.from_numpy(alive.astype(np.uint8)).to(dev)
        vec.harvest(acc, groups, mask=mask)
        vec.harvest_visitation(table, groups, mask=mask)
    assert (want[:, 0] >= 2).all() and want[:, 8:].any()
    assert torch.equal(acc.cpu(), torch.from_numpy(want)), "the episode table"
    assert torch.equal(table.cpu(), torch.from_numpy(want_v)), "the visitation table"
    assert _guards_kept(big) and _guards_kept(big_v)
    _status_ok(vec, followers)
    vec.close()


def _lockstep(config, log_metrics):
    n = config[0]
    seeds = ac.seeds()
    vec = _make(config, seeds, log_metrics=log_metrics)
    g, gs, dev, H = vec.GRID_SIZE, int(vec.cfg.game_steps), vec.device, vec.harvest_words
    followers = _followers(vec.cfg, seeds)
    acts = _acts(vec)
    env = np.arange(E)
    runs, thirds = env // 16, env % 3
    for t in range(gs):
        if t == gs - 1:  # nothing has ended yet
            _, acc = _guarded((5, H), dev)
            vec.harvest(acc, torch.from_numpy(runs.astype(np.int32)).to(dev))
            assert not bool(acc.any()), "an episode was harvested before its last step"
        vec.random_actions(acts, seed=ac.ACT_SEED, step=t)
        vec.step(acts, auto_reset=True)
        for e, f in enumerate(followers):
            f.step(oracle.philox_actions(n, ac.ACT_SEED, t, e))
    alive = _alive(followers)
    rows = {e: _row(followers[e].env.get_state(), n, g) for e in np.flatnonzero(alive)}
    counts = {e: followers[e].checked() for e in np.flatnonzero(alive)} if log_metrics else {}
    assert all(int(r[0]) == 1 and int(r[6]) == gs for r in rows.values())
    picked = ac.lockstep_mask(alive)
    assert int(picked[:32].sum()) == 7 and int(picked[32:64].sum()) == 9
    for what, groups_h, mask_h in (("runs of 16", runs, alive), ("e % 3", thirds, alive), ("7 and 9 of a wave", runs, picked)):
        G = int(groups_h.max()) + 1
        groups = torch.from_numpy(groups_h.astype(np.int32)).to(dev)
        mask = torch.from_numpy(np.asarray(mask_h).astype(np.uint8)).to(dev)
        taken = [e for e in env if mask_h[e]]
        big, acc = _guarded((G, H), dev)
        vec.harvest(acc, groups, mask=mask)
        want = np.zeros((G, H), np.int64)
        for e in taken:
            want[groups_h[e]] += rows[e]
        if not log_metrics:
            assert not want[:, 8:].any()
        assert int(want[:, 0].sum()) == len(taken) and torch.equal(acc.cpu(), torch.from_numpy(want)), f"{what}: the episode table"
        assert _guards_kept(big), what
        if log_metrics:
            big_v, table = _guarded((G, n, g, g), dev)
            vec.harvest_visitation(table, groups, mask=mask)
            want_v = np.zeros((G, n, g, g), np.int64)
            for e in taken:
                want_v[groups_h[e]] += counts[e]
            assert torch.equal(table.cpu(), torch.from_numpy(want_v)), f"{what}: the visitation table"
            assert _guards_kept(big_v), what
    _status_ok(vec, followers)
    vec.close()


@pytest.mark.parametrize("config", ac.CONFIGS, ids=IDS)
def test_harvests_of_a_lockstep_batch_under_three_group_assignments(config):
    """Every env still followed ends in step GAME_STEPS.  Groups in runs of 16 (the id changes inside a batch of eight), e % 3 (at
    every env), and a mask that leaves exactly 7 taken envs in the first wave and 9 in the second: no batch of eight in one, one
    batch and then a single env in the other.  Expected: the integer sums of the oracle's rows and of the tracked visit counts;
    the rows either side of each table keep their pattern."""
    _lockstep(config, True)


@pytest.mark.parametrize("config", [(16, 0), (16, 1)], ids=lambda c: ac.config_id(c))
def test_harvest_of_a_lockstep_batch_without_metrics(config):
    """k_harvest_0 at N = 16: the seven scalars, the counter words untouched."""
    _lockstep(config, False)


# ---- (d) export and import of states as plain arrays ----------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ac.CONFIGS, ids=IDS)
def test_states_export_and_import_at_every_count(config):
    """After 25 steps every exported field of every env followed equals the oracle's view (hp as bits), visitation() its maps; the
    batch, imported into a fresh handle with the generators' states, runs 20 steps on with the oracle's results."""
    n = config[0]
    seeds = ac.seeds()
    x, y = _make(config, seeds), _make(config, _other_seeds())
    g, dev = x.GRID_SIZE, x.device
    followers = _followers(x.cfg, seeds)
    acts = _acts(x)
    for t in range(25):
        x.random_actions(acts, seed=ac.ACT_SEED, step=t)
        x.step(acts, auto_reset=True)
        a = acts.cpu().numpy()
        for e, f in enumerate(followers):
            f.step(a[e])
    for t in range(3):  # (the fresh handle is somewhere else)
        y.random_actions(acts, seed=OTHER_SEED, step=t)
        y.step(acts, auto_reset=True)
    states = x.get_states()
    assert sorted(states) == sorted(EXPORTED)
    host, vis = _host(states), x.visitation()
    counts = _i64(vis).cpu().numpy()
    kept = np.flatnonzero(_alive(followers))
    for e in kept:
        _assert_record_is_view(host, e, followers[e].arrays(), EXPORTED, ac.config_id(config))
        assert np.array_equal(counts[e], followers[e].checked()), e
    idx = torch.from_numpy(kept).to(dev)
    states["visitation"] = (vis.view(torch.int32) & 0xFF).to(torch.uint8)
    if len(kept) == E:
        y.set_states(states)
    else:  # an env the oracle has dropped is in no defined state: the others
        y.set_states({f: t[idx].contiguous() for f, t in states.items()}, idx=idx)
    py, npw = x.get_rng_states()
    py_y, npw_y = y.get_rng_states()
    py_y[idx], npw_y[idx] = py[idx], npw[idx]
    y.set_rng_states(py_y, npw_y)
    y.observe()
    for t in range(25, 45):
        y.random_actions(acts, seed=ac.ACT_SEED, step=t)
        y.step_observe(acts, auto_reset=True, want_f64=True)
        host_out, a = _host_outputs(y), acts.cpu().numpy()
        for e in kept:
            out = followers[e].step(a[e])
            if out is not None:
                _check_outputs(y, e, followers[e], out, None, host_out, f"{ac.config_id(config)} env {e} step {t}")
    counts = _i64(y.visitation()).cpu().numpy()
    for e in kept:
        if followers[e].alive:
            _same_view(view_arrays(y.get_state(int(e)), n, g), followers[e].arrays(), f"{ac.config_id(config)} env {e} final")
            assert np.array_equal(counts[e], followers[e].checked()), e
    _status_ok(x, followers)
    assert y.status() & ~abi.ST_NO_RESPAWN == 0
    x.close(), y.close()


# ---- (f) the step in rng_mode="counter_direct" ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ac.CONFIGS, ids=IDS)
def test_counter_direct_step_at_every_count(config):
    """The Philox tape drawn inside the step kernel, whose windows are sized from N and the number of tagging pairs and whose blocks
    are spread over the env's lanes: 40 auto-reset steps against counter-mode oracles (the same tape, their own float64 compare at
    TAG_PROBABILITY 0.75): every step f64 rewards, done and the words consumed from both tapes, every tenth step and at the end the
    full state views.  From 9-even / 12-lop upwards a step draws more np.random words than the window holds: the compares past it
    are computed where the draw stands."""
    n = config[0]
    seeds = ac.seeds()
    vec = _make(config, seeds, rng_mode="counter_direct")
    g = vec.GRID_SIZE
    followers = _followers(ac.build(*config, counter=True), seeds)
    for t in range(ac.DIRECT_STEPS):
        a = np.stack([oracle.philox_actions(n, ac.ACT_SEED, t, e) for e in range(E)])
        vec.step(torch.from_numpy(a).to(vec.device), auto_reset=True, want_f64=True)
        r64, d, ctr = vec.rewards64.cpu().numpy(), vec.done.cpu().numpy(), vec.get_rng_counters().cpu().numpy()
        full = t % 10 == 9 or t == ac.DIRECT_STEPS - 1
        for e, f in enumerate(followers):
            out = f.step(a[e])
            if out is None:
                continue
            ctx = f"{ac.config_id(config)} env {e} step {t}"
            assert np.array_equal(_bits(r64[e]), _bits(out[0])) and int(d[e]) == int(out[1]), ctx
            assert tuple(int(x) for x in ctr[e]) == f.env.get_rng_counters(), ctx + ": words consumed"
            if full:
                _same_view(view_arrays(vec.get_state(e), n, g), f.arrays(), ctx)
    dropped = int((~_alive(followers)).sum())
    assert dropped <= ac.DIRECT_DROP_CAP, dropped
    _status_ok(vec, followers)
    vec.close()

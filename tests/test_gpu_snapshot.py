"""Batched snapshot, restore and clone of env states (ctf_save_states / ctf_load_states, VecGridworldCtf.save_states /
load_states / clone_envs): a restored env replays bit for bit — observations, metadata, rewards (f32 and f64), done, counters,
generator states and its record — across episode ends, the in-kernel visitation fold and every phase of the generators' rings;
records move between slots, handles and processes of the same fingerprint and are refused (CTF_ST_BAD_SNAPSHOT, env untouched)
otherwise; a restore can be captured into a graph.  Every test runs in both RNG modes on 8_arena."""
import numpy as np
import pytest

import oracle
from _cases import abi, pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MODES = ["mt19937", "counter"]
ACT_SEED = 0x5EED


def _kwargs(name="arena"):
    if name == "split":
        return dict(pkg.configs.SPLIT_KWARGS, SCENARIO=pkg.CtfScenarios.arrow)
    return dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii)


def _make(n_envs, mode, seed_base=11, log_metrics=True, name="arena"):
    seeds = np.arange(n_envs, dtype=np.uint64) * 7919 + seed_base
    return pkg.VecGridworldCtf(n_envs, device=0, py_seeds=seeds, np_seeds=seeds, rng_mode=mode, log_metrics=log_metrics,
                               tune_placement=False, **_kwargs(name))


def _outputs(vec):
    return (vec.obs.clone(), vec.meta.view(torch.int16).clone(), vec.rewards.view(torch.int32).clone(),
            vec.rewards64.view(torch.int64).clone(), vec.done.clone())


def _same(a, b, ctx):
    for x, y, what in zip(a, b, ("observations", "metadata", "rewards f32", "rewards f64", "done")):
        assert torch.equal(x, y), f"{ctx}: {what}"


def _rng(vec):
    return [vec.get_rng_counters()] if vec.rng_mode == "counter" else list(vec.get_rng_states())


def _run(vec, t0, steps, auto_reset=True, record=True, seed=ACT_SEED, acts=None, against=None):
    """step_observe for steps t0 .. t0 + steps - 1 with the synthetic action stream -> the outputs of every step (record), or
    each step's outputs checked against against[t - t0]"""
    if acts is None:
        acts = torch.empty((vec.n_envs, vec.N_AGENTS), dtype=torch.int8, device=vec.device)
    out = []
    for t in range(t0, t0 + steps):
        vec.random_actions(acts, seed=seed, step=t)
        vec.step_observe(acts, auto_reset=auto_reset, want_f64=True)
        if against is not None:
            _same(against[t - t0], _outputs(vec), f"{vec.rng_mode} step {t}")
        elif record:
            out.append(_outputs(vec))
    return out


def _state(vec, sample):
    return [*vec.counters(), *_rng(vec)], [bytes(vec.get_state(e)) for e in sample]


def _same_state(a, b, ctx):
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), f"{ctx}: counters / generator states ({k})"
    assert a[1] == b[1], f"{ctx}: state views"


def _layout(vec):
    """record segments (ctf_snapshot.h): name -> (offset, bytes)"""
    N, G = vec.N_AGENTS, vec.GRID_SIZE
    up = lambda x, a=16: (x + a - 1) // a * a
    GS, RS = up(G * G), up(up(14 * N, 4) + 16)
    segs = [("rec", RS), ("grid", GS), ("mt_py", 4992), ("mt_np", 4992), ("py_top", 1408), ("np_hit", 208), ("np_nib", 736), ("rng", 16)]
    segs += [("ctr", 48)] if vec.rng_mode == "counter" else []
    segs += [("metrics", up(52 * N)), ("vis", 4 * N * GS), ("vislog", 1024 * N)]
    out, off = {}, 64
    for name, size in segs:
        out[name] = (off, size)
        off += size
    assert up(off, 256) == vec.snapshot_bytes
    return out


def _same_records(x, y, vec, ctx):
    """Records equal but for one degree of freedom of the step kernel itself: at full size, two runs of the same envs (twin handles
    stepped alike, no snapshot involved) can differ in whether a stale ring has been regenerated yet (its words, its digests and
    the current ring's mirror of them, the ready flag and age).  Where either record has a regeneration pending for a stream,
    that much of the stream is left out; the positions and the current ring must agree everywhere."""
    L = _layout(vec)
    x, y = x.clone(), y.clone()
    o = L["rng"][0]
    pos_x, pos_y = x[:, o:o + 8].contiguous().view(torch.int32), y[:, o:o + 8].contiguous().view(torch.int32)
    assert torch.equal(pos_x, pos_y), f"{ctx}: generator positions"
    for k, (mt, digests) in enumerate((("mt_py", ("py_top",)), ("mt_np", ("np_hit", "np_nib")))):
        pending = (x[:, o + 8 + k] != 1) | (y[:, o + 8 + k] != 1)
        cur = (pos_x[:, k] >> 16) & 1
        for r in (0, 1):
            rows = pending & (cur == 1 - r)
            m0 = L[mt][0] + r * 2496
            x[rows, m0:m0 + 2496] = 0
            y[rows, m0:m0 + 2496] = 0
            if "ctr" in L:
                c0 = L["ctr"][0] + 16 * k + 8 * r
                x[rows, c0:c0 + 8] = 0
                y[rows, c0:c0 + 8] = 0
        for d in digests:
            d0, dn = L[d]
            x[pending, d0:d0 + dn] = 0
            y[pending, d0:d0 + dn] = 0
        for b in (o + 8 + k, o + 10 + k):
            x[pending, b] = 0
            y[pending, b] = 0
    assert torch.equal(x, y), f"{ctx}: records"


def _roundtrip(n_envs, mode, auto_reset, monkeypatch=None, path=None, before=480, window=40, exact=True):
    vec = _make(n_envs, mode)
    if path is not None:
        monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", path)
        assert vec.step_observe_launches() == (1 if path == "1" else 2)
    sample = sorted({0, 17, n_envs // 3, n_envs - 1})
    _run(vec, 0, before, auto_reset, record=False)
    snap = vec.save_states()
    assert snap.shape == (n_envs, vec.snapshot_bytes) and vec.snapshot_bytes % 256 == 0
    at_save = _state(vec, sample)
    recorded = _run(vec, before, window, auto_reset)
    at_end = _state(vec, sample)
    snap_end = vec.save_states()
    vec.load_states(snap)
    assert torch.equal(vec.save_states(), snap), "the restored state's records"
    _same_state(_state(vec, sample), at_save, "after the restore")
    vec.observe()
    _run(vec, before, window, auto_reset, against=recorded)
    _same_state(_state(vec, sample), at_end, "end of the replay")
    if exact:
        assert torch.equal(vec.save_states(), snap_end), "records at the end of the replay"
    else:
        _same_records(vec.save_states(), snap_end, vec, "end of the replay")
    assert vec.status() == 0
    assert any(bool(r[4].any()) for r in recorded), "the window crosses the episode end"
    del recorded
    vec.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("auto_reset", [True, False])
def test_round_trip_replays_bit_for_bit(mode, auto_reset):
    """4 096 envs with metrics: save at step 480, record 40 steps, restore, replay.  auto_reset: over the episode end at 500;
    without: past the in-kernel visitation fold at step 511."""
    _roundtrip(4096, mode, auto_reset)


def _ring_window(n_envs, mode):
    """the step around which most envs' `random` generator leaves its 624-word block (its position wraps)"""
    vec = _make(n_envs, mode)
    acts = torch.empty((n_envs, vec.N_AGENTS), dtype=torch.int8, device=vec.device)
    prev, wraps = None, []
    for t in range(320):
        _run(vec, t, 1, record=False, acts=acts)
        pos = vec.get_rng_states()[0][:, 624].cpu().numpy()
        if prev is not None:
            wraps.append(((pos < prev).sum(), t))
        prev = pos
    vec.close()
    best = max(w for w in wraps if w[1] >= 60)
    return best[1]


@pytest.mark.parametrize("mode", MODES)
def test_every_ring_phase(mode):
    """64 envs: save after each of 30 consecutive steps, restore every save point and replay 10 steps against the recording.  In
    MT19937 mode the window is placed so that both generators of most envs move to their next ring inside it: save points lie
    on both sides of a ring switch, stale rings (waiting for their regeneration) included."""
    n_envs, n_points, replay = 64, 30, 10
    t0 = _ring_window(n_envs, "mt19937") - n_points // 2
    vec = _make(n_envs, mode)
    acts = torch.empty((n_envs, vec.N_AGENTS), dtype=torch.int8, device=vec.device)
    _run(vec, 0, t0, record=False, acts=acts)
    saves, positions, recorded = [], [], []
    for t in range(t0, t0 + n_points + replay):
        recorded.append(_run(vec, t, 1, acts=acts)[0])
        if t < t0 + n_points:
            saves.append(vec.save_states())
            if mode == "mt19937":
                py, np_ = vec.get_rng_states()
                positions.append(torch.stack([py[:, 624], np_[:, 624]], 1).cpu().numpy())
    if mode == "mt19937":
        pos = np.stack(positions)  # [point, env, generator]
        wrapped = (np.diff(pos, axis=0) < 0).any(axis=0).all(axis=1)
        assert wrapped.sum() > n_envs // 2, f"only {wrapped.sum()} envs switch rings in both generators inside the window"
    for i, snap in enumerate(saves):
        vec.load_states(snap)
        vec.observe()
        for k, out in enumerate(_run(vec, t0 + i + 1, replay, acts=acts)):
            _same(recorded[i + 1 + k], out, f"{mode} save point {t0 + i}, replay step {k}")
    assert vec.status() == 0
    vec.close()


@pytest.mark.parametrize("mode", MODES)
def test_permutation_clone(mode):
    """clone_envs(perm, arange(E)) in place on A; its twin B is not permuted.  A stepped with X[perm] gives B's outputs
    indexed by perm, counters and generator states too."""
    n_envs = 1024
    a, b = _make(n_envs, mode), _make(n_envs, mode)
    _run(a, 0, 50, record=False)
    _run(b, 0, 50, record=False)
    perm = torch.randperm(n_envs, generator=torch.Generator().manual_seed(3)).to(a.device)
    a.clone_envs(perm, torch.arange(n_envs, device=a.device))
    a.observe()
    x = torch.empty((n_envs, a.N_AGENTS), dtype=torch.int8, device=a.device)
    for t in range(50, 90):
        b.random_actions(x, seed=ACT_SEED, step=t)
        b.step_observe(x, auto_reset=True, want_f64=True)
        a.step_observe(x[perm].contiguous(), auto_reset=True, want_f64=True)
        _same(_outputs(a), [o[perm] for o in _outputs(b)], f"{mode} step {t}")
    for p, q in zip([*a.counters(), *_rng(a)], [*b.counters(), *_rng(b)]):
        assert torch.equal(p, q[perm])
    assert a.status() == 0 and b.status() == 0
    a.close(), b.close()


@pytest.mark.parametrize("mode", MODES)
def test_broadcast_clone_follows_the_oracle(mode):
    """1 024 envs step 60 times, then env 17 is cloned into every slot and all envs step 30 times with one action row: every
    env gives the same outputs, and those are the CPU oracle's, which has followed env 17 from its seeds."""
    n_envs, src = 1024, 17
    vec = _make(n_envs, mode)
    seeds = np.arange(n_envs, dtype=np.uint64) * 7919 + 11
    ref = oracle.OracleEnv(vec.cfg)
    ref.seed(int(seeds[src]), int(seeds[src]))
    acts = torch.empty((n_envs, vec.N_AGENTS), dtype=torch.int8, device=vec.device)

    def check_oracle(a_row, ctx, full):
        if ref.get_state().done:
            ref.reset()
        rw, dn, status = ref.step(a_row)
        assert status == 0, ctx
        assert np.array_equal(vec.rewards64[src].cpu().numpy(), rw) and int(vec.done[src]) == int(dn), ctx
        if full:
            o, m = ref.observe()
            assert np.array_equal(vec.obs[src].cpu().numpy(), o), ctx
            assert np.array_equal(vec.meta[src].cpu().numpy().view(np.uint16), m.view(np.uint16)), ctx

    for t in range(60):
        _run(vec, t, 1, record=False, acts=acts)
        check_oracle(acts[src].cpu().numpy(), f"{mode} step {t}", full=t % 20 == 19)
    vec.clone_envs(np.full(n_envs, src), np.arange(n_envs))
    vec.observe()
    for t in range(60, 90):
        vec.random_actions(acts, seed=ACT_SEED, step=t)
        acts.copy_(acts[src].clone().expand(n_envs, -1))
        vec.step_observe(acts, auto_reset=True, want_f64=True)
        for x in _outputs(vec):
            assert torch.equal(x, x[:1].expand_as(x)), f"{mode} step {t}: the clones differ"
        check_oracle(acts[src].cpu().numpy(), f"{mode} step {t}", full=True)
    assert vec.status() == 0
    vec.close()


@pytest.mark.parametrize("mode", MODES)
def test_subset_load_leaves_the_others_alone(mode):
    n_envs = 1024
    vec = _make(n_envs, mode)
    _run(vec, 0, 20, record=False)
    early = vec.save_states()
    _run(vec, 20, 25, record=False)
    before = vec.save_states()
    g = torch.Generator().manual_seed(9)
    dst = torch.randperm(n_envs, generator=g)[: n_envs // 10].to(vec.device)
    src = torch.randint(0, n_envs, (dst.numel(),), generator=g).to(vec.device)
    vec.load_states(early[src].contiguous(), dst)
    after = vec.save_states()
    keep = torch.ones(n_envs, dtype=torch.bool, device=vec.device)
    keep[dst] = False
    assert torch.equal(after[keep], before[keep]), "an env outside the subset changed"
    assert torch.equal(after[dst], early[src]), "the loaded envs"
    assert vec.status() == 0
    vec.close()


@pytest.mark.parametrize("mode", MODES)
def test_records_move_across_handles_and_through_a_file(mode, tmp_path):
    """A (4 096 envs, seeds s1) -> torch.save -> torch.load -> B (1 024 envs, seeds s2, same kwargs) at chosen indices: B's
    envs replay A's."""
    a, b = _make(4096, mode, seed_base=11), _make(1024, mode, seed_base=123457)
    assert a.fingerprint == b.fingerprint and a.snapshot_bytes == b.snapshot_bytes
    _run(a, 0, 120, record=False)
    _run(b, 0, 7, record=False)
    g = torch.Generator().manual_seed(21)
    src = torch.randperm(4096, generator=g)[:300]
    dst = torch.randperm(1024, generator=g)[:300]
    torch.save(a.save_states(src), tmp_path / "records.pt")
    recs = torch.load(tmp_path / "records.pt").to(b.device)
    b.load_states(recs, dst.numpy())
    b.observe()
    src, dst = src.to(a.device), dst.to(a.device)
    xa = torch.empty((4096, a.N_AGENTS), dtype=torch.int8, device=a.device)
    xb = torch.empty((1024, b.N_AGENTS), dtype=torch.int8, device=b.device)
    for t in range(120, 160):
        a.random_actions(xa, seed=ACT_SEED, step=t)
        b.random_actions(xb, seed=77, step=t)
        xb[dst] = xa[src]
        a.step_observe(xa, auto_reset=True, want_f64=True)
        b.step_observe(xb, auto_reset=True, want_f64=True)
        _same([o[dst] for o in _outputs(b)], [o[src] for o in _outputs(a)], f"{mode} step {t}")
    assert a.status() == 0 and b.status() == 0
    a.close(), b.close()


@pytest.mark.parametrize("mode", MODES)
def test_rejection(mode):
    n_envs = 256
    vec = _make(n_envs, mode)
    _run(vec, 0, 30, record=False)
    good = vec.save_states(torch.tensor([3], device=vec.device))

    def refused(recs, idx=None, check=True):
        before = vec.save_states()
        vec.load_states(recs, idx, check=check)
        assert vec.status() == abi.ST_BAD_SNAPSHOT
        assert torch.equal(vec.save_states(), before), "a refused record changed an env"

    for offset, what in ((8, "fingerprint"), (0, "magic"), (4, "layout version")):
        bad = good.clone()
        bad[0, offset] ^= 0x5A
        refused(bad, [5])
    refused(good, torch.tensor([n_envs], dtype=torch.int32, device=vec.device), check=False)
    refused(good, torch.tensor([-1], dtype=torch.int64, device=vec.device), check=False)

    # other configs: another map, the other RNG mode, metrics off
    others = [_make(8, mode, name="split"), _make(8, "counter" if mode == "mt19937" else "mt19937"), _make(8, mode, log_metrics=False)]
    fps = {vec.fingerprint} | {o.fingerprint for o in others}
    assert len(fps) == 4, "the fingerprints of four different configs"
    for o in others:
        recs = o.save_states(torch.tensor([1], device=o.device))
        if recs.shape[1] != vec.snapshot_bytes:
            with pytest.raises(ValueError):
                vec.load_states(recs, [2])
        else:
            refused(recs, [2])
        assert o.status() == 0
        o.close()
    twin = _make(64, mode, seed_base=999)
    assert twin.fingerprint == vec.fingerprint
    twin.close()

    with pytest.raises(ValueError):
        vec.load_states(good.view(torch.int8), [1])
    with pytest.raises(ValueError):
        vec.load_states(good[:, :-256], [1])
    with pytest.raises(ValueError):
        vec.load_states(good.reshape(-1), [1])
    with pytest.raises(ValueError):
        vec.load_states(good.cpu(), [1])
    with pytest.raises(ValueError):
        vec.load_states(torch.cat([good, good]), [4, 4])
    with pytest.raises(ValueError):
        vec.load_states(good, [n_envs])
    with pytest.raises(ValueError):
        vec.save_states(out=torch.empty((n_envs, vec.snapshot_bytes), dtype=torch.uint8))
    assert vec.status() == 0
    vec.close()


@pytest.mark.parametrize("mode", MODES)
def test_restore_inside_a_captured_graph(mode):
    """load_states(fixed, check=False) + 16 step_observe calls with fixed actions, captured once, replayed three times: every
    replay gives the eager run's outputs and ends in its state."""
    n_envs, K = 512, 16
    vec = _make(n_envs, mode)
    _run(vec, 0, 25, record=False)
    fixed = vec.save_states()
    table = torch.empty((K, n_envs, vec.N_AGENTS), dtype=torch.int8, device=vec.device)
    for k in range(K):
        vec.random_actions(table[k], seed=ACT_SEED, step=100 + k)
    bufs = [tuple(torch.empty_like(x) for x in _outputs(vec)) for _ in range(K)]

    def steps():
        vec.load_states(fixed, check=False)
        for k in range(K):
            vec.step_observe(table[k], auto_reset=True, want_f64=True)
            for dst, src in zip(bufs[k], (vec.obs, vec.meta.view(torch.int16), vec.rewards.view(torch.int32),
                                          vec.rewards64.view(torch.int64), vec.done)):
                dst.copy_(src)

    steps()
    eager = [tuple(x.clone() for x in b) for b in bufs]
    eager_end = vec.save_states()
    _run(vec, 25, 5, record=False)  # move away from that state
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream(device=vec.device)):
        steps()
    torch.cuda.synchronize()
    for rep in range(3):
        for b in bufs:
            for x in b:
                x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in range(K):
            _same(eager[k], bufs[k], f"{mode} replay {rep} step {k}")
        assert torch.equal(vec.save_states(), eager_end), f"{mode} replay {rep}: the state after the graph"
    assert vec.status() == 0
    vec.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["0", "1"])
def test_full_size_round_trip_both_launch_modes(mode, path, monkeypatch):
    """The round trip of test_round_trip_replays_bit_for_bit at bench size (65 536 envs) through both forms of step_observe:
    two launches (k_step + the tile render) and one (k_step_observe).  The final records are compared as _same_records says: at
    this size the step kernel's ring regeneration is not deterministic in its timing, only in its results."""
    _roundtrip(65536, mode, True, monkeypatch=monkeypatch, path=path, exact=False)


def test_the_reward_constants_are_part_of_the_fingerprint(monkeypatch):
    """ctf_snapshot.h hashes the six reward constants of the config; the env kwargs cannot vary them, so no other test does.  Two
    handles that differ in ``reward_tag`` alone (tests/_rule_cases.py edits the config build_config returns) have different
    fingerprints and each refuses the other's records, env untouched; so does a change of any other of the six."""
    import _rule_cases as rc

    seeds = np.arange(8, dtype=np.uint64) + 3
    make = lambda consts: rc.open_vec(monkeypatch, "tag", consts, 8, device=0, py_seeds=seeds, np_seeds=seeds)
    a, twin, b = make("VIS"), make("VIS"), make(dict(rc.VIS, reward_tag=0.41))
    assert a.fingerprint == twin.fingerprint and a.fingerprint != b.fingerprint and a.snapshot_bytes == b.snapshot_bytes
    acts = torch.full((8, a.N_AGENTS), 1, dtype=torch.int8, device=a.device)
    for vec in (a, b):
        vec.step(acts)
    for src, dst in ((a, b), (b, a)):
        recs, before = src.save_states(), dst.save_states()
        dst.load_states(recs)
        assert dst.status() == abi.ST_BAD_SNAPSHOT
        assert torch.equal(dst.save_states(), before), "a refused record changed an env"
        assert src.status() == 0
    twin.load_states(a.save_states())
    assert twin.status() == 0 and torch.equal(twin.save_states(), a.save_states())
    fps = {a.fingerprint, b.fingerprint}
    for field in rc.VIS:
        if field != "reward_tag":
            other = make(dict(rc.VIS, **{field: rc.VIS[field] + 0.25}))
            fps.add(other.fingerprint)
            other.close()
    assert len(fps) == 7, "every one of the six constants changes the fingerprint"
    for vec in (a, twin, b):
        vec.close()

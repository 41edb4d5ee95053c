"""The retained observation buffer (include/ctf_env.h: ctf_obs_retain): renders into the buffer a VecGridworldCtf allocated itself
rewrite only the 128-byte lines that changed since the last render into it (k_observe_delta).  The bytes must be those of the
full render whatever happened in between: checked against the CPU oracle, and against a TWIN handle seeded alike whose
retention is switched off (CTF_OBS_RETAIN=0 is read when a buffer is retained), after every step.

Small shapes at which the kernel can still go wrong: the arena at 3, 70 and 1 030 envs (ragged blocks of four waves; env blocks of
196.875 lines, so every lead of a block inside its first line occurs), 0_the_split at 64 (a block smaller than a render tile),
the 20 x 20 arena at 33 (more than one pass of grid dwords per wave) and a config whose block is no multiple of 16 bytes
(retention does not apply).  Everything runs with tune_placement=False."""
import numpy as np
import pytest

import oracle
from _cases import Case, abi, pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPES = [("arena", 3), ("arena", 70), ("arena", 1030), ("split", 64), ("arena20", 33)]
POISON = 0xA5


def _kwargs(name, **over):
    if name == "arena20":
        kw = dict(pkg.configs.ARENA20_KWARGS, SCENARIO=pkg.configs.arena20_scenario())
    elif name == "split":
        kw = dict(pkg.configs.SPLIT_KWARGS, SCENARIO=pkg.CtfScenarios.arrow)
    elif name == "arena":
        kw = dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii)
    else:
        kw = dict(Case(name).kwargs)
    kw.update(over)
    return kw


def _seeds(n, first=0):
    return (np.arange(n, dtype=np.uint64) + np.uint64(first)) * np.uint64(7919) + np.uint64(11)


def _make(kwargs, n_envs, retain, monkeypatch, first=0, **opts):
    """a handle whose own observation buffer is retained (or, ``retain=False``, the twin: the same buffer rendered in full)"""
    s = _seeds(n_envs, first)
    v = pkg.VecGridworldCtf(n_envs, device=0, py_seeds=s, np_seeds=s, tune_placement=False, **opts, **kwargs)
    monkeypatch.setenv("CTF_OBS_RETAIN", "1" if retain else "0")
    v.obs  # allocated, and handed to the library, here
    monkeypatch.delenv("CTF_OBS_RETAIN")
    return v


def _pair(name, n_envs, monkeypatch, over=None, **opts):
    kw = _kwargs(name, **(over or {}))
    a, b = _make(kw, n_envs, True, monkeypatch, **opts), _make(kw, n_envs, False, monkeypatch, **opts)
    assert a.observe_retained() and not b.observe_retained()
    assert a.step_observe_launches() == 2 and a.observe_kernel() == b.observe_kernel()  # the existing queries keep their answers
    return a, b


def _same(a, b, ctx):
    assert torch.equal(a.obs, b.obs), f"{ctx}: observations"
    assert torch.equal(a.meta.view(torch.int16), b.meta.view(torch.int16)), f"{ctx}: metadata"


def _acts(v, steps, seed=0x51DE, env_offset=0):
    acts = torch.empty((steps, v.n_envs, v.N_AGENTS), dtype=torch.int8, device=v.device)
    for t in range(steps):
        v.random_actions(acts[t], seed=seed, step=t, env_offset=env_offset)
    return acts


def _steps(a, b, acts, ctx, t0=0):
    for t in range(acts.shape[0]):
        a.step_observe(acts[t], auto_reset=True)
        b.step_observe(acts[t], auto_reset=True)
        _same(a, b, f"{ctx} step {t0 + t}")
        assert torch.equal(a.rewards, b.rewards) and torch.equal(a.done, b.done), f"{ctx} step {t0 + t}: rewards / done"


def _close(*vs):
    for v in vs:
        assert v.status() == 0
        v.close()


@pytest.mark.parametrize("name,n_envs", SHAPES)
def test_against_the_oracle_bit_for_bit(name, n_envs, monkeypatch):
    """obs and meta after every one of 40 step_observe(auto_reset=True) calls; GAME_STEPS = 7, so episodes end (and envs are reset
    inside the step launch, behind the render's back) five times in the run."""
    kw = _kwargs(name, GAME_STEPS=7)
    a = _make(kw, n_envs, True, monkeypatch)
    assert a.observe_retained()
    refs = [oracle.OracleEnv(a.cfg) for _ in range(n_envs)]
    for r, s in zip(refs, _seeds(n_envs)):
        r.seed(int(s), int(s))
    acts = _acts(a, 40)
    host_acts = acts.cpu().numpy()
    done = [False] * n_envs
    want_obs = np.zeros(tuple(a.obs.shape), np.uint8)
    want_meta = np.zeros(tuple(a.meta.shape), np.uint16)
    for t in range(40):
        a.step_observe(acts[t], auto_reset=True)
        for e, r in enumerate(refs):
            if done[e]:
                r.reset()
            _, done[e], st = r.step(host_acts[t, e])
            assert st == 0, f"{name}: the oracle raised status {st} for env {e} at step {t}"
            o, m = r.observe()
            want_obs[e], want_meta[e] = o, np.asarray(m).view(np.uint16)
        got = a.obs.cpu().numpy()
        if not np.array_equal(got, want_obs):
            bad = np.argwhere(got != want_obs)
            raise AssertionError(f"{name} {n_envs} step {t}: {len(bad)} observation bytes differ from the oracle's, the first at {bad[0]}")
        assert np.array_equal(a.meta.cpu().numpy().view(np.uint16), want_meta), f"{name} {n_envs} step {t}: metadata"
    _close(a)


@pytest.mark.parametrize("name,n_envs,opts,lanes", [(n, e, {}, None) for n, e in SHAPES] + [
    ("arena", 70, {"log_metrics": False}, None),
    ("arena", 70, {"rng_mode": "counter"}, None),
    ("arena", 70, {}, 1), ("arena", 70, {}, 2), ("arena", 70, {}, 4), ("arena", 70, {}, 8),
])
def test_against_the_twin_that_renders_in_full(name, n_envs, opts, lanes, monkeypatch):
    if lanes is not None:
        monkeypatch.setenv("CTF_STEP_W", str(lanes))  # read when the handle is created
    a, b = _pair(name, n_envs, monkeypatch, over=dict(GAME_STEPS=25), **opts)
    _steps(a, b, _acts(a, 60), f"{name} {n_envs} {opts} W={lanes}")
    _close(a, b)


def test_a_block_that_is_no_multiple_of_16_bytes_is_not_retained(monkeypatch):
    a, b = (_make(_kwargs("donut_1v1"), 37, r, monkeypatch) for r in (True, False))
    assert int(np.prod(a.obs.shape[1:])) % 16 != 0
    assert not a.observe_retained() and not b.observe_retained() and a.observe_kernel() == "k_observe"
    _steps(a, b, _acts(a, 20), "donut_1v1")
    _close(a, b)


def test_state_changed_behind_the_render(monkeypatch):
    """reset of a subset, set_state of one env, the batched import, snapshot restore and clone: the next render equals the twin's"""
    a, b = _pair("arena", 70, monkeypatch, over=dict(GAME_STEPS=25))
    acts = _acts(a, 24)
    early = [v.save_states() for v in (a, b)]
    _steps(a, b, acts[:6], "warm-up")
    mask = (torch.arange(70, device=a.device) % 3 == 1).to(torch.uint8)

    def each(what, fn):
        for v in (a, b):
            fn(v)
            v.observe()
        _same(a, b, what)

    each("reset(mask)", lambda v: v.reset(mask))
    _steps(a, b, acts[6:9], "after reset(mask)", 6)
    each("set_state", lambda v: v.set_state(5, v.get_state(9)))
    _steps(a, b, acts[9:12], "after set_state", 9)
    src, dst = np.array([1, 2, 3, 68]), np.array([40, 0, 69, 7])
    each("batched import", lambda v: v.set_states(v.get_states(src, fields=[f for f in abi.STATE_FIELDS[:-2]]), dst))
    _steps(a, b, acts[12:15], "after the batched import", 12)
    for v, rec in zip((a, b), early):
        v.load_states(rec[10:30], np.arange(20, 40))
        v.observe()
    _same(a, b, "snapshot restore")
    _steps(a, b, acts[15:18], "after the restore", 15)
    each("clone", lambda v: v.clone_envs(np.array([0, 1, 2]), np.array([2, 0, 1])))
    _steps(a, b, acts[18:], "after the clone", 18)
    _close(a, b)


@pytest.mark.parametrize("flip", [None, 0, 1, 2])
def test_buffer_changed_behind_the_render_and_reverse_masks(flip, monkeypatch):
    """somebody fills the retained buffer: invalidate_obs() and the next render is whole again; then reverse masks A, B, A (a
    render under another mask than the last is a full one by the shadow's key alone)"""
    scen = dict(pkg.CtfScenarios.arena_iii, FLIP_AXIS=flip)
    a, b = _pair("arena", 70, monkeypatch, over=dict(SCENARIO=scen, GAME_STEPS=25))
    acts = _acts(a, 8)
    _steps(a, b, acts[:3], f"flip {flip}")
    a.obs.fill_(POISON)
    a.invalidate_obs()
    for v in (a, b):
        v.observe()
    _same(a, b, f"flip {flip}: after fill + invalidate")
    A, B = 0b10100110, 0b00001111
    for k, m in enumerate((A, B, A, A, None, B)):
        for v in (a, b):
            v.step(acts[3 + k % 5], auto_reset=True)
            v.observe(reverse_mask=m)
        _same(a, b, f"flip {flip}: mask #{k} = {m}")
    _close(a, b)


def test_the_delta_path_is_really_taken(monkeypatch):
    """Poison the buffer behind a delta render and step once WITHOUT invalidating: every env keeps poison somewhere (it was not
    rewritten whole), and every line in which the twin's two renders differ was rewritten (within the env the change is in)."""
    E = 70
    a, b = _pair("arena", E, monkeypatch, over=dict(GAME_STEPS=25))
    acts = _acts(a, 6)
    _steps(a, b, acts[:4], "warm-up")
    before = b.obs.clone()
    a.obs.fill_(POISON)
    a.step_observe(acts[4], auto_reset=True)
    b.step_observe(acts[4], auto_reset=True)
    OB = int(np.prod(a.obs.shape[1:]))
    got, want, old = (x.reshape(E, OB).cpu().numpy() for x in (a.obs, b.obs, before))
    assert ((got == POISON).any(axis=1)).all(), "an env's block was rewritten whole: not the delta path"
    lead0 = a.obs.data_ptr() % 128
    changed = 0
    for e, f in zip(*np.nonzero(want != old)):
        line = (lead0 + e * OB + f) >> 7
        lo, hi = max(0, line * 128 - lead0 - e * OB), min(OB, (line + 1) * 128 - lead0 - e * OB)
        assert np.array_equal(got[e, lo:hi], want[e, lo:hi]), f"env {e}: the line of changed byte {f} was not rewritten"
        changed += 1
    assert changed > E, "the step changed almost nothing: the test shows nothing"
    a.invalidate_obs()
    a.step_observe(acts[5], auto_reset=True)
    b.step_observe(acts[5], auto_reset=True)
    _same(a, b, "after invalidate")
    _close(a, b)


def test_metadata_only_call_between_two_delta_renders(monkeypatch):
    a, b = _pair("arena", 70, monkeypatch)
    acts = _acts(a, 6)
    _steps(a, b, acts[:3], "before")
    for v in (a, b):
        v.step(acts[3], auto_reset=True)
        v.observe(obs=False)  # the state has moved on, the buffer (and so the shadow) must not
        v.step(acts[4], auto_reset=True)
        v.observe(obs=False)
    assert torch.equal(a.meta.view(torch.int16), b.meta.view(torch.int16))
    _steps(a, b, acts[5:], "after", 5)
    _close(a, b)


def test_full_render_into_a_second_buffer_and_back(monkeypatch):
    a, b = _pair("arena", 70, monkeypatch)
    acts = _acts(a, 8)
    _steps(a, b, acts[:3], "before")
    second = torch.full_like(a.obs, POISON)
    for v in (a, b):
        v.step(acts[3], auto_reset=True)
    a._call("ctf_observe", second.data_ptr(), a.meta.data_ptr(), abi.REVERSE_DEFAULT, a._stream())  # not the retained pointer
    b.observe()
    assert torch.equal(second, b.obs), "a render into another pointer is a full render"
    assert a.observe_retained()
    _steps(a, b, acts[4:6], "back on the retained buffer", 4)  # whose shadow still describes the render of step 2
    own = a.obs
    a.obs = second  # assigned: the caller's, released
    assert not a.observe_retained()
    second.fill_(POISON)
    _steps(a, b, acts[6:7], "assigned buffer", 6)
    a.obs = own
    assert not a.observe_retained()
    own.fill_(POISON)
    _steps(a, b, acts[7:], "own buffer after a release: full renders", 7)
    _close(a, b)


def test_one_launch_alternating_with_two_launches_on_one_retained_buffer(monkeypatch):
    """CTF_STEP_OBSERVE_ONE_LAUNCH (read at every call) wins over retention: k_step_observe renders in full and clears the keys"""
    a, b = _pair("arena", 70, monkeypatch, over=dict(GAME_STEPS=25))
    acts = _acts(a, 40)
    for t, one in enumerate([1, 0, 0, 1, 1, 0, 1, 0] * 5):
        monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", str(one))
        assert a.step_observe_launches() == (1 if one else 2) and a.observe_retained()
        a.step_observe(acts[t], auto_reset=True)
        monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", "0")
        b.step_observe(acts[t], auto_reset=True)
        _same(a, b, f"step {t} ({'one launch' if one else 'two launches'})")
    _close(a, b)


def test_guard_bands_around_a_retained_caller_buffer(monkeypatch):
    """obs and meta inside padded allocations (the observation block starts 80 bytes into a line: the first and the last line of
    every env's span are shared with a neighbour or with the pad): after 20 steps the pads hold their pattern"""
    E, PAD = 70, 80
    a, b = _pair("arena", E, monkeypatch, over=dict(GAME_STEPS=9))
    n_obs, n_meta = a.obs.numel(), a.meta.numel()
    big = torch.full((PAD + n_obs + 2 * PAD,), 0x5A, dtype=torch.uint8, device=a.device)
    mbig = torch.full((4 + n_meta + 8,), -1.5, dtype=torch.float16, device=a.device)
    assert big.data_ptr() % 128 == 0
    a.obs = big[PAD:PAD + n_obs].view(a.obs.shape)
    a.meta = mbig[4:4 + n_meta].view(a.meta.shape)
    a._call("ctf_obs_retain", a.obs.data_ptr(), a._stream())  # the caller's own promise for its own buffer
    assert a.observe_retained()
    _steps(a, b, _acts(a, 20), "padded")
    assert bool((big[:PAD] == 0x5A).all()) and bool((big[PAD + n_obs:] == 0x5A).all()), "observation pad bytes were written"
    assert bool((mbig[:4] == -1.5).all()) and bool((mbig[4 + n_meta:] == -1.5).all()), "metadata pad elements were written"
    _close(a, b)


def test_captured_step_observe_on_a_retained_buffer(monkeypatch):
    """A graph captured before the shadow was ever written (validity is device state: nothing the capture could freeze), replayed
    30 times against the eager twin; a second capture after eager calls; an invalidation between replays."""
    a, b = _pair("arena", 70, monkeypatch, over=dict(GAME_STEPS=11))
    acts = _acts(a, 44)
    cur = torch.empty_like(acts[0])
    side = torch.cuda.Stream(device=a.device)

    def capture():
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            a.step_observe(cur, auto_reset=True)
        torch.cuda.synchronize()
        return g

    def replay(g, t, ctx):
        cur.copy_(acts[t])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        b.step_observe(acts[t], auto_reset=True)
        _same(a, b, f"{ctx} step {t}")

    g1 = capture()  # (capturing runs nothing: the first render of all is replay 0)
    for t in range(30):
        replay(g1, t, "first graph")
    _steps(a, b, acts[30:33], "eager", 30)
    g2 = capture()
    for t in range(33, 38):
        replay(g2, t, "second graph")
    a.obs.fill_(POISON)
    a.invalidate_obs()
    for t in range(38, 41):
        replay(g2, t, "after fill + invalidate")
    a.obs.fill_(POISON)
    a.invalidate_obs()
    replay(g1, 41, "the first graph again")
    _steps(a, b, acts[42:], "eager again", 42)
    _close(a, b)


def test_two_handles_on_two_streams_against_one_batch(monkeypatch):
    """two retained handles of 35 envs each, free-running on two streams (no synchronisation inside the run), are the two
    halves of one batch of 70 rendered in full"""
    kw = _kwargs("arena", GAME_STEPS=9)
    h1 = _make(kw, 35, True, monkeypatch)
    h2 = _make(kw, 35, True, monkeypatch, first=35)
    b = _make(kw, 70, False, monkeypatch)
    assert h1.observe_retained() and h2.observe_retained()
    acts = _acts(b, 30)
    acts1, acts2 = acts[:, :35].contiguous(), acts[:, 35:].contiguous()
    s1, s2 = torch.cuda.Stream(device=b.device), torch.cuda.Stream(device=b.device)
    for lo in (0, 10, 20):
        torch.cuda.synchronize()
        for t in range(lo, lo + 10):
            with torch.cuda.stream(s1):
                h1.step_observe(acts1[t], auto_reset=True)
            with torch.cuda.stream(s2):
                h2.step_observe(acts2[t], auto_reset=True)
            b.step_observe(acts[t], auto_reset=True)
        torch.cuda.synchronize()
        assert torch.equal(torch.cat([h1.obs, h2.obs]), b.obs), f"after step {lo + 9}: observations"
        assert torch.equal(torch.cat([h1.meta, h2.meta]).view(torch.int16), b.meta.view(torch.int16)), f"after step {lo + 9}: metadata"
    _close(h1, h2, b)

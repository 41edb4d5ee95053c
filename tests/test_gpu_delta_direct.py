"""k_observe_delta as it makes its chunks from the slot images (marl-ctf-development_amd/csrc/ctf_obs_chunk.h), on the GPU: the
bytes of a retained buffer must be those of the full render, byte for byte — against a TWIN handle seeded alike whose retention
is switched off (CTF_OBS_RETAIN=0 is read when a buffer is retained).

Smallest shapes at which this kernel can still go wrong:
  arena, 9 envs     the block is 112 mod 128 bytes: eight consecutive envs take every lead 0, 16 .. 112 inside a line, plus one
  split, 5 envs     121-cell planes, a block smaller than a render tile
  arena20, 3 envs   planes that are whole chunks; 100 grid dwords: the second pass of the loads
  rand32, 3 envs    a random 32 x 32 map with 2 agents: 256 grid dwords, the fourth pass
each under all four flip axes and the reverse masks none / all / alternating / the default, 2-, 3- and 16-agent configurations
(slots nobody looks through, lopsided teams, 16 views), env counts one off a multiple of eight blocks, a caller-owned buffer at a
16-byte aligned address between guard bands, the round-11 kernel behind its switch, and both kinds of store."""
import numpy as np
import pytest

import _agent_counts
import test_gpu_random_configs as random_configs
from _cases import abi, pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = 0xA5
SHAPES = [("arena", 9), ("split", 5), ("arena20", 3), ("rand32", 3)]
FLIPS = [None, 0, 1, 2]


def _kwargs(name, flip="own", **over):
    if name == "arena20":
        kw = dict(pkg.configs.ARENA20_KWARGS, SCENARIO=pkg.configs.arena20_scenario())
    elif name == "split":
        kw = dict(pkg.configs.SPLIT_KWARGS, SCENARIO=pkg.CtfScenarios.arrow)
    elif name == "arena":
        kw = dict(pkg.configs.ARENA_KWARGS, SCENARIO=pkg.CtfScenarios.arena_iii)
    elif name == "rand32":
        kw = dict(random_configs.config_kwargs(32, 2))
    elif name.startswith("agents"):  # agents-N-lop: the agent-count sweep's config; agents-N-lop-g8: the same agents on an 8 x 8 map
        n, lop = (int(x) for x in name.split("-")[1:3])
        kw = dict(_agent_counts.config_kwargs(n, lop))
        if name.endswith("-g8"):  # 64-cell planes: a block of whole chunks whatever N and C are
            kw.update(SCENARIO=random_configs.random_scenario(np.random.default_rng(500 + n), 8, n), GRID_SIZE=8)
    else:
        raise KeyError(name)
    if flip != "own":
        kw["SCENARIO"] = dict(kw["SCENARIO"], FLIP_AXIS=flip)
        kw["MAP_SYMMETRY_CHECK"] = False
    kw.update(over)
    return kw


def _seeds(n):
    return np.arange(n, dtype=np.uint64) * np.uint64(7919) + np.uint64(11)


def _make(kwargs, n_envs, retain, monkeypatch, env=None):
    """a handle whose own observation buffer is retained (``env``: switches read at that moment) or, ``retain=False``, the twin"""
    s = _seeds(n_envs)
    v = pkg.VecGridworldCtf(n_envs, device=0, py_seeds=s, np_seeds=s, tune_placement=False, **kwargs)
    monkeypatch.setenv("CTF_OBS_RETAIN", "1" if retain else "0")
    for k, val in (env or {}).items():
        monkeypatch.setenv(k, val)
    v.obs  # allocated, and handed to the library, here
    monkeypatch.delenv("CTF_OBS_RETAIN")
    for k in env or {}:
        monkeypatch.delenv(k)
    return v


def _pair(kwargs, n_envs, monkeypatch, env=None):
    a, b = _make(kwargs, n_envs, True, monkeypatch, env), _make(kwargs, n_envs, False, monkeypatch)
    assert a.observe_retained() and not b.observe_retained()
    return a, b


def _acts(v, steps, seed=0xD1EC):
    acts = torch.empty((steps, v.n_envs, v.N_AGENTS), dtype=torch.int8, device=v.device)
    for t in range(steps):
        v.random_actions(acts[t], seed=seed, step=t)
    return acts


def _same(a, b, ctx):
    if not torch.equal(a.obs, b.obs):
        bad = torch.nonzero(a.obs != b.obs)
        raise AssertionError(f"{ctx}: {len(bad)} observation bytes differ from the full render's, the first at {bad[0].tolist()}")
    assert torch.equal(a.meta.view(torch.int16), b.meta.view(torch.int16)), f"{ctx}: metadata"


def _steps(vs, acts, ctx, reverse_mask=None):
    for t in range(acts.shape[0]):
        for v in vs:
            v.step_observe(acts[t], auto_reset=True, reverse_mask=reverse_mask)
        for v in vs[:-1]:
            _same(v, vs[-1], f"{ctx} step {t}")


def _close(*vs, clean=True):
    """``clean=False``: a random many-agent map may run out of respawn cells — then both handles say so alike"""
    for v in vs:
        assert v.status() == (0 if clean else vs[-1].status())
    for v in vs:
        v.close()


def _masks(n):
    every = (1 << n) - 1
    return [0, every, 0x5555 & every]


@pytest.mark.parametrize("flip", FLIPS)
@pytest.mark.parametrize("name,n_envs", SHAPES)
def test_every_chunk_of_a_first_render_is_the_full_renders(name, n_envs, flip, monkeypatch):
    """An unknown key makes every line dirty: one render into the poisoned retained buffer goes through the chunk computation for
    every chunk of every env.  A change of the reverse mask is an unknown key again."""
    a, b = _pair(_kwargs(name, flip), n_envs, monkeypatch)
    acts = _acts(a, 3)
    for t in range(3):  # away from the start state
        for v in (a, b):
            v.step(acts[t], auto_reset=True)
    for m in _masks(a.N_AGENTS):
        a.obs.fill_(POISON)
        a.invalidate_obs()
        a.observe(reverse_mask=m)
        b.observe(reverse_mask=m)
        _same(a, b, f"{name} flip {flip} mask {m:#x}")
    _close(a, b)


@pytest.mark.parametrize("mask", ["default", "alternating"])
@pytest.mark.parametrize("name,n_envs", SHAPES + [("agents-2-0", 9), ("agents-3-1", 9), ("agents-16-0", 9), ("agents-16-1", 9),
                                                  ("agents-2-0-g8", 9), ("agents-3-1-g8", 9)])
def test_forty_steps_against_the_twin_that_renders_in_full(name, n_envs, mask, monkeypatch):
    kw = _kwargs(name, GAME_STEPS=13)
    a, b = _make(kw, n_envs, True, monkeypatch), _make(kw, n_envs, False, monkeypatch)
    whole_chunks = int(np.prod(a.obs.shape[1:])) % 16 == 0
    assert a.observe_retained() == whole_chunks and not b.observe_retained()  # (a block of ragged chunks is rendered in full)
    if name.endswith("-g8") or name in dict(SHAPES):
        assert whole_chunks
    m = None if mask == "default" else 0x5555 & ((1 << a.N_AGENTS) - 1)
    _steps([a, b], _acts(a, 40), f"{name} {mask}", reverse_mask=m)
    _close(a, b, clean=not name.startswith("agents"))


@pytest.mark.parametrize("n_envs", [1, 7, 9, 15, 17, 31, 33])
def test_a_partial_last_block(n_envs, monkeypatch):
    """The launch is a multiple of eight blocks of 1, 2 or 4 waves (one env each): one env more and one less than 8, 16 and 32."""
    a, b = _pair(_kwargs("arena", GAME_STEPS=9), n_envs, monkeypatch)
    _steps([a, b], _acts(a, 12), f"arena {n_envs}")
    _close(a, b)


def test_guard_bands_around_a_callers_retained_buffer(monkeypatch):
    """The kernel writes a caller's buffer at addresses its lanes compute: 4 KiB of poison on both sides of a buffer that starts 16
    bytes into a 128-byte line stay poison over 20 steps."""
    E, GUARD = 9, 4096
    kw = _kwargs("arena", GAME_STEPS=9)
    s = _seeds(E)
    a = pkg.VecGridworldCtf(E, device=0, py_seeds=s, np_seeds=s, tune_placement=False, **kw)
    b = _make(kw, E, False, monkeypatch)
    shape = tuple(b.obs.shape)
    size = int(np.prod(shape))
    big = torch.full((GUARD + 128 + size + GUARD,), POISON, dtype=torch.uint8, device=a.device)
    off = GUARD + (16 - big.data_ptr() - GUARD) % 128
    buf = big[off:off + size].view(shape)
    assert buf.data_ptr() % 128 == 16
    a.obs = buf
    a._call("ctf_obs_retain", abi.ptr(buf), a._stream())
    assert a.observe_retained()
    _steps([a, b], _acts(a, 20), "guard bands")
    torch.cuda.synchronize()
    assert bool((big[:off] == POISON).all()) and bool((big[off + size:] == POISON).all()), "the render wrote outside the caller's buffer"
    _close(a, b)


def _delta_path_taken(vs, twin, acts, ctx):
    """Poison behind a delta render and step once WITHOUT invalidating: every env keeps poison somewhere (its block was not
    rewritten whole), and every line in which the twin's two renders differ was rewritten."""
    before = twin.obs.clone()
    for v in vs:
        v.obs.fill_(POISON)
    for v in vs + [twin]:
        v.step_observe(acts, auto_reset=True)
    E = twin.n_envs
    OB = int(np.prod(twin.obs.shape[1:]))
    want, old = (x.reshape(E, OB).cpu().numpy() for x in (twin.obs, before))
    for v in vs:
        got = v.obs.reshape(E, OB).cpu().numpy()
        assert ((got == POISON).any(axis=1)).all(), f"{ctx}: an env's block was rewritten whole: not the delta path"
        lead0 = v.obs.data_ptr() % 128
        changed = 0
        for e, f in zip(*np.nonzero(want != old)):
            line = (lead0 + e * OB + f) >> 7
            lo, hi = max(0, line * 128 - lead0 - e * OB), min(OB, (line + 1) * 128 - lead0 - e * OB)
            assert np.array_equal(got[e, lo:hi], want[e, lo:hi]), f"{ctx}: env {e}: the line of changed byte {f} was not rewritten"
            changed += 1
        assert changed > E, "the step changed almost nothing: the test shows nothing"
        v.invalidate_obs()


def test_the_round_11_kernel_behind_its_switch_writes_the_same_bytes(monkeypatch):
    kw = _kwargs("arena", GAME_STEPS=13)
    E = 33
    new = _make(kw, E, True, monkeypatch)
    old = _make(kw, E, True, monkeypatch, env={"CTF_OBS_DELTA_BITMAP": "1"})
    twin = _make(kw, E, False, monkeypatch)
    assert new.observe_retained() and old.observe_retained()
    acts = _acts(new, 41)
    _steps([new, old, twin], acts[:20], "before the poison")
    _delta_path_taken([new, old], twin, acts[20], "switch")
    _steps([new, old, twin], acts[21:], "after the poison")
    assert torch.equal(new.obs, old.obs)
    _close(new, old, twin)


def test_hinted_and_plain_stores_write_the_same_bytes(monkeypatch):
    kw = _kwargs("arena", GAME_STEPS=13)
    E = 33
    plain = _make(kw, E, True, monkeypatch, env={"CTF_OBS_DELTA_NT": "0"})
    hinted = _make(kw, E, True, monkeypatch, env={"CTF_OBS_DELTA_NT": "1"})
    twin = _make(kw, E, False, monkeypatch)
    acts = _acts(plain, 40)
    _steps([plain, hinted, twin], acts, "store hint")
    assert torch.equal(plain.obs, hinted.obs)
    _close(plain, hinted, twin)

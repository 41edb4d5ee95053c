"""k_observe_delta with the slot images kept in the shadow and carried forward (round 13), on the GPU.  A retained image that is
wrong by one bit shows in the buffer only once a line holding that bit is rewritten, so most tests here retain their buffer with
CTF_OBS_DELTA_ALL_DIRTY=1: every line is rewritten at every render while the images still come from the shadow and are still
carried forward, and the whole buffer must equal, after every step, that of a TWIN handle seeded alike which renders in full
(CTF_OBS_RETAIN=0).  Helpers and shapes are those of test_gpu_delta_direct.py.

Batches: 1 env (one wave), 9 (under one group of eight blocks, every lead 0 .. 112 of the arena's block), 33 (a ragged last group).
Shapes: arena (two slots under the default mask: one image unit per lane), split (the image load is largest relative to the
block), arena20 (two passes over the grid dwords), the 16-agent configurations (16 viewers per changed cell; four slots)."""
import numpy as np
import pytest

import test_gpu_delta_direct as dd
from _cases import abi, pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ALL_DIRTY = {"CTF_OBS_DELTA_ALL_DIRTY": "1"}
POISON = dd.POISON


def _alternating(v):
    """every other agent OF EACH TEAM reversed: all four slots (2 * team + reversed) are looked through where a team has two agents
    (0x5555 would not do: the arena's teams alternate with the agent index themselves)"""
    seen, m = [0, 0], 0
    for i in range(v.N_AGENTS):
        t = int(v.cfg.agent_team[i]) & 1
        m |= (seen[t] & 1) << i
        seen[t] += 1
    return m


def _slots(v, m):
    return {2 * (int(v.cfg.agent_team[i]) & 1) + ((m >> i) & 1) for i in range(v.N_AGENTS)}


@pytest.mark.parametrize("mask", ["default", "alternating"])
@pytest.mark.parametrize("name,n_envs", [("arena", 9), ("arena", 1), ("split", 33), ("arena20", 9), ("agents-16-0", 9), ("agents-16-1", 33)])
def test_sixty_all_dirty_steps_show_the_carried_images(name, n_envs, mask, monkeypatch):
    """Episodes of 13 steps: resets and auto-resets (many cells at once) come with the steps' few cells."""
    kw = dd._kwargs(name, GAME_STEPS=13)
    a, b = dd._make(kw, n_envs, True, monkeypatch, env=ALL_DIRTY), dd._make(kw, n_envs, False, monkeypatch)
    assert a.observe_retained() and not b.observe_retained()
    m = None if mask == "default" else _alternating(a)
    if m is not None:
        assert _slots(a, m) == {0, 1, 2, 3}
    dd._steps([a, b], dd._acts(a, 60), f"{name} {mask} all-dirty", reverse_mask=m)
    dd._close(a, b, clean=not name.startswith("agents"))


def _planted(states, rng):
    """``states`` with other grids in most envs — any tile code may stand in any cell (set_state's rules): env 0 .. E-4 a random
    grid (nearly every cell changes), env E-3 the first six rows only (> 64 cells), env E-2 nothing, env E-1 only agent 0's position"""
    out = {k: v.clone() for k, v in states.items()}
    E, G = out["grid"].shape[0], out["grid"].shape[1]
    noise = torch.from_numpy(rng.integers(0, 14, size=(E, G, G), dtype=np.uint8)).to(out["grid"].device)
    out["grid"][:E - 3] = noise[:E - 3]
    out["grid"][E - 3, :6] = noise[E - 3, :6]
    pos = out["pos"][E - 1, 0]
    out["pos"][E - 1, 0] = torch.stack(((pos[0] + 3) % G, (pos[1] + 5) % G)).to(torch.int8)
    return out


@pytest.mark.parametrize("switch", ["default", "all-dirty"])
def test_whole_grid_replacement_at_a_known_key(switch, monkeypatch):
    """Between two retained renders set_states plants other grids: hundreds of changed cells at a key that is still the expected
    one — several marking passes, several image passes, several compaction passes, the emit loop's second iteration.  An env
    with no changed cell (its block is not written at all) and one in which only a viewer moved ride along."""
    E = 9
    kw = dd._kwargs("arena", GAME_STEPS=50)
    a = dd._make(kw, E, True, monkeypatch, env=ALL_DIRTY if switch == "all-dirty" else None)
    b = dd._make(kw, E, False, monkeypatch)
    acts = dd._acts(a, 12)
    dd._steps([a, b], acts[:4], "before")
    saved = a.get_states()
    planted = _planted(saved, np.random.default_rng(7))
    changed = (planted["grid"] != saved["grid"]).flatten(1).sum(1).cpu().numpy()
    assert (changed[:E - 2] >= 64).all() and changed[E - 2] == 0 and changed[E - 1] == 0
    quiet = a.obs[E - 2].flatten()[128:-128]  # inside env E-2's block, away from the lines it shares with its neighbours
    for what, states in (("planted", planted), ("restored", saved)):
        if switch == "default" and what == "planted":
            quiet.fill_(POISON)
        for v in (a, b):
            v.set_states(states)
            v.observe()
        if switch == "default" and what == "planted":
            assert bool((quiet == POISON).all()), "an env without a changed cell was rewritten: not the delta path"
            quiet.copy_(b.obs[E - 2].flatten()[128:-128])
        dd._same(a, b, f"{switch}: {what}")
    dd._steps([a, b], acts[4:], "after")
    dd._close(a, b)


def _further(a, c, b, mask, ctx):
    """One further all-dirty render through a second handle whose state is copied from the first: what its own carried (or, after
    a mask change, rebuilt) images give across the jump must be the twin's bytes too."""
    c.set_states(a.get_states())
    c.observe(reverse_mask=mask)
    assert torch.equal(c.obs, b.obs), f"{ctx}: the second handle's all-dirty render"


@pytest.mark.parametrize("switch", ["default", "all-dirty"])
@pytest.mark.parametrize("n_envs", [9, 33])
def test_events_that_make_the_images_stale(n_envs, switch, monkeypatch):
    """A mask change (default -> alternating -> default), invalidate_obs(), a masked reset and auto-resets at episodes' ends (the
    step count planted two short of GAME_STEPS): the bytes are the twin's at every step."""
    GAME_STEPS = 50
    kw = dd._kwargs("arena", GAME_STEPS=GAME_STEPS)
    a = dd._make(kw, n_envs, True, monkeypatch, env=ALL_DIRTY if switch == "all-dirty" else None)
    c = dd._make(kw, n_envs, True, monkeypatch, env=ALL_DIRTY)
    b = dd._make(kw, n_envs, False, monkeypatch)
    acts = dd._acts(a, 24)
    alt = _alternating(a)
    dd._steps([a, b], acts[:4], "start")
    _further(a, c, b, None, "start")
    at = 4
    for what, m in (("alternating", alt), ("default again", None)):
        for t in range(3):
            dd._steps([a, b], acts[at:at + 1], f"mask {what} {t}", reverse_mask=m)
            _further(a, c, b, m, f"mask {what} {t}")
            at += 1
    a.invalidate_obs()
    dd._steps([a, b], acts[at:at + 2], "invalidated")
    _further(a, c, b, None, "invalidated")
    at += 2
    some = (torch.arange(n_envs, device=a.device) % 3 == 1).to(torch.uint8)
    for v in (a, b):
        v.reset(some)
        v.observe()
    dd._same(a, b, "masked reset")
    _further(a, c, b, None, "masked reset")
    states = a.get_states()
    states["step_count"][::2] = GAME_STEPS - 2
    for v in (a, b):
        v.set_states(states)
    for t in range(5):  # the planted envs end their episodes at the second of these steps
        dd._steps([a, b], acts[at:at + 1], f"episode end {t}")
        _further(a, c, b, None, f"episode end {t}")
        at += 1
    assert int((a.get_states(fields=["step_count"])["step_count"][::2] < 5).sum()) == (n_envs + 1) // 2, "no auto-reset happened"
    dd._close(a, b)
    c.close()


@pytest.mark.parametrize("nt", ["0", "1"])
def test_rebuild_carried_and_bitmap_write_the_same_bytes(nt, monkeypatch):
    kw = dd._kwargs("arena", GAME_STEPS=13)
    E = 33
    new = dd._make(kw, E, True, monkeypatch, env={"CTF_OBS_DELTA_NT": nt})
    rebuild = dd._make(kw, E, True, monkeypatch, env={"CTF_OBS_DELTA_NT": nt, "CTF_OBS_DELTA_REBUILD": "1"})
    bitmap = dd._make(kw, E, True, monkeypatch, env={"CTF_OBS_DELTA_NT": nt, "CTF_OBS_DELTA_BITMAP": "1"})
    twin = dd._make(kw, E, False, monkeypatch)
    assert new.observe_retained() and rebuild.observe_retained() and bitmap.observe_retained()
    acts = dd._acts(new, 41)
    dd._steps([new, rebuild, bitmap, twin], acts[:20], "before the poison")
    dd._delta_path_taken([new, rebuild, bitmap], twin, acts[20], "switches")
    dd._steps([new, rebuild, bitmap, twin], acts[21:], "after the poison")
    assert torch.equal(new.obs, rebuild.obs) and torch.equal(new.obs, bitmap.obs)
    dd._close(new, rebuild, bitmap, twin)


def test_guard_bands_stay_untouched_under_the_all_dirty_switch(monkeypatch):
    """Every line of every env is written at every render: 4 KiB of poison on both sides of a caller's buffer that starts 16 bytes
    into a 128-byte line stay poison over 20 steps."""
    E, GUARD = 9, 4096
    kw = dd._kwargs("arena", GAME_STEPS=9)
    s = dd._seeds(E)
    a = pkg.VecGridworldCtf(E, device=0, py_seeds=s, np_seeds=s, tune_placement=False, **kw)
    b = dd._make(kw, E, False, monkeypatch)
    shape = tuple(b.obs.shape)
    size = int(np.prod(shape))
    big = torch.full((GUARD + 128 + size + GUARD,), POISON, dtype=torch.uint8, device=a.device)
    off = GUARD + (16 - big.data_ptr() - GUARD) % 128
    buf = big[off:off + size].view(shape)
    assert buf.data_ptr() % 128 == 16
    a.obs = buf
    monkeypatch.setenv("CTF_OBS_DELTA_ALL_DIRTY", "1")
    a._call("ctf_obs_retain", abi.ptr(buf), a._stream())
    monkeypatch.delenv("CTF_OBS_DELTA_ALL_DIRTY")
    assert a.observe_retained()
    dd._steps([a, b], dd._acts(a, 20), "guard bands, all dirty")
    torch.cuda.synchronize()
    assert bool((big[:off] == POISON).all()) and bool((big[off + size:] == POISON).all()), "the render wrote outside the caller's buffer"
    dd._close(a, b)

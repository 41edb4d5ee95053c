"""The metadata rows of the two-launch ctf_step_observe come from the step kernel (k_step / k_step_direct with META, ctf_meta.h) and
its render runs without them.  CTF_STEP_META=0, read at every call, gives the render's rows as before — so both run in one process.

  test_twin        two handles seeded alike and fed the same actions, one stepping with CTF_STEP_META=0: meta, obs, rewards, done after
                   every step and the status at the end, bit for bit, over 16 steps of GAME_STEPS = 6 (two episode ends; with
                   auto-reset and, without it, with the done envs stepped on), at E = 1, 15, 16, 17 and 33 (the ragged last step block
                   at every lane width), at CTF_STEP_W = 1, 2, 4, 8, in the three generator modes, on the arena, the split map and a
                   16-agent map, with metrics on and off, the buffer retained and not
  test_oracle      the metadata cases of tests/_obs_cases.py planted one step back (tests/_step_meta_cases.py; tests/test_step_meta_cpu.py
                   shows on the oracle alone that after the step they still reach every conversion class and hp / flag pattern),
                   stepped once: every env's rows are the oracle's, exactly
  the caller's buffer: guard bands around ``meta`` at E = 17, meta == NULL, obs == NULL, and a captured launch replayed over episode ends"""
import numpy as np
import pytest

import _obs_cases as oc
import _step_meta_cases as smc
import test_gpu_retained_render as rr
from _cases import abi, pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ENVS = (1, 15, 16, 17, 33)
STEPS, GAME_STEPS = 16, 6
GUARD = 0x7DAD  # a NaN no row holds
# (metrics, auto_reset, retained): two halves of the eight combinations, each holding every pair of settings of two switches
COMBOS = (((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)), ((0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)))


def _kwargs(name):
    if name == "term16":
        return dict(oc.kwargs("term16"), GAME_STEPS=GAME_STEPS)
    return rr._kwargs(name, GAME_STEPS=GAME_STEPS)


def _bits(t):
    return t.view(torch.int16)


def _step(vec, acts, on, monkeypatch, auto_reset=True):
    monkeypatch.setenv("CTF_STEP_META", "1" if on else "0")  # read at every call
    vec.step_observe(acts, auto_reset=auto_reset)


def _same(a, b, ctx):
    assert torch.equal(_bits(a.meta), _bits(b.meta)), f"{ctx}: metadata"
    assert torch.equal(a.obs, b.obs), f"{ctx}: observations"
    assert torch.equal(a.rewards, b.rewards) and torch.equal(a.done, b.done), f"{ctx}: rewards / done"


# ---- twin ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
@pytest.mark.parametrize("mode", ["mt19937", "counter", "counter_direct"])
@pytest.mark.parametrize("name", ["arena", "split", "term16"])
def test_twin(name, mode, lanes, monkeypatch):
    monkeypatch.setenv("CTF_STEP_W", str(lanes))  # read when a handle is created
    kw = _kwargs(name)
    seen = set()
    for k, n_envs in enumerate(ENVS):
        for metrics, auto_reset, retained in COMBOS[k % 2]:
            opts = dict(log_metrics=bool(metrics), rng_mode=mode)
            a, b = (rr._make(kw, n_envs, bool(retained), monkeypatch, **opts) for _ in range(2))
            assert a.step_observe_launches() == 2 and a.observe_retained() == b.observe_retained()
            seen.add((metrics, auto_reset, a.observe_retained()))
            acts = rr._acts(a, STEPS)
            ended = 0
            for t in range(STEPS):
                a.meta.fill_(float("nan"))  # every row is written at every call
                _step(a, acts[t], True, monkeypatch, bool(auto_reset))
                _step(b, acts[t], False, monkeypatch, bool(auto_reset))
                _same(a, b, f"{name} {mode} W={lanes} E={n_envs} metrics={metrics} auto_reset={auto_reset} retained={retained} step {t}")
                ended += int(a.done.sum())
            assert ended >= 2 * n_envs  # two episode ends per env (without auto-reset: done from the first end on)
            assert a.status() == b.status()
            a.close(), b.close()
    assert {s[:2] for s in seen} == {(m, r) for m in (0, 1) for r in (0, 1)}
    if name != "split":  # (the arena's and the 16-agent map's blocks are whole 16-byte chunks: retention applies)
        assert {s[2] for s in seen} == {True, False}


# ---- oracle ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
@pytest.mark.parametrize("name", oc.MAP_NAMES)
def test_oracle(name, lanes, monkeypatch):
    monkeypatch.setenv("CTF_STEP_W", str(lanes))
    pre = smc.predecessors(name)
    _, want = smc.stepped(name)
    sd = smc.seeds(len(pre))
    vec = pkg.VecGridworldCtf(len(pre), device=0, py_seeds=sd, np_seeds=sd, tune_placement=False, log_metrics=True, **oc.kwargs(name))
    vec.set_states({f: torch.from_numpy(a).to(vec.device) for f, a in oc.stacked(pre).items()})
    vec.meta.fill_(float("nan"))
    acts = torch.from_numpy(smc.stay(name, len(pre))).to(vec.device)
    _step(vec, acts, True, monkeypatch, auto_reset=False)
    torch.cuda.synchronize()
    bad = oc.compare(None, vec.meta.cpu().numpy(), None, want)
    assert not bad, f"{name} W={lanes}: " + "; ".join(bad)
    assert vec.status() == 0
    vec.close()


# ---- the caller's buffer -------------------------------------------------------------------------------------------------------------------------
def _raw_step_observe(vec, acts, obs, meta, monkeypatch, on=True):
    monkeypatch.setenv("CTF_STEP_META", "1" if on else "0")
    a = vec._check_dev(acts, torch.int8, vec.n_envs * vec.N_AGENTS)
    vec._call("ctf_step_observe", a, abi.ptr(vec.rewards), None, abi.ptr(vec.done), abi.ptr(obs), abi.ptr(meta), vec._reverse_bits(None),
              abi.STEP_AUTO_RESET, vec._stream())


@pytest.mark.parametrize("mode", ["mt19937", "counter_direct"])
@pytest.mark.parametrize("retained", [True, False])
def test_guard_bands_around_meta_stay_intact(retained, mode, monkeypatch):
    kw, n_envs, band = _kwargs("arena"), 17, 256
    a, b = (rr._make(kw, n_envs, retained, monkeypatch, rng_mode=mode) for _ in range(2))
    size = a.meta.numel()
    big = torch.full((size + 2 * band,), GUARD, dtype=torch.int16, device=a.device)
    a.meta = big[band:band + size].view(torch.float16).view(a.meta.shape)
    assert a.meta.data_ptr() % 8 == 0
    acts = rr._acts(a, 8)
    for t in range(8):
        _step(a, acts[t], True, monkeypatch)
        _step(b, acts[t], False, monkeypatch)
        _same(a, b, f"arena 17 retained={retained} {mode} step {t}")
        assert bool((big[:band] == GUARD).all()) and bool((big[band + size:] == GUARD).all()), f"step {t}: the step wrote outside the caller's meta"
    assert not bool((big[band:band + size] == GUARD).any())
    a.close(), b.close()


@pytest.mark.parametrize("retained", [True, False])
def test_meta_null_writes_no_row_and_obs_null_writes_the_rows(retained, monkeypatch):
    kw, n_envs = _kwargs("arena"), 17
    a, b = (rr._make(kw, n_envs, retained, monkeypatch) for _ in range(2))
    acts = rr._acts(a, 9)
    for t in range(9):
        _step(b, acts[t], False, monkeypatch)
        a.meta.view(torch.int16).fill_(GUARD)
        if t % 3 == 0:    # meta == NULL: the observations alone
            _raw_step_observe(a, acts[t], a.obs, None, monkeypatch)
            assert bool((a.meta.view(torch.int16) == GUARD).all()), f"step {t}: meta == NULL, and a row was written"
            assert torch.equal(a.obs, b.obs), f"step {t}: observations"
        elif t % 3 == 1:  # obs == NULL: the rows, from the step launch alone
            before = a.obs.clone()
            _raw_step_observe(a, acts[t], None, a.meta, monkeypatch)
            assert torch.equal(_bits(a.meta), _bits(b.meta)), f"step {t}: obs == NULL: metadata"
            assert torch.equal(a.obs, before), f"step {t}: obs == NULL, and the buffer was written"
        else:             # both again: the retained buffer catches up with the steps it did not see
            _step(a, acts[t], True, monkeypatch)
            _same(a, b, f"step {t}")
        assert torch.equal(a.rewards, b.rewards) and torch.equal(a.done, b.done), f"step {t}: rewards / done"
    assert a.status() == b.status() == 0
    a.close(), b.close()


@pytest.mark.parametrize("mode", ["mt19937", "counter_direct"])
def test_a_captured_launch_replays_over_episode_ends(mode, monkeypatch):
    kw, n_envs = _kwargs("arena"), 33
    a, b = (rr._make(kw, n_envs, True, monkeypatch, rng_mode=mode) for _ in range(2))
    acts = rr._acts(a, STEPS)
    table = torch.zeros_like(acts[0])
    a.observe(), b.observe()  # the first, full pass of the retained buffers: not part of the captured launch
    monkeypatch.setenv("CTF_STEP_META", "1")  # read when the call is captured
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=a.device)
    torch.cuda.synchronize(a.device)
    with torch.cuda.graph(graph, stream=side):  # capture only: nothing runs
        a.step_observe(table, auto_reset=True)
    torch.cuda.synchronize(a.device)
    ended = 0
    for t in range(STEPS):
        table.copy_(acts[t])
        a.meta.fill_(float("nan"))
        graph.replay()
        _step(b, acts[t], False, monkeypatch)
        torch.cuda.synchronize(a.device)
        _same(a, b, f"{mode} replay {t}")
        ended += int(a.done.sum())
    assert ended == 2 * n_envs and a.status() == b.status() == 0
    a.close(), b.close()

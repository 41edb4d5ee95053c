"""Every kernel that writes planes or metadata, on the planted states of tests/_obs_cases.py, against the CPU oracle — bytes of the
planes, bits of the metadata, every env of every handle (tests/test_obs_cases_cpu.py shows that the oracle equals the reference on the
whole table and that the table reaches every class of the f64 -> binary16 conversion, every hp and flag element, every tile code in
every cell and every ordered pair of codes; nothing of that is measured here).

One handle per (map, flip axis): env k holds state k of ``_states`` (the map's plane cases, then its metadata cases), planted with one
``set_states`` call, rendered under the table's four masks.  Which launch a case reaches is asserted before anything runs, through
the library's own queries and the header's rule (as tests/test_gpu_render_contract.py does):
  test_k_observe            k_observe<16>, <4>, <1>, by map and by the class of the output pointer; once with log_metrics off
  test_k_observe_tiles      k_observe_tiles<0> and <1> (term16's 11 264-byte blocks; wide16 for its metadata)
  test_k_observe_codes      k_observe_codes<true> and <false>: expanded codes, self cells, and the per-wave copy of the metadata table
  test_k_observe_delta      k_observe_delta in its four modes: a first render at an unknown key, the whole transition sequence at a
                            known one, then the metadata cases planted over an unchanged grid
  test_k_step_observe       one launch (k_step_observe) beside the two-launch call: planted, stepped once, compared after the step
  test_host_step            ctf_host_step on one-env handles"""
import numpy as np
import pytest

import _obs_cases as oc
import oracle
import test_gpu_delta_direct as dd
import test_gpu_retained_images as ri
from _cases import abi, pkg
from _rule_cases import STAY, to_view

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = 8192
POISON = 0xA5


# ---- states, handles, expectations -------------------------------------------------------------------------------------------------------
def _states(name):
    return [c.state for c in oc.plane_cases(name) + oc.meta_cases(name)]


def _tensors(states, device):
    return {f: torch.from_numpy(a).to(device) for f, a in oc.stacked(states).items()}


def _seeds(n):
    return np.arange(n, dtype=np.uint64) * np.uint64(6151) + np.uint64(17)


def _open(monkeypatch, name, flip, n_envs, log_metrics=True, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = _seeds(n_envs)
    vec = pkg.VecGridworldCtf(n_envs, device=0, py_seeds=s, np_seeds=s, tune_placement=False, log_metrics=log_metrics, **oc.kwargs(name, flip))
    assert (vec.N_AGENTS, vec.N_CHANNELS, vec.GRID_SIZE, vec.META_LEN) == oc.shape(name)
    assert oc.masks(name)[3] == ri._alternating(vec)
    return vec


_wanted = {}


def _want(name, flip, mask):
    """the oracle's render of ``_states(name)``, computed once per (map, flip axis, mask) and left unchanged"""
    key = (name, flip, mask)
    if key not in _wanted:
        obs, meta = oc.oracle_observe(oc.config(name, flip), _states(name), mask)
        obs.setflags(write=False), meta.setflags(write=False)
        _wanted[key] = (obs, meta)
    return _wanted[key]


def _caller_buffer(vec, delta):
    """``vec.obs`` := a caller's buffer ``delta`` bytes past a 128-byte line (an assigned buffer is rendered in full every time)"""
    shape = (vec.n_envs, vec.N_AGENTS, vec.N_CHANNELS, vec.GRID_SIZE, vec.GRID_SIZE)
    size = int(np.prod(shape))
    big = torch.full((size + 512,), POISON, dtype=torch.uint8, device=vec.device)
    off = (-big.data_ptr()) % 128 + delta
    vec.obs = big[off:off + size].view(shape)
    assert vec.obs.data_ptr() % 128 == delta and not vec.observe_retained()
    return big


def _launch(vec, tiles, nt="0", one_launch=0):
    """Asserts what the library says a render into ``vec.obs`` launches, by the header's rule -> the kernel's name"""
    a, ob = vec.obs.data_ptr(), int(np.prod(vec.obs.shape[1:]))
    assert ob == vec._lib.ctf_obs_bytes_per_env(vec._h)
    want_tiles = bool(a % 16 == 0 and ob % 16 == 0 and ob >= TILE and tiles)
    assert vec.observe_kernel() == ("k_observe_tiles" if want_tiles else "k_observe")
    assert vec.observe_stores() == ("nontemporal" if want_tiles and nt == "1" else "plain")
    assert vec.step_observe_launches() == (1 if want_tiles and one_launch else 2)
    if want_tiles:
        return f"k_observe_tiles<{nt}>"
    return "k_observe<%d>" % (16 if ob % 16 == 0 and a % 16 == 0 else 4 if ob % 4 == 0 and a % 4 == 0 else 1)


def _check(vec, want, what, obs=True):
    torch.cuda.synchronize()
    bad = oc.compare(vec.obs.cpu().numpy() if obs else None, vec.meta.cpu().numpy(), want[0] if obs else None, want[1])
    assert not bad, f"{what}: " + "; ".join(bad)


def _render_all(vec, name, flip, what):
    """the handle's states under the four masks, into a poisoned buffer each time"""
    for mask in oc.masks(name):
        vec.obs.fill_(POISON)
        vec.meta.fill_(float("nan"))
        vec.observe(reverse_mask=mask)
        _check(vec, _want(name, flip, mask), f"{what} flip {flip} mask {mask}")


# ---- k_observe<16>, <4>, <1> -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,delta,kernel,log_metrics", [
    ("term16", 0, "k_observe<16>", True), ("term16", 4, "k_observe<4>", True), ("term16", 1, "k_observe<1>", True),
    ("tag16", 16, "k_observe<16>", True), ("tag", 0, "k_observe<4>", True), ("tag", 0, "k_observe<4>", False), ("tag", 2, "k_observe<1>", True),
    ("flags", 0, "k_observe<4>", True), ("wide16", 48, "k_observe<16>", True)])
def test_k_observe(name, delta, kernel, log_metrics, monkeypatch):
    """By map (tag's 4 860-byte block is no multiple of 16) and by pointer class (a 4-aligned and a 1-aligned view of a larger tensor)."""
    monkeypatch.setenv("CTF_OBS_TILES", "0")  # read at every call: term16's blocks would take the tile render
    states = _states(name)
    for flip in oc.FLIPS:
        vec = _open(monkeypatch, name, flip, len(states), log_metrics=log_metrics)
        big = _caller_buffer(vec, delta)
        assert _launch(vec, tiles=0) == kernel
        vec.set_states(_tensors(states, vec.device))
        _render_all(vec, name, flip, f"{name} {kernel}")
        size = vec.obs.numel()
        lead = vec.obs.data_ptr() - big.data_ptr()
        assert bool((big[:lead] == POISON).all()) and bool((big[lead + size:] == POISON).all()), "the render wrote outside the caller's buffer"
        assert vec.status() == 0
        vec.close()


# ---- k_observe_tiles<0>, <1> ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nt", [("term16", "0"), ("term16", "1"), ("wide16", "0"), ("wide16", "1")])
def test_k_observe_tiles(name, nt, monkeypatch):
    monkeypatch.setenv("CTF_OBS_TILES", "1")
    states = _states(name)
    for flip in oc.FLIPS:
        vec = _open(monkeypatch, name, flip, len(states), CTF_OBS_NT=nt)  # read when the handle is created
        _caller_buffer(vec, 16)
        assert _launch(vec, tiles=1, nt=nt) == f"k_observe_tiles<{nt}>"
        vec.set_states(_tensors(states, vec.device))
        _render_all(vec, name, flip, f"{name} k_observe_tiles<{nt}>")
        assert vec.status() == 0
        vec.close()


# ---- k_observe_codes<true>, <false> --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,delta,variant", [
    ("term16", 0, "k_observe_codes<true>"), ("term16", 1, "k_observe_codes<false>"), ("tag16", 4, "k_observe_codes<true>"),
    ("tag", 0, "k_observe_codes<false>"), ("flags", 0, "k_observe_codes<true>"), ("flags", 2, "k_observe_codes<false>"),
    ("wide16", 0, "k_observe_codes<true>")])
def test_k_observe_codes(name, delta, variant, monkeypatch):
    """The codes expanded are the oracle's planes, the self cells are where the oracle's plane 0 holds its bit, and the metadata —
    through the table k_observe_codes builds per wave — are the oracle's bits."""
    states = _states(name)
    n, c, g, _ = oc.shape(name)
    for flip in oc.FLIPS:
        vec = _open(monkeypatch, name, flip, len(states))
        big = torch.full((len(states) * n * g * g + 256,), POISON, dtype=torch.uint8, device=vec.device)
        off = (-big.data_ptr()) % 128 + delta
        vec._codes = big[off:off + len(states) * n * g * g].view(len(states), n, g, g)
        assert variant == "k_observe_codes<%s>" % ("true" if (n * g * g) % 4 == 0 and vec.codes.data_ptr() % 4 == 0 else "false")
        vec.set_states(_tensors(states, vec.device))
        for mask in oc.masks(name):
            vec.codes.fill_(POISON)
            vec.meta.fill_(float("nan"))
            codes, meta = vec.observe_codes(reverse_mask=mask)
            torch.cuda.synchronize()
            want_obs, want_meta = _want(name, flip, mask)
            what = f"{name} {variant} flip {flip} mask {mask}"
            bad = oc.compare(pkg.expand_codes(codes.cpu().numpy(), c), meta.cpu().numpy(), want_obs, want_meta)
            assert not bad, f"{what}: " + "; ".join(bad)
            own = want_obs[:, :, 0].reshape(len(states), n, g * g)
            assert (own.sum(axis=2) == 1).all()
            assert np.array_equal(vec.self_cells.cpu().numpy().astype(np.int64), own.argmax(axis=2)), f"{what}: self cells"
        assert bool((big[:off] == POISON).all()) and bool((big[off + vec.codes.numel():] == POISON).all())
        assert vec.status() == 0
        vec.close()


# ---- k_observe_delta -------------------------------------------------------------------------------------------------------------------------
DELTA_MODES = {"default": {}, "all-dirty": {"CTF_OBS_DELTA_ALL_DIRTY": "1"}, "rebuild": {"CTF_OBS_DELTA_REBUILD": "1"},
               "bitmap": {"CTF_OBS_DELTA_BITMAP": "1"}}
POISON_AT = 5  # the transition render (the shift by five grids) behind which the quiet env must keep its poison


def _meta_over(states, cases):
    """``states`` with the metadata fields of ``cases`` planted over them, grid and positions unchanged (the cases are repeated to fill)"""
    out = []
    for k, s in enumerate(states):
        m = cases[k % len(cases)].state
        out.append(dict(s, hp=m["hp"], has_flag=m["has_flag"], step_count=m["step_count"], team_captures=m["team_captures"], done=m["done"]))
    return out


@pytest.mark.parametrize("flip", oc.FLIPS)
@pytest.mark.parametrize("name,mode", [("term16", m) for m in DELTA_MODES] + [("wide16", "default")])
def test_k_observe_delta(name, mode, flip, monkeypatch):
    cfg = oc.config(name, flip)
    K = oc.transition_renders(name)
    E = K + 1
    ref = oracle.OracleEnv(cfg)
    for mask in oc.masks(name):
        vec = dd._make(oc.kwargs(name, flip), E, True, monkeypatch, env=DELTA_MODES[mode])
        assert vec.observe_retained() and vec.obs.data_ptr() % 128 == 0
        what = f"{name} {mode} flip {flip} mask {mask}"
        # 1. the first render, at an unknown key: every byte of the poisoned buffer is written
        states = oc.transition_states(name, 0)
        vec.set_states(_tensors(states, vec.device))
        vec.obs.fill_(POISON)
        vec.invalidate_obs()
        vec.observe(reverse_mask=mask)
        _check(vec, oc.oracle_observe(cfg, states, mask, ref), f"{what}: first render")
        # 2. the transition sequence at a known key (set_states does not invalidate it): every ordered pair of codes
        quiet = vec.obs[K].flatten()[128:-128]  # inside the last env's block, which nothing changes
        for r in range(1, K):
            states = oc.transition_states(name, r)
            vec.set_states(_tensors(states, vec.device))
            poisoned = mode == "default" and r == POISON_AT
            if poisoned:
                quiet.fill_(POISON)
            vec.observe(reverse_mask=mask)
            want = oc.oracle_observe(cfg, states, mask, ref)
            if poisoned:
                assert bool((quiet == POISON).all()), f"{what}: an env nothing changed in was rewritten: not the delta path"
                quiet.copy_(torch.from_numpy(want[0][K].reshape(-1)[128:-128]).to(vec.device))
            _check(vec, want, f"{what}: shift by {r}")
        # 3. the metadata cases over the unchanged grid
        cases = oc.meta_cases(name)
        for lo in range(0, len(cases), E):
            planted = _meta_over(states, cases[lo:lo + E])
            vec.set_states(_tensors(planted, vec.device))
            vec.observe(reverse_mask=mask)
            _check(vec, oc.oracle_observe(cfg, planted, mask, ref), f"{what}: metadata cases from {lo}")
        assert vec.observe_retained() and vec.status() == 0
        vec.close()


# ---- k_step_observe ------------------------------------------------------------------------------------------------------------------------
_stepped = {}


def _actions(name, row, n_envs):
    n = oc.shape(name)[0]
    if row == "stay":
        return np.full((n_envs, n), STAY, np.int8)
    return np.random.default_rng(2718).integers(0, 9, (n_envs, n)).astype(np.int8)


def _want_stepped(name, flip, mask, row):
    """the oracle planted with every state, seeded as its env, stepped once with the row (no auto-reset) -> (planes, metadata bits)"""
    key = (name, flip, mask, row)
    if key not in _stepped:
        states, cfg = _states(name), oc.config(name, flip)
        acts, seeds = _actions(name, row, len(states)), _seeds(len(states))
        ref = oracle.OracleEnv(cfg)
        obs, meta = [], []
        for e, s in enumerate(states):
            ref.seed(int(seeds[e]), int(seeds[e]))
            ref.set_state(to_view(s))
            _, _, status = ref.step(acts[e])
            assert status == 0, (name, e)  # (the state after a step that found no respawn cell is not defined: the table has none)
            o, m = ref.observe(abi.REVERSE_DEFAULT if mask is None else mask)
            obs.append(o), meta.append(m.view(np.uint16))
        _stepped[key] = (np.stack(obs), np.stack(meta))
    return _stepped[key]


@pytest.mark.parametrize("flip", oc.FLIPS)
@pytest.mark.parametrize("name,one_launch", [("term16", 1), ("term16", 0), ("wide16", 1)])
def test_k_step_observe(name, one_launch, flip, monkeypatch):
    """Every state stepped once without auto-reset, all STAY and one drawn row: the done envs' step fraction passes 1, the capture
    counts of 2**31 - 2 and the step counts of 2**28 - 1 go through the step's own registers into the render."""
    monkeypatch.setenv("CTF_OBS_TILES", "1")
    monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", str(one_launch))  # both read at every call
    states = _states(name)
    assert any(s["done"] for s in states) and any(max(s["team_captures"]) == oc.CAPS_MAX for s in states)
    vec = _open(monkeypatch, name, flip, len(states))
    _caller_buffer(vec, 0)
    assert _launch(vec, tiles=1, one_launch=one_launch) == "k_observe_tiles<0>" and vec.step_observe_launches() == (1 if one_launch else 2)
    planted = _tensors(states, vec.device)
    seeds = _seeds(len(states))
    for mask in oc.masks(name):
        for row in ("stay", "drawn"):
            vec.seed(seeds, seeds)
            vec.set_states(planted)
            vec.obs.fill_(POISON)
            acts = torch.from_numpy(_actions(name, row, len(states))).to(vec.device)
            vec.step_observe(acts, auto_reset=False, reverse_mask=mask)
            _check(vec, _want_stepped(name, flip, mask, row), f"{name} launches {2 - one_launch} flip {flip} mask {mask} {row}")
    assert vec.status() == 0
    vec.close()


# ---- ctf_host_step -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flags", "tag16"])
def test_host_step(name, monkeypatch):
    """A one-env handle: ``set_state`` a case, ``host_step`` without a step, compare — every metadata case, and every plane case under
    every flip axis and mask."""
    n, c, g, m = oc.shape(name)
    for flip in oc.FLIPS:
        vec = _open(monkeypatch, name, flip, 1)
        cfg = oc.config(name, flip)
        ref = oracle.OracleEnv(cfg)
        cases = oc.plane_cases(name) + (oc.meta_cases(name) if flip is None else [])
        for case in cases:
            vec.set_state(0, to_view(case.state))
            for mask in oc.masks(name) if case in oc.plane_cases(name) else [None]:
                obs, meta = np.full((n, c, g, g), POISON, np.uint8), np.full((n, m), np.nan, np.float16)
                _, _, status, _, _, _ = vec.host_step(None, reverse_mask=mask, obs=obs, meta=meta)
                want = oc.oracle_observe(cfg, [case.state], mask, ref)
                bad = oc.compare(obs[None], meta[None], want[0], want[1])
                assert status == 0 and not bad, f"{name} flip {flip} {case.name} mask {mask}: " + "; ".join(bad)
        vec.close()

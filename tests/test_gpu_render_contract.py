"""What include/ctf_env.h promises a C caller about ctf_observe, ctf_observe_codes and ctf_step_observe beyond what the facade ever asks
for: output pointers of every alignment class (the launch is picked from the pointer's value), nothing written outside the caller's
buffers, reversal masks that use all four (team x reversed) views at once, every "or NULL" output, and the 8-byte alignment of meta_dev.

The entry points are called with plain integer addresses inside guarded allocations (``Guarded``: 16 KiB of 0x5A on either side, two
render tiles).  The reference is the CPU oracle: the device env is driven ~40 random steps, every env's state is handed to an
``oracle.OracleEnv`` (set_state(get_state)) and ``observe`` of that is the expectation; codes and self cells are derived from the
oracle's planes by the header's own sentence.  Every comparison is exact and covers every env.

Which launch a case reaches (asserted through ctf_observe_kernel / ctf_observe_stores_hinted / ctf_step_observe_launches before
anything runs; the width of k_observe and the variant of k_observe_codes follow from the header's rule for the pointer and the block):
  test_obs_pointer_classes        k_observe<16>, <4>, <1> and k_observe_tiles<0>, by pointer class
  test_codes_pointer_classes      k_observe_codes<true> and <false>
  test_masks_observe              k_observe<16>, <4>, <1>, k_observe_tiles<0> and <1> under seven masks
  test_masks_step_observe         k_step_observe (plain and hinted stores), and k_step + k_observe<4> behind one call
  test_masks_codes                k_observe_codes<true> and <false> under seven masks
  test_observe_null_outputs, test_observe_codes_output_subsets, test_step_null_outputs_twin     the "or NULL" outputs
  test_meta_aligned_offsets_render_exactly, test_misaligned_meta_is_refused                     meta_dev's alignment
"""
import math

import numpy as np
import pytest

import oracle
from _cases import Case, abi, pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = 0x5A
GUARD = 16384  # two render tiles: even a whole misplaced tile lands inside the test's own allocation
TILE = 8192
WARM = 40


# ---- guarded buffers ------------------------------------------------------------------------------------------------------------
class Guarded:
    """``nbytes`` of payload at ``base + GUARD + delta`` inside a uint8 tensor filled with 0x5A, ``base`` = the tensor's first
    4096-aligned address; at least GUARD bytes of the tensor follow the payload."""

    def __init__(self, nbytes, delta=0, device="cuda"):
        self.nbytes, self.delta = int(nbytes), int(delta)
        self.t = torch.full((4096 + 2 * GUARD + self.delta + self.nbytes,), FILL, dtype=torch.uint8, device=device)
        self.off = (-self.t.data_ptr()) % 4096 + GUARD + self.delta
        self.addr = self.t.data_ptr() + self.off
        assert (self.addr - self.delta) % 4096 == 0 and self.t.numel() - self.off - self.nbytes >= GUARD

    def payload(self):
        return self.t[self.off:self.off + self.nbytes]

    def bytes(self):
        return self.payload().cpu().numpy()

    def touched(self):
        """Offsets relative to the payload's first byte of the bytes outside the payload that are no longer 0x5A (the first few)."""
        bad = []
        for lo, part in ((0, self.t[:self.off]), (self.off + self.nbytes, self.t[self.off + self.nbytes:])):
            idx = (part != FILL).nonzero().flatten()
            bad += [int(i) + lo - self.off for i in idx[:8]]
        return bad

    def check_guards(self, what):
        bad = self.touched()
        assert not bad, f"{what}: bytes outside the caller's buffer were written, at payload offsets {bad}"

    def check_untouched(self, what):
        self.check_guards(what)
        assert bool((self.payload() == FILL).all()), f"{what}: a buffer that was not passed was written"


# ---- scenes: a device batch in a scattered state and the oracle's view of every env -----------------------------------------------
def _g32_kwargs():
    """The (G = 32, N = 16) shape of tests/test_gpu_random_configs.py, drawn as that test draws it."""
    from test_gpu_random_configs import random_scenario

    g, n = 32, 16
    rng = np.random.default_rng(1000 * g + n)
    scen = random_scenario(rng, g, n)
    return dict(
        SCENARIO=scen, AGENT_CONFIG={i: {"team": i % 2, "type": int(rng.integers(4))} for i in range(n)},
        GAME_STEPS=int(rng.integers(20, 45)), MAP_SYMMETRY_CHECK=False, USE_ADJUSTED_REWARDS=bool(rng.integers(2)),
        HOME_FLAG_CAPTURE=bool(rng.integers(2)), DROP_FLAG_WHEN_NO_HP=bool(rng.integers(2)),
        TAG_PROBABILITY=float(rng.choice([0.5, 0.75, 1.0])), AGENT_TYPE_HP={0: 2, 1: 3, 2: 2.5, 3: 1.5},
        AGENT_TYPE_DAMAGE={0: 1, 1: 0.5, 2: 0.75, 3: 1}, VAULT_HP_COST=0.5, VAULT_MIN_HP=0.75,
        AGENT_HP_HEALING_PER_STEP=float(rng.choice([0.25, 0.1])),
    )


SCENES = {  # key -> (golden case or None = the G = 32 shape, envs)
    "arena1": ("arena_random", 1), "arena3": ("arena_random", 3), "arena513": ("arena_random", 513), "g32": (None, 5),
    "split130": ("split_random", 130), "fence70": ("fence_axis0", 70), "donut77": ("donut_1v1", 77),
}


class Scene:
    def __init__(self, key, monkeypatch, nt="0", seed_mul=7919):
        name, E = SCENES[key]
        kwargs = _g32_kwargs() if name is None else Case(name).kwargs
        monkeypatch.setenv("CTF_OBS_NT", nt)  # read when the handle is created
        seeds = np.arange(E, dtype=np.uint64) * seed_mul + 11
        self.vec = v = pkg.VecGridworldCtf(E, device=0, py_seeds=seeds, np_seeds=seeds, tune_placement=False, **kwargs)
        self.key, self.nt = key, nt
        self.E, self.N, self.C, self.G, self.M = E, v.N_AGENTS, v.N_CHANNELS, v.GRID_SIZE, v.META_LEN
        self.GG = self.G * self.G
        self.obs_bytes = self.N * self.C * self.GG
        assert self.obs_bytes == v._lib.ctf_obs_bytes_per_env(v._h) and self.N * self.M == v._lib.ctf_meta_elems_per_env(v._h)
        self.tile_capable = self.obs_bytes % 16 == 0 and self.obs_bytes >= TILE
        self.acts = torch.empty((E, self.N), dtype=torch.int8, device=v.device)
        self.t = 0
        self.refs = [oracle.OracleEnv(v.cfg) for _ in range(E)]
        for _ in range(WARM):
            self.next_actions()
            v.step(self.acts, auto_reset=True)
        self.resync()

    def next_actions(self):
        self.vec.random_actions(self.acts, seed=0x0B5E, step=self.t)
        self.t += 1

    def resync(self):
        """The oracle envs take over the device's states as they are now."""
        torch.cuda.synchronize()
        self.views = [self.vec.get_state(e) for e in range(self.E)]
        for ref, view in zip(self.refs, self.views):
            ref.set_state(view)
        self._want = {}

    def want(self, mask):
        """-> dict(obs u8 [E,N,C,G,G], meta u16 [E,N,M], codes u8 [E,N,GG], selfcell u16 [E,N]) of the oracle under ``mask``."""
        if mask not in self._want:
            E, N, C, G = self.E, self.N, self.C, self.G
            obs, meta = np.empty((E, N, C, G, G), np.uint8), np.empty((E, N, self.M), np.uint16)
            rm = abi.REVERSE_DEFAULT if mask is None else int(mask)
            for e, ref in enumerate(self.refs):
                o, m = ref.observe(reverse_mask=rm)
                obs[e], meta[e] = o, m.view(np.uint16)
            # include/ctf_env.h: low 7 bits = index of the plane among 1..C-1 that is 1 (0 = none), bit 7 = plane 0; selfcell = the
            # flat index of plane 0's single bit
            planes = obs[:, :, 1:].reshape(E, N, C - 1, self.GG)
            assert planes.max() <= 1 and planes.sum(axis=2).max() <= 1, "the oracle's tile planes are not one-hot"
            index = (planes * np.arange(1, C, dtype=np.uint8)[None, None, :, None]).sum(axis=2).astype(np.uint8)
            own = obs[:, :, 0].reshape(E, N, self.GG)
            assert (own.sum(axis=2) == 1).all(), "the oracle's plane 0 does not hold exactly one bit"
            codes = (index | (own << 7)).astype(np.uint8)
            self._want[mask] = dict(obs=obs, meta=meta, codes=codes, selfcell=own.argmax(axis=2).astype(np.uint16))
        return self._want[mask]

    # -- sizes of the outputs in bytes
    def nbytes(self, what):
        return {"obs": self.E * self.obs_bytes, "meta": self.E * self.N * self.M * 2, "codes": self.E * self.N * self.GG,
                "selfcell": self.E * self.N * 2, "rw32": self.E * self.N * 4, "rw64": self.E * self.N * 8, "done": self.E}[what]

    def buf(self, what, delta=0):
        return Guarded(self.nbytes(what), delta)

    def masks(self):
        """[None, both views in each team, its complement, 1, 1 << (N - 1), two drawn ones]"""
        N, teams = self.N, self.vec.AGENT_TEAMS
        rank, seen = {}, {0: 0, 1: 0}
        for i in range(N):
            rank[i] = seen[teams[i]]
            seen[teams[i]] += 1
        both = sum(1 << i for i in range(N) if (rank[i] + teams[i]) % 2 == 0)
        for t in (0, 1):
            mine = [i for i in range(N) if teams[i] == t]
            if len(mine) >= 2:  # (a team of one has one view whatever the mask)
                assert {(both >> i) & 1 for i in mine} == {0, 1}, f"team {t} does not hold both views under {both:#x}"
        rng = np.random.default_rng(20 * N + self.G)
        drawn = [int(rng.integers(0, 1 << N)) for _ in range(2)]
        return [None, both, ~both & ((1 << N) - 1), 1, 1 << (N - 1)] + drawn

    def check_status(self):
        assert self.vec.status() & ~abi.ST_NO_RESPAWN == 0

    def close(self):
        self.vec.close()


@pytest.fixture(scope="module")
def scenes():
    """key (+ "+nt": hinted stores) -> Scene, built on first use and shared: nothing in the tests that take one changes its env state."""
    cache = {}

    def get(key):
        if key not in cache:
            with pytest.MonkeyPatch.context() as mp:
                cache[key] = Scene(key.split("+")[0], mp, nt="1" if key.endswith("+nt") else "0")
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


# ---- calls through the C ABI with plain addresses ---------------------------------------------------------------------------------
def _addr(b):
    return None if b is None else b.addr


def _observe(s, obs, meta, mask):
    abi.call(s.vec._lib, "ctf_observe", s.vec._h, _addr(obs), _addr(meta), s.vec._reverse_bits(mask), s.vec._stream())
    torch.cuda.synchronize()


def _observe_codes(s, codes, meta, selfcell, mask):
    abi.call(s.vec._lib, "ctf_observe_codes", s.vec._h, _addr(codes), _addr(meta), _addr(selfcell), s.vec._reverse_bits(mask),
             s.vec._stream())
    torch.cuda.synchronize()


def _step_observe(s, rw32, rw64, done, obs, meta, mask):
    abi.call(s.vec._lib, "ctf_step_observe", s.vec._h, s.acts.data_ptr(), _addr(rw32), _addr(rw64), _addr(done), _addr(obs), _addr(meta),
             s.vec._reverse_bits(mask), abi.STEP_AUTO_RESET, s.vec._stream())
    torch.cuda.synchronize()


def _knobs(monkeypatch, tiles=1, one_launch=0):
    monkeypatch.setenv("CTF_OBS_TILES", str(tiles))  # both are read at every call
    monkeypatch.setenv("CTF_STEP_OBSERVE_ONE_LAUNCH", str(one_launch))


def _expect_launch(s, obs, tiles, one_launch=0):
    """Asserts what the library says a render into ``obs`` launches, by the header's rule, and returns its name.  The facade's own
    queries are asked too, with the test's pointer as the object's buffer."""
    v, a = s.vec, obs.addr
    want_tiles = a % 16 == 0 and s.tile_capable and tiles != 0
    assert v._lib.ctf_observe_kernel(v._h, a) == int(want_tiles), f"ctf_observe_kernel for a pointer % 16 = {a % 16}"
    assert v._lib.ctf_observe_stores_hinted(v._h, a) == int(want_tiles and s.nt == "1")
    assert v._lib.ctf_step_observe_launches(v._h, a) == (1 if want_tiles and one_launch else 2)
    keep = v._obs
    v.obs = obs.payload().view(s.E, s.N, s.C, s.G, s.G)
    try:
        assert v.observe_kernel() == ("k_observe_tiles" if want_tiles else "k_observe")
        assert v.observe_stores() == ("nontemporal" if want_tiles and s.nt == "1" else "plain")
        assert v.step_observe_launches() == (1 if want_tiles and one_launch else 2)
    finally:
        v.obs = keep
    if want_tiles:
        return f"k_observe_tiles<{s.nt}>"
    return "k_observe<%d>" % (16 if s.obs_bytes % 16 == 0 and a % 16 == 0 else 4 if s.obs_bytes % 4 == 0 and a % 4 == 0 else 1)


def _codes_variant(s, codes):
    return "k_observe_codes<%s>" % ("true" if (s.N * s.GG) % 4 == 0 and codes.addr % 4 == 0 else "false")


def _same(got, want, shape, what):
    """``got``: the payload's bytes; ``want``: the oracle's array.  Exact; the message names the first byte that differs."""
    want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        at = np.unravel_index(i // (len(want) // int(np.prod(shape))), shape)
        raise AssertionError(f"{what}: {int((got != want).sum())} bytes differ, the first at byte {i} = index {tuple(int(x) for x in at)}: "
                             f"{got[i]:#x} != {want[i]:#x}")


def _check_obs(s, obs, meta, mask, what):
    w = s.want(mask)
    if obs is not None:
        obs.check_guards(what + " (obs)")
        _same(obs.bytes(), w["obs"], w["obs"].shape, what + ": observation")
    if meta is not None:
        meta.check_guards(what + " (meta)")
        _same(meta.bytes(), w["meta"], w["meta"].shape, what + ": metadata")


def _check_codes(s, codes, meta, selfcell, mask, what):
    w = s.want(mask)
    for b, k in ((codes, "codes"), (meta, "meta"), (selfcell, "selfcell")):
        if b is not None:
            b.check_guards(f"{what} ({k})")
            _same(b.bytes(), w[k], w[k].shape, f"{what}: {k}")


# ---- 1. pointer classes of obs_dev -----------------------------------------------------------------------------------------------
OBS_DELTAS = [0, 16, 48, 1008, 4, 8, 12, 1, 2, 3]


@pytest.mark.parametrize("delta", OBS_DELTAS)
@pytest.mark.parametrize("key,tiles", [("arena3", 1), ("arena3", 0), ("arena513", 1), ("arena513", 0), ("split130", 1)])
def test_obs_pointer_classes(key, tiles, delta, scenes, monkeypatch):
    """"identical bytes either way": the render into a pointer of every class — line-aligned, 16-byte aligned only, 4-byte, odd.  On the
    arena (25 200-byte blocks: 3.08 tiles, tiles straddle envs, a clamped last tile, at 513 envs a second group of one env) the
    4-byte and byte paths render a tile-capable config; split_random (3 872 bytes: under one tile) varies k_observe<16>'s k0."""
    s = scenes(key)
    if key.startswith("arena"):
        assert s.tile_capable and TILE // math.gcd(s.obs_bytes, TILE) == 512 and s.obs_bytes % TILE != 0
    else:
        assert s.obs_bytes % 16 == 0 and s.obs_bytes < TILE
    _knobs(monkeypatch, tiles=tiles, one_launch=1)
    obs = s.buf("obs", delta)
    kernel = _expect_launch(s, obs, tiles, one_launch=1)
    assert s.vec._lib.ctf_observe_kernel(s.vec._h, obs.addr) == int(delta % 16 == 0 and key.startswith("arena") and tiles != 0)
    assert kernel == ("k_observe_tiles<0>" if delta % 16 == 0 and key.startswith("arena") and tiles else
                      "k_observe<16>" if delta % 16 == 0 else "k_observe<4>" if delta % 4 == 0 else "k_observe<1>")
    for mask in (None, s.masks()[1]):
        meta = s.buf("meta")
        obs.payload().fill_(FILL)
        _observe(s, obs, meta, mask)
        _check_obs(s, obs, meta, mask, f"{key} tiles={tiles} delta={delta} {kernel} mask={mask}")
    s.check_status()


# ---- 2. pointer classes of codes_dev ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0, 4, 1, 2, 3])
@pytest.mark.parametrize("key", ["arena3", "arena513", "donut77"])
def test_codes_pointer_classes(key, delta, scenes):
    """The compact observation through the dword and the byte variant.  Arena: N * GG % 4 == 0 and GG % 4 != 0, so output dwords run
    across agent rows and a dword-capable row is also written through the byte path."""
    s = scenes(key)
    if key.startswith("arena"):
        assert (s.N * s.GG) % 4 == 0 and s.GG % 4 != 0
    codes = s.buf("codes", delta)
    variant = _codes_variant(s, codes)
    if key.startswith("arena"):
        assert variant == ("k_observe_codes<true>" if delta % 4 == 0 else "k_observe_codes<false>")
    for mask in (None, s.masks()[1]):
        meta, selfcell = s.buf("meta"), s.buf("selfcell")
        codes.payload().fill_(FILL)
        _observe_codes(s, codes, meta, selfcell, mask)
        _check_codes(s, codes, meta, selfcell, mask, f"{key} delta={delta} {variant} mask={mask}")
    s.check_status()


# ---- 3. mixed reversal masks against the oracle, every render launch --------------------------------------------------------------
@pytest.mark.parametrize("kernel,key,tiles,delta", [
    ("k_observe<16>", "arena3", 0, 0), ("k_observe<16>", "arena513", 0, 48), ("k_observe<16>", "split130", 1, 0), ("k_observe<16>", "g32", 0, 16),
    ("k_observe<4>", "fence70", 1, 0), ("k_observe<4>", "arena3", 1, 4), ("k_observe<4>", "arena513", 0, 12),
    ("k_observe<1>", "donut77", 1, 0), ("k_observe<1>", "arena3", 1, 1), ("k_observe<1>", "fence70", 1, 2), ("k_observe<1>", "arena513", 1, 3),
    ("k_observe_tiles<0>", "arena1", 1, 0), ("k_observe_tiles<0>", "arena3", 1, 0), ("k_observe_tiles<0>", "arena513", 1, 1008),
    ("k_observe_tiles<0>", "g32", 1, 0),
    ("k_observe_tiles<1>", "arena3+nt", 1, 0), ("k_observe_tiles<1>", "arena513+nt", 1, 16), ("k_observe_tiles<1>", "g32+nt", 1, 0),
])
def test_masks_observe(kernel, key, tiles, delta, scenes, monkeypatch):
    """Masks under which all four (team x reversed) views are live at once and two agents of one team look differently — including
    the views of env e0 + 1 in a tile that straddles two envs (arena) and a config whose blocks are whole tiles (G = 32)."""
    s = scenes(key)
    if key.startswith("g32"):
        assert TILE // math.gcd(s.obs_bytes, TILE) <= 2  # envs per tile group: the blocks are whole tiles (or halves), tile_k is small
    _knobs(monkeypatch, tiles=tiles)
    obs = s.buf("obs", delta)
    assert _expect_launch(s, obs, tiles) == kernel
    for mask in s.masks():
        meta = s.buf("meta")
        obs.payload().fill_(FILL)
        _observe(s, obs, meta, mask)
        _check_obs(s, obs, meta, mask, f"{key} {kernel} delta={delta} mask={mask if mask is None else bin(mask)}")
    s.check_status()


@pytest.mark.parametrize("key,nt,one_launch", [("arena3", "0", 1), ("arena513", "0", 1), ("arena3", "1", 1), ("g32", "0", 1), ("arena3", "0", 0)])
def test_masks_step_observe(key, nt, one_launch, monkeypatch):
    """ctf_step_observe under the seven masks, one step each, into obs pointers that are 16-byte but not line aligned and meta pointers
    at 8-byte offsets: the expectation is the oracle's render of get_state AFTER the call.  One launch (k_step_observe), and for
    comparison the two launches; a 4-byte obs pointer stays two launches whatever the switch says."""
    s = Scene(key, monkeypatch, nt=nt, seed_mul=6151)
    _knobs(monkeypatch, tiles=1, one_launch=one_launch)
    deltas = [0, 16, 48, 1008, 4, 16, 48]
    meta_deltas = [0, 8, 24, 1000, 8, 0, 24]
    for mask, delta, md in zip(s.masks(), deltas, meta_deltas):
        obs, meta = s.buf("obs", delta), s.buf("meta", md)
        rw32, rw64, done = s.buf("rw32"), s.buf("rw64"), s.buf("done")
        kernel = _expect_launch(s, obs, 1, one_launch=one_launch)
        launches = s.vec._lib.ctf_step_observe_launches(s.vec._h, obs.addr)
        assert launches == (1 if one_launch and delta % 16 == 0 else 2)
        assert kernel == ("k_observe<4>" if delta % 16 else f"k_observe_tiles<{nt}>")
        s.next_actions()
        _step_observe(s, rw32, rw64, done, obs, meta, mask)
        s.resync()
        what = f"{key} nt={nt} launches={launches} delta={delta} meta+{md} mask={mask if mask is None else bin(mask)}"
        _check_obs(s, obs, meta, mask, what)
        for b in (rw32, rw64, done):
            b.check_guards(what)
        assert np.array_equal(rw64.bytes().view(np.float64).astype(np.float32), rw32.bytes().view(np.float32)), what
        assert np.array_equal(done.bytes(), np.array([v.done for v in s.views], np.uint8)), what
    s.check_status()
    s.close()


@pytest.mark.parametrize("variant,key,delta", [
    ("k_observe_codes<true>", "arena3", 0), ("k_observe_codes<true>", "arena513", 4), ("k_observe_codes<true>", "g32", 0),
    ("k_observe_codes<false>", "arena3", 1), ("k_observe_codes<false>", "arena513", 2), ("k_observe_codes<false>", "donut77", 0),
    ("k_observe_codes<false>", "fence70", 3),
])
def test_masks_codes(variant, key, delta, scenes):
    s = scenes(key)
    codes = s.buf("codes", delta)
    assert _codes_variant(s, codes) == variant
    for mask in s.masks():
        meta, selfcell = s.buf("meta"), s.buf("selfcell")
        codes.payload().fill_(FILL)
        _observe_codes(s, codes, meta, selfcell, mask)
        _check_codes(s, codes, meta, selfcell, mask, f"{key} {variant} delta={delta} mask={mask if mask is None else bin(mask)}")
    s.check_status()


# ---- 4. the "or NULL" outputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,tiles", [("arena1", 1), ("arena3", 1), ("arena3", 0), ("arena513", 1), ("split130", 1), ("donut77", 1)])
def test_observe_null_outputs(key, tiles, scenes, monkeypatch):
    """ctf_observe with (obs, NULL) and with (NULL, meta): the buffer that is not passed stays 0x5A."""
    s = scenes(key)
    _knobs(monkeypatch, tiles=tiles)
    mask = s.masks()[1]
    for give_obs in (True, False):
        obs, meta = s.buf("obs"), s.buf("meta")
        if give_obs:
            _expect_launch(s, obs, tiles)
        _observe(s, obs if give_obs else None, None if give_obs else meta, mask)
        what = f"{key} tiles={tiles} " + ("(obs, NULL)" if give_obs else "(NULL, meta)")
        _check_obs(s, obs if give_obs else None, None if give_obs else meta, mask, what)
        (meta if give_obs else obs).check_untouched(what)
    obs, meta = s.buf("obs"), s.buf("meta")
    _observe(s, None, None, mask)  # nothing asked for: nothing launched
    obs.check_untouched("(NULL, NULL)"), meta.check_untouched("(NULL, NULL)")
    s.check_status()


@pytest.mark.parametrize("subset", [("codes",), ("meta",), ("selfcell",), ("codes", "meta"), ("codes", "selfcell"), ("meta", "selfcell"),
                                    ("codes", "meta", "selfcell")], ids="+".join)
@pytest.mark.parametrize("key,delta", [("arena3", 0), ("arena513", 1), ("donut77", 0)])
def test_observe_codes_output_subsets(key, delta, subset, scenes):
    """Every non-empty subset of ctf_observe_codes's three optional outputs (the kernel leaves early for "no codes", "no codes and no
    self cells" and "no meta"): what is passed is exact, what is not stays 0x5A."""
    s = scenes(key)
    mask = s.masks()[2]
    bufs = dict(codes=s.buf("codes", delta), meta=s.buf("meta"), selfcell=s.buf("selfcell"))
    given = {k: (b if k in subset else None) for k, b in bufs.items()}
    _observe_codes(s, given["codes"], given["meta"], given["selfcell"], mask)
    what = f"{key} outputs {subset}"
    _check_codes(s, given["codes"], given["meta"], given["selfcell"], mask, what)
    for k, b in bufs.items():
        if k not in subset:
            b.check_untouched(f"{what}: {k}")
    s.check_status()


@pytest.mark.parametrize("entry", ["ctf_step", "ctf_step_observe two launches", "ctf_step_observe one launch"])
def test_step_null_outputs_twin(entry, monkeypatch):
    """rewards_f32_dev = rewards_f64_dev = done_dev = NULL on a twin of a handle that passes them (same seeds, same actions, 24 steps
    with auto-reset): states, counters, both generators' states and the render afterwards are identical, and the render is the oracle's."""
    _knobs(monkeypatch, tiles=1, one_launch=int(entry.endswith("one launch")))
    a, b = Scene("arena3", monkeypatch, seed_mul=4099), Scene("arena3", monkeypatch, seed_mul=4099)
    for t in range(24):
        a.next_actions(), b.next_actions()
        assert torch.equal(a.acts, b.acts)
        outs = [a.buf("rw32"), a.buf("rw64"), a.buf("done")]
        obs = [x.buf("obs", 16) for x in (a, b)]
        meta = [x.buf("meta") for x in (a, b)]
        if entry == "ctf_step":
            for x, o in ((a, outs), (b, [None] * 3)):
                abi.call(x.vec._lib, "ctf_step", x.vec._h, x.acts.data_ptr(), _addr(o[0]), _addr(o[1]), _addr(o[2]), abi.STEP_AUTO_RESET,
                         x.vec._stream())
                _observe(x, obs[x is b], meta[x is b], None)
        else:
            assert a.vec._lib.ctf_step_observe_launches(a.vec._h, obs[0].addr) == (1 if entry.endswith("one launch") else 2)
            _step_observe(a, outs[0], outs[1], outs[2], obs[0], meta[0], None)
            _step_observe(b, None, None, None, obs[1], meta[1], None)
        for o in outs + obs + meta:
            o.check_guards(f"{entry} step {t}")
        assert torch.equal(obs[0].payload(), obs[1].payload()) and torch.equal(meta[0].payload(), meta[1].payload()), f"{entry} step {t}"
    a.resync(), b.resync()
    for e in range(a.E):
        assert bytes(a.views[e]) == bytes(b.views[e]), f"{entry}: state of env {e}"
    for x, y, what in zip(a.vec.counters(), b.vec.counters(), ("metrics", "captures", "step counts")):
        assert torch.equal(x, y), f"{entry}: {what}"
    for x, y in zip(a.vec.get_rng_states(), b.vec.get_rng_states()):
        assert torch.equal(x, y), f"{entry}: generator states"
    _check_obs(b, obs[1], meta[1], None, f"{entry}: the twin's last render")
    a.check_status(), b.check_status()
    a.close(), b.close()


# ---- 5. meta_dev must be 8-byte aligned ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [8, 24, 1000])
def test_meta_aligned_offsets_render_exactly(off, scenes, monkeypatch):
    """8-byte aligned is all the metadata rows' 8-byte stores need: through the tile render (the rows leave from the tile that holds
    an env's first byte), k_observe and k_observe_codes.  (ctf_step_observe at these offsets: test_masks_step_observe.)"""
    s = scenes("arena513")
    mask = s.masks()[1]
    for tiles in (1, 0):
        _knobs(monkeypatch, tiles=tiles)
        obs, meta = s.buf("obs"), s.buf("meta", off)
        kernel = _expect_launch(s, obs, tiles)
        _observe(s, obs, meta, mask)
        _check_obs(s, obs, meta, mask, f"meta + {off} {kernel}")
    codes, meta, selfcell = s.buf("codes"), s.buf("meta", off), s.buf("selfcell")
    _observe_codes(s, codes, meta, selfcell, mask)
    _check_codes(s, codes, meta, selfcell, mask, f"meta + {off} k_observe_codes")
    meta = s.buf("meta", off)
    _observe(s, None, meta, mask)
    _check_obs(s, None, meta, mask, f"meta + {off} (NULL, meta)")
    s.check_status()


@pytest.mark.parametrize("off", [2, 4])
def test_misaligned_meta_is_refused(off, monkeypatch):
    """Any other meta_dev is refused with CTF_E_INVALID and a message before anything is launched: no output is written, no status
    bit is raised, and ctf_step_observe does not step."""
    _knobs(monkeypatch, tiles=1)
    s = Scene("arena3", monkeypatch, seed_mul=5003)
    before = [bytes(v) for v in s.views]
    rng_before = [x.clone() for x in s.vec.get_rng_states()]
    obs, meta, codes, selfcell = s.buf("obs"), s.buf("meta", off), s.buf("codes"), s.buf("selfcell")
    rw32, rw64, done = s.buf("rw32"), s.buf("rw64"), s.buf("done")
    assert meta.addr % 8 == off
    s.next_actions()
    calls = {
        "ctf_observe": lambda: _observe(s, obs, meta, None),
        "ctf_observe (NULL, meta)": lambda: _observe(s, None, meta, None),
        "ctf_observe_codes": lambda: _observe_codes(s, codes, meta, selfcell, None),
        "ctf_observe_codes (NULL, meta, NULL)": lambda: _observe_codes(s, None, meta, None, None),
        "ctf_step_observe": lambda: _step_observe(s, rw32, rw64, done, obs, meta, None),
    }
    for name, fn in calls.items():
        with pytest.raises(abi.CtfLibraryError, match="meta_dev must be 8-byte aligned"):
            fn()
        torch.cuda.synchronize()
        for b in (obs, meta, codes, selfcell, rw32, rw64, done):
            b.check_untouched(f"{name} with meta_dev % 8 = {off}")
    assert s.vec.status() == 0
    s.resync()
    assert [bytes(v) for v in s.views] == before, "a refused ctf_step_observe stepped the envs"
    for x, y in zip(s.vec.get_rng_states(), rng_before):
        assert torch.equal(x, y), "a refused ctf_step_observe drew random numbers"
    s.close()

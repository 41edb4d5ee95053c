"""Host-side mirror of the reference's ``GridworldCtf`` (reference gridworld_ctf.py:13) over the C ABI.

Two classes:

``VecGridworldCtf``  E independent envs resident in HBM, stepped and rendered by HIP kernels; all I/O is
                     torch CUDA tensors handed to the C ABI as raw device pointers on the caller's
                     current HIP stream.  This is the fast path.
``GridworldCtf``     the reference's single-env API (same constructor kwargs, methods, attributes and
                     exceptions) as a batch of one, so ``ppo.py`` / ``utils.duel`` / the ``0_..8_*.py``
                     scripts run against it unchanged (put this directory first on sys.path).

There is no CPU fallback: without the HIP library and a GPU, construction raises.
"""
import ctypes as C
import random as _py_random
from collections import defaultdict
from functools import partial

import numpy as np

try:
    from . import _abi, config as _config
except ImportError:  # pragma: no cover - this directory itself on sys.path (drop-in use)
    import _abi
    import config as _config

__all__ = ["GridworldCtf", "VecGridworldCtf"]


def _torch():
    import torch

    return torch


def _as_seed_array(seeds, n):
    if seeds is None:
        seeds = np.arange(n, dtype=np.uint64)
    arr = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
    if arr.shape[0] != n:
        raise ValueError(f"need {n} seeds, got {arr.shape[0]}")
    return arr


def expand_codes(codes, n_channels):
    """codes uint8 [..., G, G] (observe_codes) -> the one-hot planes uint8 [..., C, G, G] of standardise_state
    (torch tensor or numpy array)."""
    if isinstance(codes, np.ndarray):
        k = np.arange(n_channels, dtype=np.uint8).reshape((n_channels, 1, 1))
        low, c = (codes & 0x7F)[..., None, :, :], codes[..., None, :, :]
        return np.where(k == 0, c >> 7, (low == k) & (k > 0)).astype(np.uint8)
    torch = _torch()
    k = torch.arange(n_channels, dtype=torch.uint8, device=codes.device).reshape((n_channels, 1, 1))
    low, c = (codes & 0x7F).unsqueeze(-3), codes.unsqueeze(-3)
    return torch.where(k == 0, c >> 7, ((low == k) & (k > 0)).to(torch.uint8))


class VecGridworldCtf:
    """``n_envs`` GridworldCtf instances on one MI355X.

    Env ``e`` reproduces, bit for bit, a reference process that ran
    ``random.seed(py_seeds[e]); np.random.seed(np_seeds[e])`` before constructing its env and was fed
    the same actions.  Outputs live in tensors owned by this object and are overwritten by the next call.

    RETAINED OBSERVATIONS.  The observation buffer this object allocates itself (``obs``, on first use) is handed to the library
    as retained (include/ctf_env.h, ctf_obs_retain): ``observe`` and ``step_observe`` then rewrite only the 128-byte lines of it
    that changed since their last render.  The results are the same bytes — as long as nobody else writes into ``vec.obs``.
    Whoever does (``vec.obs.fill_(...)``, a copy into it, another library) must call ``invalidate_obs()`` before the next
    render.  A buffer assigned through ``vec.obs = buf`` is the caller's and is rendered in full every time.
    ``observe_retained()`` says which of the two holds; CTF_OBS_RETAIN=0 in the environment switches retention off.
    """

    def __init__(self, n_envs, device=None, py_seeds=None, np_seeds=None, log_metrics=True, tune_placement=None, _lib=None,
                 rng_mode="mt19937", placement_tries=None, placement_gib=None, **env_kwargs):
        """tune_placement: pick the observation buffer among a few candidate allocations by timing the render into each
        (default: on for batches whose observation block exceeds 256 MiB).  On MI355X about half of all large hipMalloc
        allocations stream 20 % slower than the others (6.5 vs 5.3 TB/s for a bare store stream into the very same
        virtual address range after a free / re-allocate: it is the physical backing, profiles/r02_alloc_probe*.txt)."""
        torch = _torch()
        self._lib = _lib or _abi.load_library()  # _lib: a side-by-side build, profiling only (tools/ab_inproc.py)
        modes = {"mt19937": _abi.RNG_MT19937, "counter": _abi.RNG_COUNTER, "counter_direct": _abi.RNG_COUNTER_DIRECT}
        if rng_mode not in modes:
            raise ValueError("rng_mode must be 'mt19937' (the reference's generators, bit for bit), 'counter' or 'counter_direct'")
        # "counter": opt-in counter-based streams (include/ctf_env.h CTF_RNG_COUNTER) — word n of an env's stream is
        # Philox4x32-10(seed, n); the draws are made from those words by the reference's own rules.  "counter_direct": the same
        # streams, so the same trajectories, with no generator words stored (CTF_RNG_COUNTER_DIRECT: 32 bytes of RNG state per env)
        self.rng_mode = rng_mode
        self.cfg, self.derived = _config.build_config(env_kwargs, log_metrics=log_metrics, rng_mode=modes[rng_mode])
        if not torch.cuda.is_available():
            raise _abi.CtfLibraryError("no HIP device visible: the GridworldCtf kernels need a GPU (there is no CPU fallback)")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self.n_envs = int(n_envs)
        d = self.derived
        self.N_AGENTS, self.GRID_SIZE = d["n_agents"], d["grid_size"]
        self.N_CHANNELS, self.META_LEN = self.cfg.n_channels, 2 * d["n_agents"] + 6
        self.AGENT_TEAMS, self.AGENT_TYPES = d["agent_teams"], d["agent_types"]
        self.TILES_USED = d["tiles_used"]
        with torch.cuda.device(self.device):
            torch.cuda.current_stream()  # make sure torch has initialised HIP on this device first
            h = C.c_void_p()
            _abi.call(self._lib, "ctf_create", C.byref(self.cfg), self.n_envs, self.device.index, C.byref(h))
        self._h = h
        E, N = self.n_envs, self.N_AGENTS
        self.rewards = torch.zeros((E, N), dtype=torch.float32, device=self.device)
        self.rewards64 = torch.zeros((E, N), dtype=torch.float64, device=self.device)
        self.done = torch.zeros((E,), dtype=torch.uint8, device=self.device)
        self._obs = None  # uint8 [E, N, C, G, G]: allocated (and placed) on first use — a codes-only caller never pays for it
        self._codes = None
        self._self_cells = None
        self.meta = torch.zeros((E, N, self.META_LEN), dtype=torch.float16, device=self.device)
        self.seed(py_seeds, np_seeds)
        if tune_placement is None:
            tune_placement = E * N * self.N_CHANNELS * self.GRID_SIZE ** 2 > (256 << 20)
        self._tune_placement = bool(tune_placement)
        import os

        self._placement_tries = int(placement_tries if placement_tries is not None else os.environ.get("CTF_PLACEMENT_TRIES", 256))
        self._placement_gib = float(placement_gib if placement_gib is not None else os.environ.get("CTF_PLACEMENT_GIB", 16))
        self._placement_seconds = float(os.environ.get("CTF_PLACEMENT_SECONDS", 3.0))
        self.placement_probe_ms = None
        self.placement_fill_ms = None
        self.placement = None  # what the placement search found: kind fast / intermediate / slow, render / fill ratio, ...

    @property
    def obs(self):
        if self._obs is None:
            torch = _torch()
            self._obs = torch.zeros((self.n_envs, self.N_AGENTS, self.N_CHANNELS, self.GRID_SIZE, self.GRID_SIZE),
                                    dtype=torch.uint8, device=self.device)
            if self._tune_placement:
                self._tune_obs_placement()
            # ours, and nobody writes it from here on (the search's last fill_ is behind us): retained
            self._call("ctf_obs_retain", _abi.ptr(self._obs), self._stream())
        return self._obs

    @obs.setter
    def obs(self, buf):
        self._call("ctf_obs_retain", None, self._stream())  # an assigned buffer is the caller's: rendered in full (also the search's probes)
        self._obs = buf

    def invalidate_obs(self):
        """Tell the library that somebody else has written into the retained ``obs``: the next render writes every byte.
        Stream-ordered."""
        self._call("ctf_obs_invalidate", self._stream())

    def observe_retained(self):
        """True when ``observe`` / ``step_observe`` rewrite only the changed lines of this object's buffer (the delta render)."""
        return self._lib.ctf_observe_retained(self._h, _abi.ptr(self.obs)) == 1

    @property
    def codes(self):
        if self._codes is None:
            self._codes = _torch().zeros((self.n_envs, self.N_AGENTS, self.GRID_SIZE, self.GRID_SIZE), dtype=_torch().uint8,
                                         device=self.device)
        return self._codes

    def _tune_obs_placement(self, good_enough=0.95):
        """Keep the candidate allocation the render streams into fastest (see __init__).

        BOUNDED in what it HOLDS: one candidate beside the best one so far — two observation buffers, 3.3 GB for the arena batch —
        never more than ``placement_gib`` GiB (default 16; CTF_PLACEMENT_GIB; a batch whose two buffers exceed it is not searched)
        nor 45 % of the free device memory: a co-resident policy / learner is not starved while this searches.  A rejected candidate
        goes back to the driver at once (``torch.cuda.empty_cache``); the next allocation is of an independent kind even when nothing
        is held in between (tools/placement_probe2.py, profiles/r03_placement_search_strategies.txt: holding the rejected ones, as
        round 2 did, finds fast buffers no more often), so the search can afford ``placement_tries`` candidates (default 256;
        CTF_PLACEMENT_TRIES) at a few milliseconds each.  An allocation failure ends the search with what it has.

        The search stops at a candidate whose render takes at most ``good_enough`` x the time of a plain ``fill_`` of the same
        buffer (which does not depend on the buffer's kind; 0.95 is the very top of what any workload has shown, so in practice the
        time limit ends the search: stopping at 1.00 cost the 20 x 20 map 5-8 % when the first candidate under it was a 0.99), or — once it holds one of the fast kind (render / fill <= 1.08: with the
        render's nontemporal stores the kinds lie at 1.02-1.07 and 1.15-1.26 for the 15 x 15 arena, from 0.95 in a continuum for the
        20 x 20 one, the fill itself 0.234-0.245 ms from box to box; profiles/r05_render_nontemporal.md) — when
        ``placement_seconds`` of wall time are used up; ten seconds while it holds none.  ``self.placement`` says what was found."""
        import time

        torch = _torch()
        stream = torch.cuda.current_stream(self.device)

        def timed(fn, reps=3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            a.record(stream)
            for _ in range(reps):
                fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / reps

        def probe(buf):
            self.obs = buf
            return timed(lambda: self.observe(meta=False))

        t0 = time.perf_counter()
        best = self.obs
        nbytes = max(1, best.numel())
        free_bytes, _ = torch.cuda.mem_get_info(self.device)
        budget = min(int(self._placement_gib * (1 << 30)), int(0.45 * free_bytes) + nbytes)  # (the first buffer is already ours)
        tries = max(1, int(self._placement_tries)) if 2 * nbytes <= budget else 1
        best_ms = probe(best)
        times = [best_ms]
        fill_ms = timed(lambda: best.fill_(0))
        # Once a buffer of the good cluster is in hand the search goes on for its BEST members — the cluster itself spans 5 % of the
        # render's time (round 5, plain stores: one box's two runs kept 0.2614 and 0.2497 ms = 199 and 207 M env-steps/s) and a
        # candidate costs 1.5 ms — until one is good enough, the tries are used up, or `placement_seconds` (default 3.0;
        # CTF_PLACEMENT_SECONDS) have gone by (3.3 times that, i.e. ten seconds by default, while no buffer of the fast kind has turned up at all).  (Round 3's rule — eight more tries — found a second good one 4 times in 10.)
        for _ in range(tries - 1):
            if best_ms <= good_enough * fill_ms:
                break
            elapsed = time.perf_counter() - t0
            in_hand = best_ms <= 1.08 * fill_ms  # a buffer of the fast kind (the relative test of round 3 — 7 % under the slowest seen —
                                                 # misfires on one outlier: a slow-only box stopped at 1.19 after 3.7 s)
            if (in_hand and elapsed > self._placement_seconds) or elapsed > min(10.0, 3.3 * self._placement_seconds):
                break  # (the second bound: a box that hands out slow allocations only — one in six to thirteen fresh boxes; at 50 ms a
                       # candidate ten seconds are ~200 tries, enough where one allocation in fifty is fast)
            try:
                cand = torch.empty_like(best)
            except torch.cuda.OutOfMemoryError:
                break  # (fragmentation, another process on the GPU): the best one so far is kept
            ms = probe(cand)
            times.append(ms)
            if ms < best_ms:
                best, best_ms = cand, ms
            self.obs = best
            del cand
            torch.cuda.empty_cache()  # the loser goes back to the driver now, not into torch's cache
        self.obs = best
        fill_ms = timed(lambda: best.fill_(0))  # of the buffer that is kept
        ratio = best_ms / fill_ms
        self.placement_probe_ms = times
        self.placement_fill_ms = fill_ms
        self.placement = dict(kind="fast" if ratio <= 1.08 else ("intermediate" if ratio <= 1.14 else "slow"), render_over_fill=ratio,
                              render_ms=best_ms, fill_ms=fill_ms, candidates=len(times), slowest_candidate_render_ms=max(times),
                              peak_held_bytes=min(len(times), 2) * nbytes, searched_bytes=len(times) * nbytes,
                              search_ms=(time.perf_counter() - t0) * 1e3)

    # -- plumbing -----------------------------------------------------------------------------
    def _stream(self):
        return _abi.stream_ptr(self.device)

    def _call(self, name, *args):
        """One status-returning entry point of include/ctf_env.h on this object's handle (a failure raises CtfLibraryError)."""
        _abi.call(self._lib, name, self._h, *args)

    def _reverse_bits(self, reverse_mask):
        return _abi.REVERSE_DEFAULT if reverse_mask is None else int(reverse_mask) & ((1 << self.N_AGENTS) - 1)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ctf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_dev(self, t, dtype, numel):
        torch = _torch()
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == self.device and t.dtype == dtype
                and t.is_contiguous() and t.numel() == numel):
            raise ValueError(f"expected a contiguous {dtype} tensor of {numel} elements on {self.device}")
        return _abi.ptr(t)

    # -- RNG ----------------------------------------------------------------------------------
    def seed(self, py_seeds=None, np_seeds=None):
        py = _as_seed_array(py_seeds, self.n_envs)
        npz = _as_seed_array(np_seeds if np_seeds is not None else py_seeds, self.n_envs)
        if self.rng_mode == "mt19937" and (npz >> np.uint64(32)).any():
            raise ValueError("Seed must be between 0 and 2**32 - 1")  # np.random.seed's own message
        self._call("ctf_seed", py.ctypes.data_as(C.c_void_p), npz.ctypes.data_as(C.c_void_p), self._stream())
        _torch().cuda.current_stream(self.device).synchronize()  # host seed arrays may go away

    def set_rng_state(self, env_index, py_mt625=None, np_mt625=None):
        a = None if py_mt625 is None else np.ascontiguousarray(py_mt625, dtype=np.uint32)
        b = None if np_mt625 is None else np.ascontiguousarray(np_mt625, dtype=np.uint32)
        self._call("ctf_set_rng_state", env_index, None if a is None else a.ctypes.data_as(C.c_void_p),
                   None if b is None else b.ctypes.data_as(C.c_void_p))

    def get_rng_state(self, env_index):
        a, b = np.zeros(625, np.uint32), np.zeros(625, np.uint32)
        self._call("ctf_get_rng_state", env_index, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
        return a, b

    def set_rng_states(self, py_states=None, np_states=None):
        """Bulk, stream-ordered hand-over: uint32 CUDA tensors [E, 625] (624 words + position per env), either may be None."""
        torch = _torch()
        py, np_ = (None if t is None else self._check_dev(t, torch.int32 if t.dtype == torch.int32 else torch.uint32, self.n_envs * 625)
                   for t in (py_states, np_states))
        self._call("ctf_set_rng_states", py, np_, self._stream())

    def get_rng_states(self, py=True, np_=True):
        """-> (py_states, np_states): int32 CUDA tensors [E, 625] holding the uint32 words of both generators of every env in
        the standard form (None for a generator not asked for).  Stream-ordered; no device synchronisation."""
        torch = _torch()
        a = torch.empty((self.n_envs, 625), dtype=torch.int32, device=self.device) if py else None
        b = torch.empty((self.n_envs, 625), dtype=torch.int32, device=self.device) if np_ else None
        self._call("ctf_get_rng_states", _abi.ptr(a), _abi.ptr(b), self._stream())
        return a, b

    def get_rng_counters(self):
        """counter / counter_direct mode: int64 CUDA tensor [E, 2] = words consumed so far from the `random` / np.random stream of every env (the
        whole RNG state of an env there, besides its two seeds).  Stream-ordered."""
        out = _torch().empty((self.n_envs, 2), dtype=_torch().int64, device=self.device)
        self._call("ctf_get_rng_counters", _abi.ptr(out), self._stream())
        return out

    def set_rng_counters(self, counters):
        """counter / counter_direct mode: the way back (int64 CUDA tensor [E, 2]) — a checkpoint restore after ``seed``."""
        self._call("ctf_set_rng_counters", self._check_dev(counters, _torch().int64, self.n_envs * 2), self._stream())

    # -- the hot path -------------------------------------------------------------------------
    def reset(self, mask=None):
        ptr = None if mask is None else self._check_dev(mask, _torch().uint8, self.n_envs)
        self._call("ctf_reset", ptr, self._stream())

    def reset_scattered(self, mask=None, radius=1, agent_mask=None, team=None, own_side=False, seed=0, round=0, episodes=None, env_offset=0):
        """``reset`` with RANDOMISED STARTS (include/ctf_env.h, ctf_reset_scattered): the agents of ``agent_mask`` (bit i = agent i) or of
        ``team`` — neither: all — are drawn uniformly onto an open cell within Chebyshev distance ``radius`` of their start cell (or stay
        on it), one after the other so that no two share a cell; ``own_side`` keeps them no further from their own flag than from the
        other one.  Everything else is ``reset``'s: hp, flags, inventories, counters; ``perm`` and the generators stay.  The draw is
        Philox(seed; env_offset + e, round + episodes[e], agent): ``episodes`` (uint32 [E] on the device, or None) is advanced by one
        for every env of ``mask`` (uint8 [E], None = all), so a loop — or a captured graph — that passes the same arguments draws
        afresh every time.  ``radius=0`` or an empty agent mask is ``reset`` bit for bit.  One launch, stream-ordered.  The reference
        has no such reset; ``step(auto_reset=True)`` still goes to the config's start cells."""
        torch = _torch()
        agents = self._effect_mask(agent_mask, team)
        if int(radius) < 0:
            raise ValueError("radius must be >= 0")
        ptr = None if mask is None else self._check_dev(mask, torch.uint8, self.n_envs)
        ep = None if episodes is None else self._check_dev(episodes, torch.uint32, self.n_envs)
        self._call("ctf_reset_scattered", ptr, agents, min(int(radius), 0x7FFFFFFF), _abi.SCATTER_OWN_SIDE if own_side else 0, int(seed) & 0xFFFFFFFFFFFFFFFF,
                   int(round) & 0xFFFFFFFF, ep, int(env_offset) & 0xFFFFFFFF, self._stream())

    def step(self, actions, auto_reset=False, want_f64=False):
        """actions: int8 CUDA tensor [E, N].  -> (rewards float32 [E, N], done uint8 [E]) (views of
        this object's buffers).  With want_f64 the float64 rewards are also written to ``rewards64``."""
        a = self._check_dev(actions, _torch().int8, self.n_envs * self.N_AGENTS)
        self._call("ctf_step", a, _abi.ptr(self.rewards), _abi.ptr(self.rewards64 if want_f64 else None), _abi.ptr(self.done),
                   _abi.STEP_AUTO_RESET if auto_reset else 0, self._stream())
        return self.rewards, self.done

    def observe(self, reverse_mask=None, obs=True, meta=True):
        """-> (obs uint8 [E, N, C, G, G], meta float16 [E, N, 2N+6]).  ``reverse_mask`` bit i = reverse_grid
        for agent i (default: team(i) == 1, what every caller in the reference passes)."""
        self._call("ctf_observe", _abi.ptr(self.obs if obs else None), _abi.ptr(self.meta if meta else None),
                   self._reverse_bits(reverse_mask), self._stream())
        return self.obs, self.meta

    def observe_kernel(self):
        """Which kernel ``observe`` launches for this object's buffer: "k_observe_tiles" or "k_observe" (the library's own rule)."""
        return "k_observe_tiles" if self._lib.ctf_observe_kernel(self._h, _abi.ptr(self.obs)) == 1 else "k_observe"

    def step_observe_launches(self):
        """Launches ``step_observe`` makes into this object's buffer: 1 (k_step_observe) or 2 (step, then observe)."""
        return int(self._lib.ctf_step_observe_launches(self._h, _abi.ptr(self.obs)))

    def observe_stores(self):
        """"nontemporal" when ``observe`` streams this object's buffer past the caches (the tile kernel on a batch whose observations
        exceed 320 MB), else "plain"."""
        return "nontemporal" if self._lib.ctf_observe_stores_hinted(self._h, _abi.ptr(self.obs)) == 1 else "plain"

    def observe_codes(self, reverse_mask=None, codes=True, meta=True):
        """The observation in compact form -> (codes uint8 [E, N, G, G], meta float16 [E, N, 2N+6]): low 7 bits = the tile
        plane (1..C-1) that is 1 at the cell, 0 = none; bit 7 = plane 0 (own position).  ``expand_codes`` gives the planes.
        ``self.self_cells`` (uint16 [E, N]) receives the cell index of every agent's bit 7 in the same launch."""
        rm = self._reverse_bits(reverse_mask)
        if self._self_cells is None:
            self._self_cells = _torch().zeros((self.n_envs, self.N_AGENTS), dtype=_torch().int16, device=self.device)
        self._call("ctf_observe_codes", _abi.ptr(self.codes if codes else None), _abi.ptr(self.meta if meta else None),
                   _abi.ptr(self._self_cells if codes else None), rm, self._stream())
        return self.codes, self.meta

    @property
    def self_cells(self):
        """int16 [E, N]: where bit 7 sits in each agent's row of the last ``observe_codes`` (None before the first)."""
        return self._self_cells

    def step_observe(self, actions, auto_reset=False, want_f64=False, reverse_mask=None):
        """step() then observe() in one call -> (rewards, done, obs, meta)."""
        a = self._check_dev(actions, _torch().int8, self.n_envs * self.N_AGENTS)
        self._call("ctf_step_observe", a, _abi.ptr(self.rewards), _abi.ptr(self.rewards64 if want_f64 else None), _abi.ptr(self.done),
                   _abi.ptr(self.obs), _abi.ptr(self.meta), self._reverse_bits(reverse_mask), _abi.STEP_AUTO_RESET if auto_reset else 0,
                   self._stream())
        return self.rewards, self.done, self.obs, self.meta

    def host_step(self, actions=None, py_in=None, np_in=None, reverse_mask=None, rng_out=False, view=None, obs=None, meta=None):
        """ctf_host_step (a handle of ONE env): everything in host memory, one round trip to the device.  actions: int8 numpy [N]
        or None (no step); py_in / np_in: uint32 numpy [625] to install before the step; -> (rewards float64 [N], done, status
        bits, view, py_out, np_out) with obs (uint8 [N, C, G, G]) and meta (float16 [N, M]) filled in place when given."""
        n = self.N_AGENTS
        ptr = lambda a: None if a is None else a.__array_interface__["data"][0]  # (the plain address: a third of the cost of ctypes.data_as)
        rewards = np.zeros(n, np.float64)
        done, status = C.c_int32(0), C.c_uint32(0)
        view = view if view is not None else _abi.CtfStateView()
        py_out = np.empty(625, np.uint32) if rng_out else None
        np_out = np.empty(625, np.uint32) if rng_out else None
        self._call("ctf_host_step", ptr(actions), ptr(py_in), ptr(np_in), self._reverse_bits(reverse_mask), 0, ptr(rewards), C.byref(done),
                   C.byref(status), C.byref(view), ptr(py_out), ptr(np_out), ptr(obs), ptr(meta), self._stream())
        return rewards, bool(done.value), status.value, view, py_out, np_out

    def random_actions(self, out, seed, step, env_offset=0):
        """Fill ``out`` (int8 [E, N]) with the synthetic Philox action stream of bench.py / the tests."""
        a = self._check_dev(out, _torch().int8, self.n_envs * self.N_AGENTS)
        self._call("ctf_random_actions", a, int(seed), int(step), int(env_offset), self._stream())
        return out

    def team_mask(self, team):
        """The agent mask (bit i = agent i) of one team's agents."""
        return sum(1 << i for i in range(self.N_AGENTS) if self.AGENT_TEAMS[i] == int(team))

    def scripted_actions(self, agent_mask=None, team=None, out=None, epsilon=0.0, seed=0, step=None, kind="runner", env_offset=0):
        """The scripted baseline's ENV actions (include/ctf_env.h, ctf_scripted_actions), computed on the device from the env state, for
        the agents of ``agent_mask`` (bit i = agent i) or of ``team`` — exactly one of the two.  Written into ``out`` (int8 [E, N]) in
        place: only the selected agents' bytes, every other byte is left alone, so a caller fills in its own agents' actions and the
        bot the rest.  ``out=None`` uses a buffer this object owns (zero where never written).  The actions go to ``step`` as they are:
        they are not view actions, nothing maps them through the flip.  ``epsilon``: probability of a uniform move on 0..4 instead,
        drawn from Philox(seed; env_offset + e, step, agent); 0 is the deterministic bot.  ``step=None`` counts this object's calls that
        left it to None (0, 1, 2, ...).  One launch, stream-ordered; the env's state and generators are only read / not touched."""
        if kind not in _abi.SCRIPT_KINDS:
            raise ValueError(f"kind must be one of {sorted(_abi.SCRIPT_KINDS)}")
        return self._scripted("ctf_scripted_actions", _abi.SCRIPT_KINDS[kind], agent_mask, team, out, epsilon, seed, step, env_offset)

    def role_pack(self, roles):
        """``roles`` — a sequence of N names of _abi.SCRIPT_ROLES, or a dict agent -> name (the rest are runners) — as
        ctf_scripted_roles' role_pack: nibble i is agent i's role."""
        n = self.N_AGENTS
        if isinstance(roles, dict):
            if any(not isinstance(i, int) or not 0 <= i < n for i in roles):
                raise ValueError(f"roles names an agent outside 0..{n - 1}")
            names = [roles.get(i, "runner") for i in range(n)]
        else:
            names = list(roles)
            if len(names) != n:
                raise ValueError(f"roles must name {n} agents")
        if any(name not in _abi.SCRIPT_ROLES for name in names):
            raise ValueError(f"a role must be one of {sorted(_abi.SCRIPT_ROLES)}")
        return sum(_abi.SCRIPT_ROLES[name] << (4 * i) for i, name in enumerate(names))

    def scripted_roles(self, roles, agent_mask=None, team=None, out=None, epsilon=0.0, seed=0, step=None, env_offset=0):
        """``scripted_actions`` with a ROLE per agent (include/ctf_env.h, ctf_scripted_roles): "runner" heads for the flag, "chaser"
        for the opponent nearest by path until it stands within tagging reach of one, "guard" for an opponent that carries a flag
        or has come within 3 cells of its own flag, and waits next to that flag otherwise.  ``roles``: a sequence of N names, or a
        dict agent -> name with the rest runners; the roles of agents outside ``agent_mask`` / ``team`` are not used.  Everything
        else is ``scripted_actions``'."""
        return self._scripted("ctf_scripted_roles", self.role_pack(roles), agent_mask, team, out, epsilon, seed, step, env_offset)

    def ability_mask(self, abilities):
        """``abilities`` — None (every agent), a bit mask or a sequence of agent indices — as ctf_scripted_abilities' ability_mask."""
        n = self.N_AGENTS
        if abilities is None:
            return (1 << n) - 1
        if isinstance(abilities, (int, np.integer)) and not isinstance(abilities, bool):
            mask = int(abilities)
        else:
            idx = list(abilities)
            if any(isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= int(i) < n for i in idx):
                raise ValueError(f"abilities names an agent outside 0..{n - 1}")
            mask = sum(1 << int(i) for i in set(idx))
        if mask < 0 or mask >> n:
            raise ValueError(f"abilities 0x{mask:x} names an agent outside 0..{n - 1}")
        return mask

    def scripted_abilities(self, roles, abilities=None, agent_mask=None, team=None, out=None, epsilon=0.0, seed=0, step=None, env_offset=0):
        """``scripted_roles`` for agents that use their TYPE (include/ctf_env.h, ctf_scripted_abilities): an agent named by
        ``abilities`` — None: every asked agent; a bit mask; a sequence of agent indices — plans with its type's movement ability.  A
        miner (type 3) digs: destructible tiles are passable at the cost of the hits they take, and moving into one is the mining
        action.  A vaulter (type 2) whose hp permits a jump now plans with the jumps 5..8 as well.  Every other agent moves as
        ``scripted_roles`` moves it, byte for byte.  Everything else is ``scripted_roles``'."""
        return self._scripted("ctf_scripted_abilities", (self.role_pack(roles), self.ability_mask(abilities)), agent_mask, team, out, epsilon, seed,
                              step, env_offset)

    def scripted_costs(self, roles=None, abilities=False, agent_mask=None, team=None, out=None):
        """The scripted planners' cost-to-go (include/ctf_env.h, ctf_scripted_costs) -> int16 [E, N]: for the agents of ``agent_mask``
        or of ``team`` — exactly one of the two — the cost of reaching the goal set the scripted planner of that role heads for,
        under the rules it moves by: 0 when the agent stands in the goal set or is decided before the search, the number of steps
        the planner needs if nothing else moves otherwise, ``_abi.COST_NONE`` (-1) when there is no way.  ``roles``: as for
        ``scripted_roles``; None: all runners.  ``abilities`` follows ``ScriptedPolicy``: False (everybody walks), True (every agent
        plans with its type's ability), a bit mask or a sequence of agent indices.  Only the asked agents' entries of ``out`` are
        written, in place; ``out=None`` uses a buffer this object owns (zero where never written).  One launch, stream-ordered; no
        exploration, no seed: a function of the state, which is only read."""
        torch = _torch()
        pack = 0 if roles is None else self.role_pack(roles)
        abil = 0 if abilities is False else self.ability_mask(None if abilities is True else abilities)
        if (agent_mask is None) == (team is None):
            raise ValueError("give agent_mask or team (one of them)")
        if team is not None and int(team) not in (0, 1):
            raise ValueError("team must be 0 or 1")
        mask = int(agent_mask) if team is None else self.team_mask(team)
        if mask < 0 or mask >> self.N_AGENTS:
            raise ValueError(f"agent_mask 0x{mask:x} names an agent outside 0..{self.N_AGENTS - 1}")
        if out is None:
            if getattr(self, "_costs_out", None) is None:
                self._costs_out = torch.zeros((self.n_envs, self.N_AGENTS), dtype=torch.int16, device=self.device)
            out = self._costs_out
        c = self._check_dev(out, torch.int16, self.n_envs * self.N_AGENTS)
        self._call("ctf_scripted_costs", c, mask, pack, abil, self._stream())
        return out

    def _effect_mask(self, agent_mask, team):
        """the agents of ``agent_mask`` or of ``team``; neither: all agents"""
        if agent_mask is not None and team is not None:
            raise ValueError("give agent_mask or team, not both")
        if team is not None and int(team) not in (0, 1):
            raise ValueError("team must be 0 or 1")
        mask = (1 << self.N_AGENTS) - 1 if agent_mask is None and team is None else int(agent_mask) if team is None else self.team_mask(team)
        if mask < 0 or mask >> self.N_AGENTS:
            raise ValueError(f"agent_mask 0x{mask:x} names an agent outside 0..{self.N_AGENTS - 1}")
        return mask

    def effective_actions(self, agent_mask=None, team=None, out=None):
        """Which actions do anything in the state as it stands (include/ctf_env.h, ctf_action_effects) -> int16 [E, N]: bit a of entry
        [e, i] is set iff action a of agent i would change something — move it, pick a flag up, capture, mine, lay a block — if the
        agent acted now, before anyone else moves.  It knows walls, grid edges, other agents, an empty inventory, a vaulter's hp and
        the spawn windows; bit 4 ("stay") is never set: OR 0x10 in to keep it legal.  Inside a real step another agent may move
        first: every multi-agent action mask carries that caveat.  ``agent_mask`` (bit i = agent i) or ``team``, neither: all agents;
        only the asked agents' entries of ``out`` are written, in place; ``out=None`` uses a buffer this object owns (zero where never
        written).  One launch, stream-ordered; the env is only read.  ``effects_table`` turns the result into a bool table."""
        torch = _torch()
        mask = self._effect_mask(agent_mask, team)
        if out is None:
            if getattr(self, "_effmask_out", None) is None:
                self._effmask_out = torch.zeros((self.n_envs, self.N_AGENTS), dtype=torch.int16, device=self.device)
            out = self._effmask_out
        m = self._check_dev(out, torch.int16, self.n_envs * self.N_AGENTS)
        self._call("ctf_action_effects", m, None, mask, self._stream())
        return out

    def action_effects(self, agent_mask=None, team=None, out=None):
        """WHAT each action would do (include/ctf_env.h, ctf_action_effects) -> uint8 [E, N, 9]: entry [e, i, a] is a byte of
        ``_abi.EFF_*`` flags — MOVES, JUMPS, PICKS_UP, CAPTURES, MINES, BREAKS, LAYS — 0 when action a of agent i leaves everything as
        it is.  Arguments, write discipline and the caveat are ``effective_actions``'."""
        torch = _torch()
        mask = self._effect_mask(agent_mask, team)
        if out is None:
            if getattr(self, "_effects_out", None) is None:
                self._effects_out = torch.zeros((self.n_envs, self.N_AGENTS, _abi.N_ACTIONS), dtype=torch.uint8, device=self.device)
            out = self._effects_out
        f = self._check_dev(out, torch.uint8, self.n_envs * self.N_AGENTS * _abi.N_ACTIONS)
        self._call("ctf_action_effects", None, f, mask, self._stream())
        return out

    def random_effective_actions(self, out, seed, step, agent_mask=None, team=None, env_offset=0):
        """A uniform draw among the actions that do something (include/ctf_env.h, ctf_random_effective_actions), for the agents of
        ``agent_mask`` or of ``team`` (neither: all), written into ``out`` (int8 [E, N]) in place, the other agents' bytes left alone:
        a random walker that never bumps into a wall.  An agent none of whose actions does anything gets 4.  The draw is
        Philox(seed; env_offset + e, step, agent): the same arguments on the same state give the same actions.  ENV actions: they go
        to ``step`` as they are.  One launch, stream-ordered; the env is only read."""
        mask = self._effect_mask(agent_mask, team)
        a = self._check_dev(out, _torch().int8, self.n_envs * self.N_AGENTS)
        self._call("ctf_random_effective_actions", a, mask, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF, int(env_offset) & 0xFFFFFFFF,
                   self._stream())
        return out

    def _scripted(self, call, what, agent_mask, team, out, epsilon, seed, step, env_offset):
        """``what``: the call's own arguments between the mask and epsilon (one value or a tuple)"""
        torch = _torch()
        what = what if isinstance(what, tuple) else (what,)
        if (agent_mask is None) == (team is None):
            raise ValueError("give agent_mask or team (one of them)")
        if team is not None and int(team) not in (0, 1):
            raise ValueError("team must be 0 or 1")
        mask = int(agent_mask) if team is None else self.team_mask(team)
        if mask < 0 or mask >> self.N_AGENTS:
            raise ValueError(f"agent_mask 0x{mask:x} names an agent outside 0..{self.N_AGENTS - 1}")
        if not 0.0 <= float(epsilon) <= 1.0:
            raise ValueError("epsilon must be in [0, 1]")
        if out is None:
            if getattr(self, "_scripted_out", None) is None:
                self._scripted_out = torch.zeros((self.n_envs, self.N_AGENTS), dtype=torch.int8, device=self.device)
            out = self._scripted_out
        if step is None:
            step = getattr(self, "_scripted_calls", 0)
            self._scripted_calls = step + 1
        a = self._check_dev(out, torch.int8, self.n_envs * self.N_AGENTS)
        eps_q32 = min(int(float(epsilon) * 4294967296.0), 0xFFFFFFFF)
        self._call(call, a, mask, *what, eps_q32, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF, int(env_offset) & 0xFFFFFFFF, self._stream())
        return out

    def counters(self):
        """-> (metrics int32 [E, 13, N] in _abi.METRIC_NAMES order, team_flag_captures int32 [E, 2], env_step_count int32 [E]):
        what utils.duel / MetricsLogger.harvest_metrics read from ``env.metrics``, for every env at once."""
        torch = _torch()
        E, N = self.n_envs, self.N_AGENTS
        met = torch.empty((E, _abi.N_METRICS, N), dtype=torch.int32, device=self.device)
        caps = torch.empty((E, 2), dtype=torch.int32, device=self.device)
        steps = torch.empty((E,), dtype=torch.int32, device=self.device)
        self._call("ctf_export_counters", _abi.ptr(met), _abi.ptr(caps), _abi.ptr(steps), self._stream())
        return met, caps, steps

    def action_mask(self):
        """uint8 [N, 9]: 1 where the action is legal for the agent's type (agent_network.py:66-75)."""
        m = np.zeros((self.N_AGENTS, _abi.N_ACTIONS), np.uint8)
        self._call("ctf_action_mask", m.ctypes.data_as(C.c_void_p))
        return m

    # -- snapshots: whole env states as opaque device records (include/ctf_env.h, ctf_save_states) ---------------------------
    # Records are valid for any handle of the same ``fingerprint`` (same kwargs, rng_mode and log_metrics; any n_envs, seeds or
    # device), across processes (torch.save / torch.load of the buffer).  Not for the drop-in ``GridworldCtf``: it caches the
    # generator states of its env (_py_last / _np_last), so ``load_states`` on a facade's ``_vec`` is unsupported.
    @property
    def snapshot_bytes(self):
        """S: bytes of one env's record (a multiple of 256; depends on the config only)."""
        return int(self._lib.ctf_snapshot_bytes(self._h))

    @property
    def fingerprint(self):
        """64-bit fingerprint of the config: records move between handles whose fingerprints are equal."""
        return int(self._lib.ctf_snapshot_fingerprint(self._h))

    def _index_list(self, idx, what, check):
        """idx (None, int tensor, numpy array or sequence) -> (int32 tensor on the device or None, n).  Host inputs are checked
        for range here (free); device tensors only when ``check`` (one synchronisation)."""
        torch = _torch()
        if idx is None:
            return None, self.n_envs
        if isinstance(idx, torch.Tensor):
            if idx.dtype.is_floating_point or idx.dtype.is_complex or idx.dtype == torch.bool or idx.dim() != 1:
                raise ValueError(f"{what}: expected a 1-D integer index tensor")
            host = not idx.is_cuda
        else:
            arr = np.asarray(idx)
            if arr.ndim != 1 or not np.issubdtype(arr.dtype, np.integer):
                raise ValueError(f"{what}: expected a 1-D integer index array")
            idx, host = torch.from_numpy(np.ascontiguousarray(arr)), True
        if host or check:
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.n_envs):
                raise ValueError(f"{what}: an index is outside [0, {self.n_envs})")
        elif idx.device != self.device:
            raise ValueError(f"{what}: index tensor on {idx.device}, the envs are on {self.device}")
        idx = idx.to(device=self.device, dtype=torch.int32).contiguous()
        return idx, int(idx.numel())

    def _records(self, buf, n, what):
        torch = _torch()
        S = self.snapshot_bytes
        if not (isinstance(buf, torch.Tensor) and buf.dtype == torch.uint8 and buf.is_cuda and buf.device == self.device):
            raise ValueError(f"{what}: expected a uint8 tensor on {self.device}")
        if buf.dim() != 2 or buf.shape[1] != S or (n is not None and buf.shape[0] != n):
            raise ValueError(f"{what}: expected shape [{'n' if n is None else n}, {S}], got {list(buf.shape)}")
        if not buf.is_contiguous() or buf.data_ptr() % 16:
            raise ValueError(f"{what}: the record buffer must be contiguous and 16-byte aligned")
        return _abi.ptr(buf)

    def save_states(self, idx=None, out=None):
        """Records of envs ``idx`` (None: all) -> uint8 [n, snapshot_bytes] on the env's device (``out`` if given).  Stream-ordered:
        no synchronisation; repeats allowed."""
        torch = _torch()
        ix, n = self._index_list(idx, "save_states", check=False)
        if out is None:
            out = torch.empty((n, self.snapshot_bytes), dtype=torch.uint8, device=self.device)
        ptr = self._records(out, n, "save_states")
        self._call("ctf_save_states", _abi.ptr(ix), n, ptr, self._stream())
        return out

    def load_states(self, buf, idx=None, check=True):
        """Env ``idx[k]`` := record ``buf[k]`` (idx None: envs 0..n-1).  Observations are not state: call ``observe`` afterwards.
        ``check`` rejects repeated or out-of-range indices (one synchronisation); ``check=False`` skips that (graph capture) —
        the kernel still refuses a record whose header does not match this handle, or an index outside [0, E): that env is left
        as it was and ``status()`` shows ST_BAD_SNAPSHOT."""
        torch = _torch()
        n = buf.shape[0] if isinstance(buf, torch.Tensor) and buf.dim() == 2 else None
        ptr = self._records(buf, n, "load_states")
        n = int(buf.shape[0])
        if n > self.n_envs:
            raise ValueError(f"load_states: {n} records for {self.n_envs} envs")
        ix, m = (None, n) if idx is None else self._index_list(idx, "load_states", check)
        if m != n:
            raise ValueError(f"load_states: {n} records but {m} indices")
        if check and ix is not None and torch.unique(ix).numel() != n:
            raise ValueError("load_states: repeated indices")
        self._call("ctf_load_states", ptr, _abi.ptr(ix), n, self._stream())

    def clone_envs(self, src_idx, dst_idx, check=True):
        """Env ``dst_idx[k]`` := the state of env ``src_idx[k]`` (through a scratch buffer this object owns, so the two sets may
        overlap: a permutation in place is legal).  Stream-ordered apart from ``check`` (see ``load_states``)."""
        src, n = self._index_list(src_idx, "clone_envs", check)
        scratch = getattr(self, "_clone_scratch", None)
        if scratch is None or scratch.shape[0] < n:
            scratch = self._clone_scratch = _torch().empty((n, self.snapshot_bytes), dtype=_torch().uint8, device=self.device)
        recs = self.save_states(src, out=scratch[:n])
        self.load_states(recs, dst_idx, check=check)

    # -- harvest of finished episodes into per-group results (include/ctf_env.h, ctf_harvest_episodes) ------------------------
    @property
    def harvest_words(self):
        """H = 8 + 13 * N: int64 words of one group's row of a harvest table."""
        return int(self._lib.ctf_harvest_words(self._h))

    def harvest(self, acc, groups=None, mask=None, all_envs=False):
        """ADD the results of the envs whose episode ended in the most recent step (``done`` set and ``env_step_count ==
        GAME_STEPS``; with ``all_envs`` every env as it stands) into ``acc``, int64 [n_groups, harvest_words] on the envs'
        device: row ``groups[e]`` (int32 [E]; None: row 0) receives env e.  ``mask`` (uint8 [E]): only envs whose byte is
        non-zero.  One stream-ordered launch; call it once after every step (``harvest.EpisodeHarvest`` owns a table and does).
        A group id outside [0, n_groups) skips that env and ``status()`` shows ST_BAD_GROUP."""
        torch = _torch()
        H = self.harvest_words
        if not (isinstance(acc, torch.Tensor) and acc.dtype == torch.int64 and acc.is_cuda and acc.device == self.device):
            raise ValueError(f"harvest: expected an int64 table on {self.device}")
        if acc.dim() != 2 or acc.shape[0] < 1 or acc.shape[1] != H or not acc.is_contiguous():
            raise ValueError(f"harvest: expected a contiguous table of shape [n_groups >= 1, {H}], got {list(acc.shape)}")
        g = None if groups is None else self._check_dev(groups, torch.int32, self.n_envs)
        m = None if mask is None else self._check_dev(mask, torch.uint8, self.n_envs)
        self._call("ctf_harvest_episodes", g, int(acc.shape[0]), m, _abi.HARVEST_ALL if all_envs else 0, _abi.ptr(acc), self._stream())
        return acc

    # -- visitation maps in bulk (include/ctf_env.h, ctf_harvest_visitation / ctf_export_visitation) --------------------------
    @property
    def visitation_words(self):
        """N * G * G: words of one env's (or one group's) visitation maps."""
        return int(self._lib.ctf_visitation_words(self._h))

    def harvest_visitation(self, acc, groups=None, mask=None, all_envs=False):
        """ADD the visitation maps (true counts: no u8 wrap) of the envs ``harvest`` takes under the same arguments into ``acc``,
        int64 [n_groups, N, G, G] on the envs' device.  One stream-ordered launch; behind the same step it covers exactly the
        episodes ``harvest`` covers.  Needs ``log_metrics=True``."""
        torch = _torch()
        N, G = self.N_AGENTS, self.GRID_SIZE
        if not (isinstance(acc, torch.Tensor) and acc.dtype == torch.int64 and acc.is_cuda and acc.device == self.device):
            raise ValueError(f"harvest_visitation: expected an int64 table on {self.device}")
        if acc.dim() != 4 or acc.shape[0] < 1 or tuple(acc.shape[1:]) != (N, G, G) or not acc.is_contiguous():
            raise ValueError(f"harvest_visitation: expected a contiguous table of shape [n_groups >= 1, {N}, {G}, {G}], got {list(acc.shape)}")
        if not self.cfg.log_metrics:
            raise ValueError("harvest_visitation: the envs keep no visitation maps (log_metrics=False)")
        g = None if groups is None else self._check_dev(groups, torch.int32, self.n_envs)
        m = None if mask is None else self._check_dev(mask, torch.uint8, self.n_envs)
        self._call("ctf_harvest_visitation", g, int(acc.shape[0]), m, _abi.HARVEST_ALL if all_envs else 0, _abi.ptr(acc), self._stream())
        return acc

    def visitation(self, idx=None, out=None):
        """Visitation maps of envs ``idx`` (None: all) -> uint32 [n, N, G, G] on the envs' device (``out`` if given): true counts,
        ``& 0xFF`` is ``metrics['agent_visitation_maps']``.  One stream-ordered launch, repeats allowed.  Host index lists are
        range-checked here; a device list is not (no synchronisation): an index outside [0, n_envs) leaves its record unwritten and
        ``status()`` shows ST_BAD_GROUP."""
        torch = _torch()
        N, G = self.N_AGENTS, self.GRID_SIZE
        if not self.cfg.log_metrics:
            raise ValueError("visitation: the envs keep no visitation maps (log_metrics=False)")
        ix, n = self._index_list(idx, "visitation", check=False)
        if out is None:
            out = torch.empty((n, N, G, G), dtype=torch.uint32, device=self.device)
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint32 and out.is_cuda and out.device == self.device):
            raise ValueError(f"visitation: expected a uint32 output on {self.device}")
        if tuple(out.shape) != (n, N, G, G) or not out.is_contiguous():
            raise ValueError(f"visitation: expected a contiguous output of shape [{n}, {N}, {G}, {G}], got {list(out.shape)}")
        self._call("ctf_export_visitation", _abi.ptr(ix), n, _abi.ptr(out), self._stream())
        return out

    # -- env states as plain arrays, in bulk (include/ctf_env.h, ctf_export_states / ctf_import_states) -----------------------------
    def _state_specs(self):
        """name -> (dtype, shape of one record) of every member of ctf_state_arrays"""
        torch = _torch()
        N, G = self.N_AGENTS, self.GRID_SIZE
        return dict(grid=(torch.uint8, (G, G)), pos=(torch.int8, (N, 2)), hp=(torch.float64, (N,)), has_flag=(torch.uint8, (N,)),
                    inventory=(torch.int32, (N,)), perm=(torch.uint8, (N,)), step_count=(torch.int32, ()),
                    team_captures=(torch.int32, (2,)), done=(torch.uint8, ()), metrics=(torch.int32, (_abi.N_METRICS, N)),
                    visitation=(torch.uint8, (N, G, G)))

    def _state_arrays(self, tensors, n, what):
        """dict name -> tensor, validated against the specs -> the struct of device pointers"""
        torch = _torch()
        specs = self._state_specs()
        arrs = _abi.CtfStateArrays()
        for name, t in tensors.items():
            dtype, tail = specs[name]
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == self.device and t.dtype == dtype):
                raise ValueError(f"{what}: {name} must be a {dtype} tensor on {self.device}")
            if tuple(t.shape) != (n,) + tail:
                raise ValueError(f"{what}: {name} must have shape {[n] + list(tail)}, got {list(t.shape)}")
            if not t.is_contiguous() or t.data_ptr() % 16:
                raise ValueError(f"{what}: {name} must be contiguous and 16-byte aligned")
            setattr(arrs, name, t.data_ptr())
        return arrs

    def get_states(self, idx=None, fields=None, out=None):
        """The readable state of envs ``idx`` (None: all) as a dict of tensors on the envs' device, record k = what ``get_state(idx[k])``
        shows, bit for bit: grid uint8 [n, G, G], pos int8 [n, N, 2], hp float64 [n, N], has_flag uint8 [n, N], inventory int32 [n, N],
        perm uint8 [n, N], step_count int32 [n], team_captures int32 [n, 2], done uint8 [n] and, with ``log_metrics``, metrics int32
        [n, 13, N].  ``fields`` selects a subset (only those are written); ``out`` is a dict to reuse: its tensors of the selected
        names are written in place, missing ones are allocated and added.  One stream-ordered launch, repeats allowed.  Host index
        lists are range-checked here; a device list is not (no synchronisation): an index outside [0, n_envs) leaves its record
        unwritten and ``status()`` shows ST_BAD_GROUP.  The visitation maps have their own export, ``visitation()``."""
        torch = _torch()
        specs = self._state_specs()
        exportable = [f for f in _abi.STATE_FIELDS[:-1] if f != "metrics" or self.cfg.log_metrics]
        names = exportable if fields is None else list(fields)
        for f in names:
            if f == "visitation":
                raise ValueError("get_states: the visitation maps are exported by visitation()")
            if f not in specs:
                raise ValueError(f"get_states: unknown field {f!r}")
            if f == "metrics" and not self.cfg.log_metrics:
                raise ValueError("get_states: the envs keep no counters (log_metrics=False)")
        ix, n = self._index_list(idx, "get_states", check=False)
        out = {} if out is None else out
        for f in names:
            if f not in out:
                out[f] = torch.empty((n,) + specs[f][1], dtype=specs[f][0], device=self.device)
        arrs = self._state_arrays({f: out[f] for f in names}, n, "get_states")
        if n and names:
            self._call("ctf_export_states", _abi.ptr(ix), n, C.byref(arrs), self._stream())
        return out

    def set_states(self, states, idx=None, check=True):
        """Env ``idx[k]`` := record k of ``states`` (idx None: envs 0..n-1): ``set_state`` for many envs in one stream-ordered launch.
        ``states`` is a dict as ``get_states`` returns it; every field but ``metrics`` (missing: zeros) and ``visitation`` (uint8 [n, N,
        G, G], the base maps; missing: the maps restart as after ``reset()``) is required.  ``check`` rejects repeated or out-of-range
        indices (one synchronisation for a device list); with ``check=False`` the kernel still refuses a record that breaks one of
        ``set_state``'s rules or names no env: that env is left as it was and ``status()`` shows ST_BAD_STATE.  The generators are not
        touched; observations are not state: call ``observe`` afterwards."""
        torch = _torch()
        specs = self._state_specs()
        if not isinstance(states, dict):
            raise ValueError("set_states: expected a dict of tensors")
        for f in states:
            if f not in specs:
                raise ValueError(f"set_states: unknown field {f!r}")
        for f in _abi.STATE_FIELDS[:-2]:
            if states.get(f) is None:
                raise ValueError(f"set_states: {f} is required")
        given = {f: t for f, t in states.items() if t is not None}
        if not self.cfg.log_metrics and ("metrics" in given or "visitation" in given):
            raise ValueError("set_states: the envs keep no counters or visitation maps (log_metrics=False)")
        first = given["step_count"]
        n = int(first.shape[0]) if isinstance(first, torch.Tensor) and first.dim() == 1 else -1
        if n < 0:
            raise ValueError("set_states: step_count must be an int32 tensor of shape [n]")
        if n > self.n_envs:
            raise ValueError(f"set_states: {n} records for {self.n_envs} envs")
        arrs = self._state_arrays(given, n, "set_states")
        ix, m = (None, n) if idx is None else self._index_list(idx, "set_states", check)
        if m != n:
            raise ValueError(f"set_states: {n} records but {m} indices")
        if check and ix is not None and torch.unique(ix).numel() != n:
            raise ValueError("set_states: repeated indices")
        if n:
            self._call("ctf_import_states", C.byref(arrs), _abi.ptr(ix), n, self._stream())

    # -- host views ---------------------------------------------------------------------------
    def get_state(self, env_index):
        v = _abi.CtfStateView()
        self._call("ctf_get_state", int(env_index), C.byref(v))
        return v

    def set_state(self, env_index, view):
        self._call("ctf_set_state", int(env_index), C.byref(view))

    def status(self):
        bits = C.c_uint32(0)
        self._call("ctf_status", C.byref(bits), self._stream())
        return bits.value


def effects_table(mask):
    """``effective_actions``' masks (a tensor or an array of integers, any shape) -> bool [..., 9]: entry a = bit a of the mask, for
    callers that mask logits (``logits.masked_fill(~table, -inf)``; OR 0x10 into the mask first to keep "stay" legal)."""
    if isinstance(mask, np.ndarray) or not hasattr(mask, "device"):
        m = np.asarray(mask).astype(np.int64)
        return ((m[..., None] >> np.arange(_abi.N_ACTIONS)) & 1).astype(bool)
    torch = _torch()
    bits = torch.arange(_abi.N_ACTIONS, device=mask.device, dtype=torch.int32)
    return ((mask.to(torch.int32).unsqueeze(-1) >> bits) & 1).to(torch.bool)


def metrics_from_counters(counters, team_captures, agent_teams, agent_types, n_agents):
    """The reference's metrics dict (gridworld_ctf.py:425-470) without the visitation maps, from agent-level counters
    ``counters[k][i]`` (k in _abi.METRIC_NAMES order) and ``team_captures[t]``: the team_* and agent_type_* entries are sums of
    the agent-level counters, as in the reference.  One env's counters (``GridworldCtf.metrics``) or sums over many episodes
    (``harvest.EpisodeHarvest.metrics``)."""
    out = {"team_wins": {0: 0, 1: 0}}
    for k, name in enumerate(_abi.METRIC_NAMES):
        team = {0: 0, 1: 0}
        by_type = defaultdict(partial(defaultdict, int))
        agent = defaultdict(int)
        for i in range(n_agents):
            val = int(counters[k][i])
            if val:
                agent[i] = val
                team[agent_teams[i]] += val
                by_type[agent_teams[i]][agent_types[i]] += val
        out["team_" + name], out["agent_type_" + name], out["agent_" + name] = team, by_type, agent
    out["team_flag_captures"] = {0: int(team_captures[0]), 1: int(team_captures[1])}
    return out


# ----------------------------------------------------------------------------------------------
# the reference's single-env API
# ----------------------------------------------------------------------------------------------
# REVERSED_ACTION_MAP (gridworld_ctf.py:147-196) written as permutations of 0..8:
#   None: both axes flipped, 0: rows flipped, 1: columns flipped, 2: anti-diagonal reflection
_REVERSED_ACTIONS = {
    None: (1, 0, 3, 2, 4, 6, 5, 8, 7),
    0: (1, 0, 2, 3, 4, 6, 5, 7, 8),
    1: (0, 1, 3, 2, 4, 5, 6, 8, 7),
    2: (2, 3, 0, 1, 4, 7, 8, 5, 6),
}
_UNIT_MOVES = ((-1, 0), (1, 0), (0, 1), (0, -1), (0, 0))


def _action_deltas():
    table = {}
    for typ, reach in ((0, 0), (1, 0), (2, 2), (3, 1)):  # scout, guardian, vaulter (jumps 2), miner (acts at 1)
        table[typ] = {a: _UNIT_MOVES[a] for a in range(5)}
        for a in range(5, 9):
            dr, dc = _UNIT_MOVES[a - 5]
            table[typ][a] = (dr * reach, dc * reach)
    return table


class GridworldCtf:
    """Drop-in for the reference class, backed by the HIP kernels (a batch of one env).

    ``rng="global"`` (default) keeps the reference's RNG contract exactly: every ``step`` consumes
    from the process-global ``random`` and ``np.random`` generators (their MT19937 states are handed
    to the device before the step and written back after it), so ``random.seed(s); np.random.seed(s)``
    in the caller has the effect it has on the reference.  ``rng="device"`` keeps private streams on
    the device (seeded with ``seed=``) and avoids the two 2.5 KB transfers per step.
    """

    def __init__(self, rng="global", seed=0, device=None, **kwargs):
        self._ctor = dict(rng=rng, seed=seed, device=device, kwargs=dict(kwargs))
        self._vec = VecGridworldCtf(1, device=device, py_seeds=[seed], np_seeds=[seed], **kwargs)
        self._rng_mode = rng
        d = self._vec.derived
        kw = d["kwargs"]
        # attributes the reference exposes (gridworld_ctf.py:58-290)
        self.AGENT_CONFIG, self.SCENARIO = kw["AGENT_CONFIG"], kw["SCENARIO"]
        self.GAME_STEPS = kw["GAME_STEPS"]
        self.ENABLE_OBSTACLES, self.DROP_FLAG_WHEN_NO_HP = kw["ENABLE_OBSTACLES"], kw["DROP_FLAG_WHEN_NO_HP"]
        self.HOME_FLAG_CAPTURE, self.USE_EASY_CAPTURE = kw["HOME_FLAG_CAPTURE"], kw["USE_EASY_CAPTURE"]
        self.USE_ADJUSTED_REWARDS, self.MAX_BLOCK_TILE_PCT = kw["USE_ADJUSTED_REWARDS"], kw["MAX_BLOCK_TILE_PCT"]
        self.LOG_METRICS, self.MAP_SYMMETRY_CHECK = kw["LOG_METRICS"], kw["MAP_SYMMETRY_CHECK"]
        self.N_AGENTS = d["n_agents"]
        self.ACTION_SPACE = 8
        self.ENV_DIMS = (1, 1, kw["GRID_SIZE"], kw["GRID_SIZE"])
        self.WIN_MARGIN_SCALAR, self.LOSS_MARGIN_SCALAR = 0.1, 0.00
        self.REWARD_CAPTURE, self.REWARD_STEP, self.REWARD_TAG = 1, 0, 0.0
        self.OPP_FLAG_CAPTURE_PUNISHMENT_SCALAR = 0.5
        self.WINNING_POINTS = np.inf
        self.DEFENSIVE_ZONE_DISTANCE = 3
        self.ACTION_DELTAS = _action_deltas()
        self.REVERSED_ACTION_MAP = {k: dict(enumerate(v)) for k, v in _REVERSED_ACTIONS.items()}
        self.AGENT_TEAMS, self.AGENT_TYPES = d["agent_teams"], d["agent_types"]
        self.AGENT_TYPE_HP, self.AGENT_HP_HEALING_PER_STEP = kw["AGENT_TYPE_HP"], kw["AGENT_HP_HEALING_PER_STEP"]
        self.AGENT_TYPE_DAMAGE = kw["AGENT_TYPE_DAMAGE"]
        self.AGENT_TYPE_ACTION_MASK = {0: 1, 1: 1, 2: 0, 3: 0}
        self.GUARDIAN_DEFENSE_DISTANCE, self.GUARDIAN_TAGGING_RANGE = 3, 1
        self.GUARDIAN_DAMAGE_MULTIPLIER, self.TAG_PROBABILITY = kw["GUARDIAN_DAMAGE_MULTIPLIER"], kw["TAG_PROBABILITY"]
        self.VAULT_HP_COST, self.VAULT_MIN_HP = kw["VAULT_HP_COST"], kw["VAULT_MIN_HP"]
        self.AGENT_FLAG_CAPTURE_TYPES = [0, 1, 2, 3]
        self.MAX_AGENT_BLOCKS = 1000
        self.OPEN_TILE, self.BLOCK_TILE, self.DESTRUCTIBLE_TILE1, self.DESTRUCTIBLE_TILE2 = 0, 1, 2, 3
        self.AGENT_TYPE_TILE_MAP = _config.AGENT_TYPE_TILE_MAP
        self.AGENT_TILE_MAP = d["agent_tile_map"]
        self.FLAG_TILE_MAP = dict(_config.FLAG_TILE_MAP)
        self.STD_OWN_FLAG_TILE, self.STD_OPP_FLAG_TILE = 12, 13
        s = kw["SCENARIO"]
        self.SCENARIO_NAME, self.FLIP_AXIS, self.GRID_SIZE = s["SCENARIO_NAME"], s["FLIP_AXIS"], s["GRID_SIZE"]
        self.FLAG_POSITIONS, self.CAPTURE_POSITIONS = s["FLAG_POSITIONS"], s["CAPTURE_POSITIONS"]
        self.SPAWN_POSITIONS, self.AGENT_STARTING_POSITIONS = s["SPAWN_POSITIONS"], s["AGENT_STARTING_POSITIONS"]
        self.OPPONENTS = d["opponents"]
        self.TILES_USED = d["tiles_used"]
        self.agent_teams_np = np.array([v for v in self.AGENT_TEAMS.values()], dtype=np.uint8)
        self.grid = np.zeros((self.GRID_SIZE, self.GRID_SIZE), dtype=np.uint8)  # live array, updated in place
        self.has_flag = np.zeros(self.N_AGENTS, dtype=np.uint8)
        self._obs_cache = None
        c, g, n = len(self.TILES_USED) + 1, self.GRID_SIZE, self.N_AGENTS
        self._obs_host = np.zeros((n, c, g, g), dtype=np.uint8)        # filled by every ctf_host_step round trip
        self._meta_host = np.zeros((n, 2 * n + 6), dtype=np.float16)
        self._rng_in = np.empty((2, 625), dtype=np.uint32)
        self._view_buf = _abi.CtfStateView()  # refilled by every round trip (the attributes below are copies taken from it)
        self._default_mask = self._default_reverse_mask()
        self._py_last = self._np_last = None  # the generator states the last step wrote back to random / np.random
        self.reset()

    # -- pickling / deepcopy (Ray hands the env to workers by value) ------------------------------
    def __getstate__(self):
        return dict(ctor=self._ctor, view=bytes(self._vec.get_state(0)), rng=self._vec.get_rng_state(0))

    def __setstate__(self, state):
        c = state["ctor"]
        self.__init__(rng=c["rng"], seed=c["seed"], device=c["device"], **c["kwargs"])
        view = _abi.CtfStateView.from_buffer_copy(state["view"])
        self._vec.set_state(0, view)
        self._vec.set_rng_state(0, *state["rng"])
        self._pull()

    def __deepcopy__(self, memo):
        new = object.__new__(type(self))
        new.__setstate__(self.__getstate__())
        return new

    # -- host mirror of the device state --------------------------------------------------------
    def _mirror(self, v):
        """The reference's attributes from a state view (the same round trip has refreshed _obs_host / _meta_host)."""
        n, g = self.N_AGENTS, self.GRID_SIZE
        self.grid[...] = np.frombuffer(v.grid, dtype=np.uint8, count=g * g).reshape(g, g)
        self.agent_positions = {i: (int(v.pos[i][0]), int(v.pos[i][1])) for i in range(n)}
        self.has_flag[...] = np.frombuffer(v.has_flag, dtype=np.uint8, count=n)
        self.agent_hp = {i: v.hp[i] for i in range(n)}
        self.block_inventory = {i: int(v.inventory[i]) for i in range(n)}
        self._arr = [int(v.perm[i]) for i in range(n)]
        self.env_step_count = int(v.step_count)
        self.done = bool(v.done)
        self._view = v
        self._obs_cache = None  # (renders under a non-default reversal; the default one is _obs_host / _meta_host, always current)

    def _pull(self):
        """State view + the default observation of the env as it is now, in one round trip (no step)."""
        _, _, _, v, _, _ = self._vec.host_step(None, view=self._view_buf, obs=self._obs_host, meta=self._meta_host)
        self._mirror(v)

    @property
    def metrics(self):
        """The reference's metrics dict (gridworld_ctf.py:425-470), rebuilt from the device counters:
        team_* and agent_type_* entries are sums of the agent-level counters, as in the reference."""
        v, n, g = self._view, self.N_AGENTS, self.GRID_SIZE
        out = metrics_from_counters(v.metrics, v.team_captures, self.AGENT_TEAMS, self.AGENT_TYPES, n)
        vis = defaultdict(partial(np.zeros, (g, g), dtype=np.uint8))
        for i in range(n):
            vis[i] = np.frombuffer(v.visitation[i], dtype=np.uint8, count=g * g).reshape(g, g).copy()
        out["agent_visitation_maps"] = vis
        return out

    # -- reference API ----------------------------------------------------------------------------
    def reset(self):
        self._vec.reset()
        self._pull()
        if self.MAP_SYMMETRY_CHECK:
            assert np.all(self.standardise_state(0) == self.standardise_state(1, reverse_grid=True))

    def action_effects(self):
        """What each action of each agent would do in the env's present state (``VecGridworldCtf.action_effects``) -> numpy uint8
        [N, 9] of ``_abi.EFF_*`` flags; 0: the action changes nothing."""
        return self._vec.action_effects()[0].cpu().numpy()

    def effective_actions(self):
        """Which actions do anything in the env's present state (``VecGridworldCtf.effective_actions``) -> numpy int16 [N]: bit a of
        entry i = action a of agent i changes something if the agent acts before anyone else moves."""
        return self._vec.effective_actions()[0].cpu().numpy()

    def _global_rng_in(self):
        """random / np.random -> the two uint32 [625] arrays (624 words + position) ctf_host_step installs before the step.
        -> (np.random's state tuple, unchanged): True when both generators are exactly where the previous step of THIS env left
        them — the device streams are then already in place and nothing needs to go over."""
        st = np.random.get_state()
        pt = _py_random.getstate()[1]
        if self._py_last is not None and pt == self._py_last and st[2] == self._np_last[1] and np.array_equal(st[1], self._np_last[0]):
            return st, True
        both = self._rng_in
        both[0] = pt
        both[1, :624] = st[1]
        both[1, 624] = st[2]
        return st, False

    def step(self, actions):
        acts = [actions[i] for i in range(self.N_AGENTS)]
        for i, a in enumerate(acts):
            if not (isinstance(a, (int, np.integer)) and 0 <= int(a) <= 8):
                raise KeyError(a)  # ACTION_DELTAS[type][action] in the reference
        glob = self._rng_mode == "global"
        st, in_place = self._global_rng_in() if glob else (None, True)
        # ONE round trip (ctf_host_step): generator states in, step, render of all N agents, state view and generator states out
        r64, _, status, v, py, npw = self._vec.host_step(np.array(acts, dtype=np.int8), None if in_place else self._rng_in[0],
                                                         None if in_place else self._rng_in[1], rng_out=glob, view=self._view_buf,
                                                         obs=self._obs_host, meta=self._meta_host)
        if glob:
            self._py_last = tuple(py.tolist())
            self._np_last = (npw[:624], int(npw[624]))
            _py_random.setstate((3, self._py_last, None))
            np.random.set_state((st[0], npw[:624], int(npw[624]), st[3], st[4]))
        self._mirror(v)
        if status & _abi.ST_NO_RESPAWN:
            raise ValueError("high <= 0")  # np.random.randint(0) in the reference's respawn
        if status & _abi.ST_SPAWN_EDGE:
            raise IndexError("respawn window clipped at row/col 0: the reference misplaces the agent here")
        return self.grid, r64.tolist(), self.done

    def _observe(self, reverse_mask):
        if reverse_mask == self._default_mask:
            return reverse_mask, self._obs_host, self._meta_host
        if self._obs_cache is None or self._obs_cache[0] != reverse_mask:  # a non-default reversal: its own render
            obs, meta = self._vec.observe(reverse_mask)
            self._obs_cache = (reverse_mask, obs[0].cpu().numpy(), meta[0].cpu().numpy())
        return self._obs_cache

    def _default_reverse_mask(self):
        return sum(1 << i for i in range(self.N_AGENTS) if self.AGENT_TEAMS[i] == 1)

    def standardise_state(self, agent_idx, reverse_grid=False):
        i = int(agent_idx)
        mask = self._default_mask
        if bool(reverse_grid) != bool((mask >> i) & 1):
            mask ^= 1 << i
        return self._observe(mask)[1][i][None].copy()

    def get_env_metadata(self, agent_idx):
        for t in self.AGENT_TYPES.values():
            if t not in self.agent_hp:
                raise KeyError(t)  # the reference indexes agent_hp by type id (gridworld_ctf.py:1041)
        return self._meta_host[int(agent_idx)][None].copy()  # (the metadata rows do not depend on the reversal)

    def get_env_dims(self):
        c, g, n = len(self.TILES_USED) + 1, self.GRID_SIZE, self.N_AGENTS
        return (c, g, g), (c - 1, g, g), (n * 2 + 6,), (n * 6 + n * self.ACTION_SPACE + 3,)

    def get_reversed_action(self, action):
        return self.REVERSED_ACTION_MAP[self.FLIP_AXIS][action]

    def get_tiles_used(self):
        return list(self.TILES_USED)

    def max_dim_distance_to_xy(self, xy, target_xy):
        return max(abs(xy[0] - target_xy[0]), abs(xy[1] - target_xy[1]))

    def agent_distance_to_xy(self, agent_idx, object_xy):
        return self.max_dim_distance_to_xy(self.agent_positions[agent_idx], object_xy)

    def render(self, sleep_time=0.2, ego_state_agent=None):
        """Minimal matplotlib view of the grid (presentation is outside the accelerated path)."""
        import matplotlib.pyplot as plt

        plt.figure(num="env_render")
        plt.clf()
        plt.imshow(self.grid, vmin=0, vmax=13, cmap="tab20")
        plt.title(f"step {self.env_step_count}")
        plt.pause(sleep_time)

    @staticmethod
    def render_indices(grid, agent_positions, has_flag, agent_teams, flag_positions):
        """The sprite index of every cell as the reference's ``render_image`` chooses it (gridworld_ctf.py:1130-1154): the
        tile code; 112 / 113 at a team's home flag cell while the OTHER team carries that flag; + 100 for an agent that
        carries a flag.  Pure function of the host-side state (tested without a GPU)."""
        idx = np.array(grid, dtype=np.int32)
        teams_with_flag = {0: 0, 1: 0}
        for a, flag in enumerate(has_flag):
            if flag == 1:
                teams_with_flag[agent_teams[a]] = 1
        if teams_with_flag[1] == 1:
            idx[tuple(flag_positions[0])] = 112
        if teams_with_flag[0] == 1:
            idx[tuple(flag_positions[1])] = 113
        for a, pos in agent_positions.items():
            if has_flag[a] == 1:
                idx[tuple(pos)] += 100
        return idx

    # one colour per sprite index (the reference pastes PNG sprites from cwd/img; this build draws squares and letters, so
    # that ``utils.create_gif`` / ``duel(render=True)`` work without those files)
    _SPRITE_RGB = {0: (0.93, 0.93, 0.93), 1: (0.25, 0.25, 0.25), 2: (0.55, 0.45, 0.35), 3: (0.72, 0.62, 0.52),
                   12: (0.35, 0.55, 1.0), 13: (1.0, 0.4, 0.4), 112: (0.8, 0.85, 1.0), 113: (1.0, 0.85, 0.85)}
    _TYPE_LETTER = "SGVM"  # scout, guardian, vaulter, miner

    def render_image(self, frame_path=None, plot_image=False):
        """gridworld_ctf.py:1112-1163: one image of the current grid; saved to ``frame_path`` (dpi 300, then closed) and / or
        shown.  Same cell -> sprite choice as the reference (``render_indices``); drawn with matplotlib primitives."""
        import matplotlib.pyplot as plt

        idx = self.render_indices(self.grid, self.agent_positions, self.has_flag, self.AGENT_TEAMS, self.FLAG_POSITIONS)
        g = self.GRID_SIZE
        rgb = np.zeros((g, g, 3))
        fig, ax = plt.subplots(figsize=(5, 5))
        for i in range(g):
            for j in range(g):
                k = int(idx[i, j])
                base = k - 100 if (k >= 104 and k <= 111) else k
                if 4 <= base <= 11:  # an agent: team colour, type letter, a ring when it carries a flag
                    team = 0 if base < 8 else 1
                    rgb[i, j] = (0.2, 0.4, 0.9) if team == 0 else (0.9, 0.25, 0.25)
                    ax.text(j, i, self._TYPE_LETTER[(base - 4) % 4] + ("*" if k >= 100 else ""), ha="center", va="center",
                            color="white", fontsize=max(4, 110 // g), fontweight="bold")
                else:
                    rgb[i, j] = self._SPRITE_RGB.get(k, (1.0, 0.0, 1.0))
                    if k in (12, 13, 112, 113):
                        ax.text(j, i, "F" if k < 100 else "f", ha="center", va="center", color="black", fontsize=max(4, 110 // g))
        ax.imshow(rgb, interpolation="nearest")
        ax.set_xticks(np.arange(-0.5, g, 1))
        ax.set_yticks(np.arange(-0.5, g, 1))
        ax.set_xticklabels([])
        ax.set_yticklabels([])
        ax.grid(color="white", linewidth=1)
        ax.tick_params(length=0)
        if plot_image:
            plt.show()
        if frame_path is not None:
            fig.savefig(frame_path, dpi=300)
            plt.close(fig)

    def play(self, player=0, agents=None, use_ego_state=False, device="cpu", render_ego_state=False):
        """gridworld_ctf.py:1165-1262: step the env from the keyboard (w s d a x = actions 0..4, t g h f = 5..8, p = quit);
        the other agents act randomly through ``np.random.randint(8, size=N)`` as in the reference.  ``agents`` (the
        reference's path through ``choose_action`` / ``ut.add_noise``, which its own networks do not provide) is not supported."""
        if agents is not None:
            raise NotImplementedError("play(agents=...) relies on Agent.choose_action, which the reference's networks do not define")
        keys = {"w": 0, "s": 1, "d": 2, "a": 3, "x": 4, "t": 5, "g": 6, "h": 7, "f": 8}
        self.reset()
        self.render()
        move_counter, total_score = 0, 0
        while True:
            print(f"Move {move_counter}")
            raw = None
            while raw not in list(keys) + ["p"]:
                raw = input("Enter an action")
            if raw == "p":
                print("Game exited")
                break
            actions = np.random.randint(8, size=self.N_AGENTS)
            actions[player] = keys[raw]
            _, rewards, done = self.step([int(a) for a in actions])
            total_score += rewards[0]
            move_counter += 1
            self.render()
            if done:
                print(f"You win!, total score {total_score}")
                break

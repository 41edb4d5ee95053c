"""The RNG digests (ctf_mt.h, ctf_ring_dev.h, ctf_step_core.h) at crafted generator states and at every position of a block.

The step kernel never looks at a random word: it reads one hit bit per position (np.random.rand() < TAG_PROBABILITY as a 53-bit
integer compare), low nibbles (randint) and top bytes (_randbelow), through windows of 128 bits / 96 nibbles / 64 bytes, with a slow
path beyond each window, a mirror of the next ring's head behind each digest array and a hop into the other ring's own array past
it.  Seeded streams reach the edges of all this only by chance.  Here the generators are set word by word (tests/_mt_craft.py;
tests/test_rng_edges_cpu.py holds the fixtures to the stdlib and NumPy): a rand() that EQUALS the probability, every start
position of both streams, shuffles that reject 70 words in a row, seeds and counters at their boundaries.

Every case is stepped by the C oracle first (tests/_rng_edge_cases.oracle_gate: status 0, a bounded number of words per step) and only
then handed to the device.  Every test compares the float64 rewards and `done` of every step with the oracle and, at the end, the full
state view and both generators' 625 words of every env; all of it exactly."""
import random

import numpy as np
import pytest

import _rng_edge_cases as R
import oracle
from _cases import Case, pkg, view_arrays
from _mt_craft import MT_N

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _dev_states(states, dev):
    return torch.from_numpy(states.view(np.int32)).to(dev)


def _first_bad(ok):
    return int(np.flatnonzero(~ok)[0])


def _run_on_device(case, monkeypatch, lanes=None, every=None):
    """`case` through the oracle's gate, then on the device against what the oracle gave -> (vec, the oracle's run); the caller closes vec"""
    ref = R.oracle_gate(case)  # on the CPU first: a case the oracle has not stepped within the gate's bounds never reaches a kernel
    if lanes is not None:
        monkeypatch.setenv("CTF_STEP_W", str(lanes))  # both read when the handle is created
    if every is not None:
        monkeypatch.setenv("CTF_RNG_REFILL_EVERY", str(every))
    counter = case.rng_mode == "counter"
    E = case.n_envs
    seeds = (case.seeds[:, 0], case.seeds[:, 1]) if counter else (np.arange(E, dtype=np.uint64), np.arange(E, dtype=np.uint64))
    vec = pkg.VecGridworldCtf(E, device=0, py_seeds=seeds[0], np_seeds=seeds[1], rng_mode=case.rng_mode, tune_placement=False, **case.kwargs)
    N, G, dev = vec.N_AGENTS, vec.GRID_SIZE, vec.device
    if counter:
        ctr = torch.from_numpy(case.counters.view(np.int64)).to(dev)
        vec.set_rng_counters(ctr)
        assert torch.equal(vec.get_rng_counters(), ctr), f"{case.name}: the counters do not come back as they were set"
    else:
        py, npw = _dev_states(case.py_states, dev), _dev_states(case.np_states, dev)
        vec.set_rng_states(py, npw)  # one call for the batch
        back = vec.get_rng_states()
        assert torch.equal(back[0], py) and torch.equal(back[1], npw), f"{case.name}: the states do not come back as they were set"
    acts = torch.empty((E, N), dtype=torch.int8, device=dev)
    for t in range(case.steps):
        vec.random_actions(acts, seed=R.ACT_SEED, step=t)
        if t == 0:
            a = acts.cpu().numpy()
            assert all(np.array_equal(a[e], oracle.philox_actions(N, R.ACT_SEED, 0, e)) for e in range(E))
        vec.step(acts, auto_reset=True, want_f64=True)
        r64, d, live = vec.rewards64.cpu().numpy(), vec.done.cpu().numpy(), ref.live[t]
        ok = (r64 == ref.rewards[t]).all(1) & (d == ref.done[t]) | ~live
        assert ok.all(), f"{case.name} W={lanes} refill={every}: env {_first_bad(ok)} step {t}: {r64[_first_bad(ok)]} vs {ref.rewards[t][_first_bad(ok)]}"
        if counter:
            ok = (vec.get_rng_counters().cpu().numpy().view(np.uint64) == ref.counters[t]).all(1) | ~live
            assert ok.all(), f"{case.name}: env {_first_bad(ok)} step {t}: words consumed"
    for e in np.flatnonzero(ref.alive):
        got = view_arrays(vec.get_state(int(e)), N, G)
        for k in R.VIEW_KEYS:
            assert np.array_equal(np.asarray(got[k]), np.asarray(ref.views[e][k])), f"{case.name} W={lanes} refill={every}: env {e} final {k}"
    if not counter:
        py, npw = (s.cpu().numpy().view(np.uint32) for s in vec.get_rng_states())
        ok = ((py == ref.py_final).all(1) & (npw == ref.np_final).all(1)) | ~ref.alive
        assert ok.all(), f"{case.name} W={lanes} refill={every}: env {_first_bad(ok)}: generators ({py[_first_bad(ok), MT_N]}, {npw[_first_bad(ok), MT_N]})"
    assert vec.status() & ~case.allow_status == 0
    return vec, ref


def _device_tags(vec):
    return vec.counters()[0][:, R.TAG_COUNT].sum(1).cpu().numpy()


# ---- a. the threshold edge ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 8])
@pytest.mark.parametrize("every", [0, 1])
@pytest.mark.parametrize("th", R.THRESHOLDS, ids=hex)
def test_a_rand_equal_to_the_tag_probability_misses_and_the_next_one_below_hits(th, every, lanes, monkeypatch):
    """64 dense 5 x 5 envs whose np.random blocks give rand() == (th 2^26 + th / 2) / 2^53 at every pair, from start positions 0 .. 63
    (the import digests them: k_rng_refill).  With that value as TAG_PROBABILITY nothing is tagged; one unit of 2^-53 higher every
    rand() hits: ceil(p 2^53), its split at bit 26, the >> 5 / >> 6 and the < of mt_lt53 all sit on this edge."""
    tags = {}
    for which in ("equal", "above"):
        vec, ref = _run_on_device(R.threshold_case(th, which), monkeypatch, lanes, every)
        tags[which] = _device_tags(vec)
        assert np.array_equal(tags[which], ref.tags), which
        vec.close()
    assert not tags["equal"].any() and tags["above"].sum() > 0
    eq, ab = R.threshold_case(th, "equal"), R.threshold_case(th, "above")
    R.check_threshold(R.oracle_gate(eq), R.oracle_gate(ab), R.np_pairs(R.case_config(eq)))


@pytest.mark.parametrize("every", [0, 1])
@pytest.mark.parametrize("th", R.THRESHOLDS, ids=hex)
def test_the_threshold_edge_on_blocks_the_step_launches_regenerate(th, every, monkeypatch):
    """The same edge where the other two digest builders meet it: the threshold block is two twists on from the block handed over, so
    it is made by a tail block of k_step (wave_next_block / wave_digest / wave_link) or, without tail blocks, by the one-lane safety net
    (ring_make_ready).  8 x 8, 8 v 8: the third step enters the block, the fourth draws 256 words of it."""
    runs = {}
    for which in ("equal", "above"):
        vec, runs[which] = _run_on_device(R.twisted_threshold_case(th, which), monkeypatch, None, every)
        alive = runs[which].alive
        assert np.array_equal(_device_tags(vec)[alive], runs[which].tags[alive]), which
        vec.close()
    R.check_twisted(runs["equal"], runs["above"])


@pytest.mark.parametrize("every", [0, 1])
def test_the_two_ends_of_the_compare(every, monkeypatch):
    """TAG_PROBABILITY = 2^-53: only the draw 0 is below it, and hits.  1 - 2^-53: only the largest draw is not below it, and misses."""
    vec, ref = _run_on_device(R.end_case("lowest"), monkeypatch, None, every)
    tags = _device_tags(vec)
    assert tags.sum() > 0 and np.array_equal(tags, ref.tags)
    vec.close()
    vec, ref = _run_on_device(R.end_case("highest"), monkeypatch, None, every)
    assert not _device_tags(vec).any() and not ref.tags.any()
    vec.close()


# ---- b. every start position ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [0, 1])
@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_every_start_position_of_both_streams(lanes, every, monkeypatch):
    """625 arena envs, env e's `random` generator at position e and its np.random generator at (233 e) mod 625 of a seeded block, 0 and
    624 included: every alignment of the three windows next to the end of a block, a rand() on every word pair of the seam, and (the
    coverage asserted from the oracle's positions) at least 150 envs of either stream going over a seam in the 12 steps."""
    case = R.sweep_arena_case()
    R.check_sweep_coverage(case, R.oracle_gate(case))
    vec, _ = _run_on_device(case, monkeypatch, lanes, every)
    vec.close()


@pytest.mark.parametrize("every", [0, 1])
def test_every_start_position_with_steps_of_260_words(every, monkeypatch):
    """The same sweep on 8 x 8 with 8 v 8 agents: a step draws about 260 np.random words, past the hit window and — from a start near
    the end of a block — past the 208-bit mirror into the other ring's own array (stream_slow's second hop: asserted from the oracle).
    Envs that run out of respawn cells are dropped."""
    case = R.sweep_8v8_case()
    run = R.oracle_gate(case)
    R.check_second_hop(run)
    assert run.alive.sum() >= case.n_envs // 2
    vec, _ = _run_on_device(case, monkeypatch, None, every)
    vec.close()


# ---- c. rejection runs in the shuffle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_shuffles_that_reject_long_runs_of_words(lanes, monkeypatch):
    """48 arena envs whose `random` blocks hold runs of up to 70 words that every _randbelow(n), n no power of two, rejects — out of
    the 64-byte window, over the end of the block into the mirror, and ending on the window's last byte for every alignment."""
    case = R.rejection_case()
    R.check_rejection_reach(R.oracle_gate(case))
    vec, _ = _run_on_device(case, monkeypatch, lanes)
    vec.close()


# ---- d. seeding -------------------------------------------------------------------------------------------------------------------------
def test_seeds_on_both_sides_of_32_bits():
    """k_seed: init_by_array with a one-word key below 2^32 and a two-word key from 2^32 on, against random.Random(s) itself; np.random
    takes 32 bits."""
    S = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 63) + 11, (1 << 64) - 1] + [1_000_003 * k + 17 for k in range(57)]
    kw, E = Case("arena_stress").kwargs, len(S)
    vec = pkg.VecGridworldCtf(E, device=0, py_seeds=S, np_seeds=[s & 0xFFFFFFFF for s in S], tune_placement=False, **kw)
    py, npw = (s.cpu().numpy().view(np.uint32) for s in vec.get_rng_states())
    for e, s in enumerate(S):
        assert np.array_equal(py[e], np.array(random.Random(s).getstate()[1], dtype=np.uint32)), f"random.seed({s})"
        st = np.random.RandomState(s & 0xFFFFFFFF).get_state()
        assert np.array_equal(npw[e, :MT_N], st[1]) and npw[e, MT_N] == st[2] == MT_N, f"np.random.seed({s & 0xFFFFFFFF})"
    refs = [oracle.OracleEnv(vec.cfg) for _ in S]
    for r, s in zip(refs, S):
        r.seed(s, s & 0xFFFFFFFF)
    acts = torch.empty((E, vec.N_AGENTS), dtype=torch.int8, device=vec.device)
    for t in range(20):
        vec.random_actions(acts, seed=R.ACT_SEED, step=t)
        vec.step(acts, auto_reset=True, want_f64=True)
        r64, d = vec.rewards64.cpu().numpy(), vec.done.cpu().numpy()
        for e, r in enumerate(refs):
            rw, dn, status = r.step(oracle.philox_actions(vec.N_AGENTS, R.ACT_SEED, t, e))
            assert status == 0 and np.array_equal(r64[e], rw) and int(d[e]) == int(dn), f"seed {S[e]} step {t}"
    py, npw = (s.cpu().numpy().view(np.uint32) for s in vec.get_rng_states())
    for e, r in enumerate(refs):
        a, b = view_arrays(vec.get_state(e), vec.N_AGENTS, vec.GRID_SIZE), view_arrays(r.get_state(), vec.N_AGENTS, vec.GRID_SIZE)
        for k in R.VIEW_KEYS:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), f"seed {S[e]} final {k}"
        rpy, rnp = r.get_rng_state()
        assert np.array_equal(py[e], rpy) and np.array_equal(npw[e], rnp), f"seed {S[e]}: generators"
    assert vec.status() == 0
    with pytest.raises(ValueError, match="Seed must be between 0 and 2\\*\\*32 - 1"):
        vec.seed(S, [0] * (E - 1) + [1 << 32])
    with pytest.raises(ValueError, match="Seed must be between 0 and 2\\*\\*32 - 1"):
        pkg.VecGridworldCtf(E, device=0, py_seeds=S, np_seeds=S, tune_placement=False, **kw)
    vec.close()


# ---- e. counters ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.COUNTER_KS)
def test_counters_set_at_every_offset_of_a_block(k, monkeypatch):
    """k_set_counters away from values a run produced: 625 envs, the `random` tape at word 624 k + e and the np.random tape at
    624 k' + (233 e) mod 625 — every offset, both sides of a block boundary, and with k = 2^33 a block index that needs the high
    counter word of ctr_block.  The counters come back unchanged and agree with the oracle's after every one of 8 steps."""
    vec, _ = _run_on_device(R.counter_case(k), monkeypatch)
    vec.close()

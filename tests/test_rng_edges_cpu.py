"""The crafted generator states of tests/test_gpu_rng_edges.py mean what they claim — checked against the stdlib's and NumPy's own
MT19937, never against the code under test — and every crafted case passes the oracle-first gate (tests/_rng_edge_cases.py) with the
coverage its GPU test relies on.  The last three tests are the GPU tests' expectations turned the wrong way: each must fail."""
import random

import numpy as np
import pytest

import _rng_edge_cases as R
from _mt_craft import (MT_N, np_block_at_threshold, np_block_with_outputs, p_above, p_equal, py_rejection_run, seeded_np, seeded_py, temper,
                       twist, untemper, untwist)

CORNERS = [0, 1, 0x80000000, 0xFFFFFFFF, 0x7FFFFFFF, 0xFF000000, 0x00FFFFFF, 0x9D2C5680, 0xEFC60000, 0x5555555 << 5]
TH_CHECKED = R.THRESHOLDS + (2, 0x2AAAAAA, 1 << 26, (1 << 26) - 1)


def _py_outputs(words, pos, count):
    r = random.Random()
    r.setstate((3, tuple(int(w) for w in words[:MT_N]) + (int(pos),), None))
    return [r.getrandbits(32) for _ in range(count)], r


def _np_generator(words, pos):
    rs = np.random.RandomState()
    rs.set_state(("MT19937", np.asarray(words[:MT_N], dtype=np.uint32), int(pos), 0, 0.0))
    return rs


def test_temper_and_untemper_are_inverse():
    x = np.concatenate([np.random.default_rng(11).integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32), np.array(CORNERS, np.uint32)])
    assert np.array_equal(temper(untemper(x)), x) and np.array_equal(untemper(temper(x)), x)
    for c in CORNERS:
        assert temper(untemper(c)) == c and untemper(temper(c)) == c and isinstance(untemper(c), int)


@pytest.mark.parametrize("pos", [0, 1, 311, 622, 623])
def test_the_stdlib_and_numpy_draw_the_tempered_words_of_a_crafted_state(pos):
    words = np_block_at_threshold(0x5555555, np.random.default_rng(pos))
    got, _ = _py_outputs(words, pos, MT_N - pos)
    assert got == [int(t) for t in temper(words)[pos:]]
    assert np.array_equal(_np_generator(words, pos).randint(0, 1 << 32, MT_N - pos, dtype=np.uint64), temper(words)[pos:])
    assert all(t >> 5 == 0x5555555 for t in got)


@pytest.mark.parametrize("th", TH_CHECKED)
def test_every_rand_of_a_threshold_block_equals_p_equal(th):
    words = np_block_at_threshold(th, np.random.default_rng(th))
    for pos in (0, 1):  # the pairs that start at an even word, then those at an odd one: every pair inside the block
        u = _np_generator(words, pos).random_sample((MT_N - pos) // 2)
        assert (u == p_equal(th)).all()
        assert not (u < p_equal(th)).any() and (u < p_above(th)).all()
    assert p_above(th) - p_equal(th) == 2.0 ** -53


def test_the_two_ends_of_the_compare():
    lo, hi = np_block_with_outputs(seeded_np(1)[:MT_N], 10, 128, 0), np_block_with_outputs(seeded_np(1)[:MT_N], 10, 128, 0xFFFFFFFF)
    assert (_np_generator(lo, 10).random_sample(64) < 2.0 ** -53).all()
    assert not (_np_generator(hi, 10).random_sample(64) < 1.0 - 2.0 ** -53).any() and 1.0 - 2.0 ** -53 < 1.0
    assert np.array_equal(lo[:10], seeded_np(1)[:10]) and np.array_equal(lo[138:], seeded_np(1)[138:MT_N])  # (the rest stays ordinary)


@pytest.mark.parametrize("pos,run", R.REJECTION_SPECS)
def test_a_rejection_run_is_rejected_by_the_stdlibs_shuffle(pos, run):
    base = seeded_py(3000)[:MT_N]
    words = py_rejection_run(base, pos, run)
    lo, hi = min(MT_N, pos + 1), min(MT_N, pos + 1 + run)
    t, t0 = temper(words), temper(base)
    assert (t[lo:hi] >> 24 == 0xFF).all() and np.array_equal(t[lo:hi] & 0xFFFFFF, t0[lo:hi] & 0xFFFFFF)
    assert np.array_equal(words[:lo], base[:lo]) and np.array_equal(words[hi:], base[hi:])
    assert hi - lo == min(run, max(0, MT_N - 1 - pos))
    r = _py_outputs(words, lo, 0)[1]  # _randbelow(n) = getrandbits(n.bit_length()), drawn again while >= n: all ones for every word of the run
    for k in (2, 3, 4, 5) * ((hi - lo) // 4):
        assert r.getrandbits(k) == (1 << k) - 1


def test_untwist_against_numpys_own_regeneration():
    target = np_block_at_threshold(0x5555555, np.random.default_rng(3))
    middle, block = untwist(target, reachable=True)
    assert np.array_equal(block[:MT_N - 1], target[:MT_N - 1]) and np.array_equal(block, twist(middle))
    first, again = untwist(middle)
    assert np.array_equal(again, middle)  # (all 624 words: `reachable`)
    rs = _np_generator(first, MT_N)
    rs.random_sample(MT_N // 2)  # the whole of `middle` ...
    assert np.array_equal(rs.get_state()[1], middle) and rs.get_state()[2] == MT_N
    assert (rs.random_sample(300) == p_equal(0x5555555)).all()  # ... and then the threshold block
    assert np.array_equal(rs.get_state()[1][:MT_N - 1], target[:MT_N - 1])


# ---- the oracle at the crafted states, and the gate over every case ---------------------------------------------------------------------
@pytest.mark.parametrize("th", R.THRESHOLDS)
def test_oracle_at_the_threshold(th):
    eq, ab = R.threshold_case(th, "equal"), R.threshold_case(th, "above")
    assert np.array_equal(eq.np_states, ab.np_states) and np.array_equal(eq.np_states[:, MT_N], np.arange(R.DENSE_ENVS))
    pairs = R.np_pairs(R.case_config(eq))
    R.check_threshold(R.oracle_gate(eq), R.oracle_gate(ab), pairs)
    run = R.oracle_gate(ab)
    assert (run.start_np + run.words_np <= MT_N).all()  # every draw of both steps stays inside the crafted block
    eq2, ab2 = R.oracle_gate(R.twisted_threshold_case(th, "equal")), R.oracle_gate(R.twisted_threshold_case(th, "above"))
    R.check_twisted(eq2, ab2)


def test_oracle_at_the_two_ends():
    assert R.oracle_gate(R.end_case("lowest")).tags.sum() > 0 and not R.oracle_gate(R.end_case("highest")).tags.any()
    for which in ("lowest", "highest"):
        run = R.oracle_gate(R.end_case(which))
        assert (run.start_np[0] == np.arange(R.DENSE_ENVS)).all() and (run.start_np[-1] + run.words_np[-1] <= np.arange(R.DENSE_ENVS) + 128).all()


def test_gate_and_coverage_of_the_start_position_sweeps():
    case = R.sweep_arena_case()
    assert np.array_equal(case.py_states[:, MT_N], np.arange(625)) and sorted(case.np_states[:, MT_N]) == list(range(625))
    R.check_sweep_coverage(case, R.oracle_gate(case))
    big = R.sweep_8v8_case()
    run = R.oracle_gate(big)
    R.check_second_hop(run)
    assert run.alive.sum() >= big.n_envs // 2 and run.words_np[run.live].min() >= 2 * R.np_pairs(R.case_config(big)) == 256


def test_gate_and_reach_of_the_rejection_runs():
    run = R.oracle_gate(R.rejection_case())
    R.check_rejection_reach(run)
    spec_of = np.arange(R.REJECTION_ENVS) % len(R.REJECTION_SPECS)
    for k, (pos, n) in enumerate(R.REJECTION_SPECS):  # the whole run is drawn in the crafted step: 14 accepted words and the run
        crafted = min(n, max(0, MT_N - 1 - pos))
        assert (run.words_py[0][spec_of == k] >= 14 + crafted).all(), (pos, n)
    assert (run.words_py[1:] < 64).all()  # the three steps after it: ordinary words


@pytest.mark.parametrize("k", R.COUNTER_KS)
def test_oracle_counters_continue_where_they_are_set(k):
    """OracleEnv.set_rng_counters: a tape read from word n on gives the words a tape read from 0 gives after n draws"""
    case = R.counter_case(k)
    run = R.oracle_gate(case)
    assert np.array_equal(run.start_py[0], case.counters[:, 0].astype(np.int64)) and np.array_equal(run.start_np[0], case.counters[:, 1].astype(np.int64))
    assert np.array_equal(run.counters[-1, :, 0].astype(np.int64), run.start_py[0] + run.words_py.sum(0))
    if k == 0:  # moving a tape forward equals having drawn that far: a second env continues a first one's game
        import oracle

        ref, again = oracle.OracleEnv(R.case_config(case)), oracle.OracleEnv(R.case_config(case))
        for env in (ref, again):
            env.seed(int(case.seeds[0, 0]), int(case.seeds[0, 1]))
        for t in range(5):
            assert ref.step(oracle.philox_actions(ref.n, R.ACT_SEED, t, 0))[2] == 0
        assert ref.get_rng_counters() != (0, 0) and again.get_rng_counters() == (0, 0)
        again.set_rng_counters(*ref.get_rng_counters())
        again.set_state(ref.get_state())
        for t in range(5, 10):
            a, b = ref.step(oracle.philox_actions(ref.n, R.ACT_SEED, t, 0)), again.step(oracle.philox_actions(ref.n, R.ACT_SEED, t, 0))
            assert a[2] == 0 and np.array_equal(a[0], b[0]) and again.get_rng_counters() == ref.get_rng_counters()


# ---- the GPU tests' expectations can fail ------------------------------------------------------------------------------------------------
def test_swapped_probabilities_fail_the_threshold_expectations():
    th = R.THRESHOLDS[0]
    eq, ab = R.oracle_gate(R.threshold_case(th, "equal")), R.oracle_gate(R.threshold_case(th, "above"))
    with pytest.raises(AssertionError):
        R.check_threshold(ab, eq, R.np_pairs(R.case_config(R.threshold_case(th, "equal"))))
    assert not np.array_equal(eq.rewards, ab.rewards) and not np.array_equal(eq.tags, ab.tags)  # (the device run under one cannot pass as the other)


def test_short_rejection_runs_fail_the_reach_assertion():
    short = tuple((pos, min(run, 10)) for pos, run in R.REJECTION_SPECS)
    with pytest.raises(AssertionError):
        R.check_rejection_reach(R.oracle_gate(R.rejection_case(short)))


def test_one_step_fails_the_sweeps_coverage():
    case = R.sweep_arena_case(1)
    with pytest.raises(AssertionError, match="cross a seam"):
        R.check_sweep_coverage(case, R.oracle_gate(case))

"""The host-side helpers of tests/test_gpu_policy_edges.py, checked without a GPU: the NumPy Philox4x32-10 of tests/_philox.py against
the published known-answer vectors and against the independent implementation the counter-mode goldens were recorded with, and the
share of samples the sampler test's "too close to a CDF boundary" criterion can leave out."""
import importlib.util
import os
import sys

import numpy as np

import _philox
from _cases import GOLDEN


def test_numpy_philox_gives_the_published_known_answers():
    """Random123's kat_vectors for philox4x32-10: all-zero, all-ones and the digits of pi."""
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    for counter, key, want in kat:
        got = _philox.philox4x32_10(counter, key)
        assert tuple(int(w) for w in got) == want, (counter, key, [hex(int(w)) for w in got])


def test_numpy_philox_agrees_word_for_word_with_the_golden_scripts_function():
    # Loading the recording script runs its top-level imports (_refimport, make_golden: both inert without the reference, they only
    # define things) — the function itself needs nothing but M32.  If those scripts ever stop importing on a machine without the
    # reference, cut the function's source out of the file here instead of loading the module.
    spec = importlib.util.spec_from_file_location("make_golden_counter", os.path.join(GOLDEN, "make_golden_counter.py"))
    mgc = importlib.util.module_from_spec(spec)
    saved_path = list(sys.path)
    try:
        spec.loader.exec_module(mgc)
    finally:
        sys.path[:] = saved_path  # the script puts its own directory first: keep that out of the other tests' imports
    rng = np.random.default_rng(2011)
    words = rng.integers(0, 1 << 32, (300, 6), dtype=np.uint64)
    words[:8] = [[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0],
                 [0, 0, 0, 0, 0, 1], [0xFFFFFFFF] * 6]
    got = np.stack(_philox.philox4x32_10(words[:, :4].T, words[:, 4:].T), axis=1)  # vectorised: all 300 at once
    for row, g in zip(words.tolist(), got.tolist()):
        assert tuple(g) == tuple(mgc.philox4x32_10(tuple(row[4:]), tuple(row[:4]))), row
    # the sampler's packing of 64-bit index / offset / seed into the words
    seed, offset = 0x1234_5678_9ABC_DEF0, (3 << 32) | 7
    u = _philox.sampler_uniforms(seed, offset, 5)
    for i in range(5):
        x = mgc.philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (i, 0, offset & 0xFFFFFFFF, offset >> 32))[0]
        assert u[i] == (x >> 8) / 2.0 ** 24


def test_the_boundary_criterion_alone_leaves_out_far_less_than_one_percent():
    """A uniform lies within 1e-5 of one of A boundaries with probability about 2 A 1e-5 (3e-4 for 15 actions): for logits of the scale
    the head test sees (standard deviation about 2) and its mix of decisions, the share left out stays below a fifth of the 1 % cap."""
    rng = np.random.default_rng(5)
    B = 1 << 16
    u = _philox.sampler_uniforms(0x1234_5678_9ABC_DEF0, (3 << 32) | 7, B)
    assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.01
    for a in (1, 4, 5, 9, 13, 15):
        decision = (np.arange(B) % 3).astype(np.float32)
        logits = (rng.standard_normal((B, a)) * 2.0).astype(np.float32)
        prob, logp, entropy = _philox.softmax_stats(_philox.masked_logits(logits, decision))
        last = _philox.last_legal(decision, a)
        action, sure = _philox.inverse_cdf(prob, u, last)
        assert (~sure).mean() < 0.002, (a, (~sure).mean())
        assert bool((action <= last).all()) and bool((prob[np.arange(B), action] > 0).all())  # never a masked action
        assert np.allclose(np.exp(logp[decision != 2]).sum(axis=1), 1.0) and bool((entropy[decision == 2] == 0.0).all())

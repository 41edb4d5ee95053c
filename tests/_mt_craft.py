"""TEST INFRASTRUCTURE: MT19937 states built word by word, so that the digests the step kernel reads (ctf_mt.h: one hit bit per
position, low nibbles, top bytes) meet values that no seeded stream produces in a test's lifetime.  Pure Python / NumPy: nothing here
touches the code under test; tests/test_rng_edges_cpu.py checks every helper against the stdlib's and NumPy's own generators.

A generator state is 625 uint32: the 624 RAW words and the position, the form of ``random.getstate()[1]`` and
``np.random.get_state()[1:3]``.  What a draw sees is the TEMPERED word, and tempering is a bijection of the 32-bit words, so any
tempered value can be placed at any position of a block.  The block AFTER a crafted one is never crafted: it is whatever the twist
makes of the crafted words."""
import random

import numpy as np

MT_N = 624
_M32 = 0xFFFFFFFF


def _words(x):
    return np.asarray(x, dtype=np.uint64) & np.uint64(_M32)  # (64-bit lanes: the left shifts below must not wrap)


def _back(x, y):
    return int(y) if np.ndim(x) == 0 else y.astype(np.uint32)


def temper(x):
    """MT19937's output function of a raw word (scalar -> int, array -> uint32 array)"""
    y = _words(x)
    y = y ^ (y >> np.uint64(11))
    y = y ^ ((y << np.uint64(7)) & np.uint64(0x9D2C5680))
    y = y ^ ((y << np.uint64(15)) & np.uint64(0xEFC60000))
    y = y ^ (y >> np.uint64(18))
    return _back(x, y & np.uint64(_M32))


def _undo(z, shift, mask, left):
    """t with t ^ ((t << shift) & mask) == z (or >>, mask all ones): every round fixes `shift` more bits"""
    t = z
    for _ in range(32 // shift + 1):
        moved = (t << np.uint64(shift)) if left else (t >> np.uint64(shift))
        t = z ^ (moved & np.uint64(mask))
    return t & np.uint64(_M32)


def untemper(x):
    """the raw word whose output is x"""
    y = _words(x)
    y = _undo(y, 18, _M32, False)
    y = _undo(y, 15, 0xEFC60000, True)
    y = _undo(y, 7, 0x9D2C5680, True)
    y = _undo(y, 11, _M32, False)
    return _back(x, y)


def seeded_py(seed):
    """random.seed(seed) -> uint32 [625] (position 624)"""
    return np.array(random.Random(int(seed)).getstate()[1], dtype=np.uint32)


def seeded_np(seed):
    """np.random.seed(seed) -> uint32 [625] (position 624)"""
    st = np.random.RandomState(int(seed)).get_state()
    return np.concatenate([st[1].astype(np.uint32), np.array([st[2]], np.uint32)])


def at_position(state625, pos):
    """the same words, the consumer standing at `pos` (0 .. 624)"""
    assert 0 <= int(pos) <= MT_N
    out = np.array(state625, dtype=np.uint32)
    out[MT_N] = int(pos)
    return out


# ---- np.random.rand() at the threshold ---------------------------------------------------------------------------------------------
# random_sample() = ((a >> 5) * 2^26 + (b >> 6)) / 2^53 of two consecutive outputs a, b.  When the top 27 bits of EVERY output of a
# block are th, every pair gives (th * 2^26 + (th >> 1)) / 2^53, whichever word a draw starts at.
def _numerator(th):
    assert 0 < th < (1 << 27) - 1
    return (th << 26) + (th >> 1)


def p_equal(th):
    """the probability every rand() of np_block_at_threshold(th) EQUALS: rand() < p is false"""
    p = _numerator(th) / 2.0 ** 53
    assert int(p * 2 ** 53) == _numerator(th) and p * 2 ** 53 == _numerator(th)
    return p


def p_above(th):
    """one unit of 2^-53 higher: every rand() of the block is the largest draw below it"""
    p = (_numerator(th) + 1) / 2.0 ** 53
    assert int(p * 2 ** 53) == _numerator(th) + 1 and p * 2 ** 53 == _numerator(th) + 1
    return p


def np_block_at_threshold(th, rng):
    """624 raw words whose outputs are (th << 5) | 5 random bits (rng: a numpy Generator)"""
    assert 0 <= th < (1 << 27)
    low = rng.integers(0, 32, MT_N, dtype=np.uint32)
    return untemper(np.uint32(th << 5) | low)


def np_block_with_outputs(base_words, pos, count, value):
    """a copy of a normally seeded block whose outputs at pos .. pos + count - 1 (up to 623) are `value`"""
    out = np.array(base_words[:MT_N], dtype=np.uint32)
    hi = min(MT_N, int(pos) + int(count))
    out[int(pos):hi] = untemper(int(value))
    return out


# ---- random.shuffle's rejections ----------------------------------------------------------------------------------------------------
def py_rejection_run(base_words, pos, run):
    """A copy of a normally seeded block in which words pos + 1 .. pos + run (up to 623) have an output with top byte 0xFF and the low
    24 bits they had: _randbelow(n) takes the top n.bit_length() bits of a word, so every n that is no power of two rejects them.  A
    consumer at `pos` draws one ordinary word first.  The run ends inside the block, on ordinary words."""
    out = np.array(base_words[:MT_N], dtype=np.uint32)
    lo, hi = int(pos) + 1, min(MT_N, int(pos) + 1 + int(run))
    if lo < hi:
        out[lo:hi] = untemper((temper(out[lo:hi]) & np.uint32(0x00FFFFFF)) | np.uint32(0xFF000000))
    return out


# ---- a crafted block REACHED BY THE TWIST ---------------------------------------------------------------------------------------------
_UPPER, _LOWER, _MATRIX_A = 0x80000000, 0x7FFFFFFF, 0x9908B0DF


def twist(words):
    """the block after `words`: MT19937's in-place regeneration (what a generator does when its position reaches 624)"""
    mt = [int(w) for w in words[:MT_N]]
    for i in range(MT_N):
        y = (mt[i] & _UPPER) | (mt[(i + 1) % MT_N] & _LOWER)
        mt[i] = mt[(i + 397) % MT_N] ^ (y >> 1) ^ (_MATRIX_A if y & 1 else 0)
    return np.array(mt, dtype=np.uint32)


def _y_of(t):
    """y with (y >> 1) ^ (MATRIX_A if y & 1 else 0) == t (y >> 1 has no top bit: t's comes from MATRIX_A, i.e. from an odd y)"""
    return (((t ^ _MATRIX_A) << 1) | 1) & _M32 if t >> 31 else (t << 1) & _M32


def untwist(target, reachable=False):
    """-> (prev, block): 624 raw words `prev` and `block` = twist(prev), equal to `target` in words 0 .. 622.  (Word 623 of a block
    is a function of its words 0 and 396 and ONE bit of the block before, so it cannot be chosen.)  The low 31 bits of prev[0] do
    not enter the twist: they are 0, or with `reachable` what makes prev[623] follow from prev[0] and prev[396], so that `prev`
    is the twist of some block in all 624 words and can be untwisted again."""
    new = [int(w) for w in target[:MT_N]]
    old = [0] * (MT_N + 1)
    for i in range(MT_N - 1, -1, -1):  # word i of the new block fixes the top bit of old[i] and the low 31 bits of old[i + 1]
        m = old[i + 397] if i < MT_N - 397 else new[i - (MT_N - 397)]
        y = _y_of(new[i] ^ m)
        old[i] |= y & _UPPER
        if i + 1 < MT_N:  # (i = 623: y's low bits are new[0]'s — which they are only when `target` is a block that can occur)
            old[i + 1] |= y & _LOWER
    if reachable:
        old[0] |= _y_of(old[MT_N - 1] ^ old[396]) & _LOWER
    prev = np.array(old[:MT_N], dtype=np.uint32)
    return prev, twist(prev)

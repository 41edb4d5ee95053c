"""Philox4x32-10 in NumPy and the sampler contract of ctf_policy_head (include/ctf_policy.h) restated on top of it.

The generator is written from its publication (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11, and
Random123's philox.h), not from the kernel: one round maps the counter (c0, c1, c2, c3) under the round key (k0, k1) to
    (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0))
and the key is bumped by the Weyl constants between rounds (not after the last).
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)  # the two multipliers
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)  # golden ratio / sqrt(3) - 1: the key schedule
_LO, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (scalars or arrays that broadcast; only the low 32 bits of each count) -> 4 uint32 arrays."""
    words = np.broadcast_arrays(*[np.asarray(w).astype(np.uint64) & _LO for w in list(counter) + list(key)])
    c0, c1, c2, c3, k0, k1 = [w.copy() for w in words]
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LO, (p0 >> _32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def sampler_uniforms(seed, offset, n):
    """The uniform of samples 0 .. n - 1 as the header defines it: philox(counter = (i lo, i hi, offset lo, offset hi),
    key = (seed lo, seed hi)).x >> 8, scaled to [0, 1) -> float64 [n] (24-bit values: exact in float32 and float64)."""
    i = np.arange(n, dtype=np.uint64)
    seed, offset = int(seed), int(offset)
    x = philox4x32_10((i & _LO, i >> _32, offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return (x >> np.uint32(8)).astype(np.float64) / 16777216.0


def masked_logits(logits, decision):
    """logits float32 [B, A], decision [B] -> float64 [B, A]: logits + (mask - 1) * 1e9 evaluated in float32 (agent_network.py:66-75):
    decision 1 masks actions 5.., decision 0 nothing, any other value everything (-1e9 swallows a logit of ordinary size in float32)."""
    logits = np.asarray(logits, np.float32)
    a = logits.shape[1]
    dec = np.asarray(decision, np.float64).reshape(-1, 1)
    off = np.where(dec == 1.0, np.arange(a)[None, :] >= 5, dec != 0.0)
    return (logits + np.where(off, np.float32(-1e9), np.float32(0.0)).astype(np.float32)).astype(np.float64)


def softmax_stats(masked):
    """float64 masked logits [B, A] -> (probabilities, log-probabilities, entropy) in float64, with ONE float32 step: the log-normaliser
    max + log(sum exp(l - max)) is rounded to float32, as torch's float32 Categorical and the kernel have it.  That changes an ordinary
    row by 1e-7 relative; for the all-masked row (every logit -1e9) it is what makes log-prob and entropy 0: -1e9 + log A == -1e9."""
    mx = masked.max(axis=1, keepdims=True)
    e = np.exp(masked - mx)
    tot = e.sum(axis=1, keepdims=True)
    p = e / tot
    logp = masked - (mx + np.log(tot)).astype(np.float32).astype(np.float64)
    return p, logp, -(p * logp).sum(axis=1)


def last_legal(decision, n_actions):
    """The last action a sample may draw: 4 under decision 1 (or A - 1 when there are fewer than five actions), else A - 1."""
    return np.where(np.asarray(decision) == 1.0, min(4, n_actions - 1), n_actions - 1).astype(np.int64)


def inverse_cdf(p, u, last, margin=1e-5):
    """p float64 [B, A], u [B], last [B] -> (action [B], sure [B]): the number of CDF boundaries (running sums of p in index order) that
    are <= u, clamped to the last legal action; `sure` is False where u lies within `margin` of a boundary — a float32 running sum may
    fall on the other side of u there."""
    cdf = np.cumsum(p, axis=1)
    action = np.minimum((cdf <= u[:, None]).sum(axis=1), last)
    return action, (np.abs(cdf - u[:, None]) > margin).all(axis=1)

"""The stochastic-rounding rule of include/trs_abi.h in numpy integer arithmetic -- a test helper, not product code.

Written from the text of the header ("stochastic rounding of bf16 tables under the fused optimizers"), not from the HIP
source:

    sr_bf16(x, i, seed, t):  u = bits(x);  inf / NaN: u >> 16;  otherwise (u + r) >> 16
    r: 16 bits of Philox4x32-10 with counter (lo32(q), hi32(q), lo32(t), hi32(t)), q = i >> 3, and key (lo32(seed),
    hi32(seed)): word (i & 7) >> 1, the low half for even i, the high half for odd i.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # key increments
_MASK = np.uint64(0xFFFFFFFF)
_U32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two Python ints.  Returns the four output words as uint64
    arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & _MASK for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c0                 # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> _U32) ^ c1 ^ np.uint64(k0)), p1 & _MASK, ((p0 >> _U32) ^ c3 ^ np.uint64(k1)), p0 & _MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def random16(i, seed, t):
    """r of every element position in ``i`` (int64 array) for update ``t`` under ``seed``: uint32 array in [0, 65536)"""
    i = np.atleast_1d(np.asarray(i, dtype=np.int64))
    assert (i >= 0).all()
    seed, t = int(seed), int(t)
    assert 0 <= seed < 1 << 64 and 0 <= t < 1 << 64
    qi = i >> 3
    # one call serves the 8 elements of a q: where the positions are dense, hash every q of their range once
    q0, q1 = int(qi.min()), int(qi.max())
    dense = q1 - q0 + 1 <= i.size
    q = (np.arange(q0, q1 + 1, dtype=np.int64) if dense else qi).astype(np.uint64)
    z = np.zeros_like(q)
    words = np.stack(philox4x32_10((q & _MASK, q >> _U32, z + np.uint64(t & 0xFFFFFFFF), z + np.uint64(t >> 32)),
                                   (seed & 0xFFFFFFFF, seed >> 32)))
    j = i & 7
    w = words[j >> 1, (qi - q0) if dense else np.arange(i.size)]
    return np.where(j & 1, w >> np.uint64(16), w & np.uint64(0xFFFF)).astype(np.uint32)


def sr_bits(u, r):
    """the rule on the fp32 bit patterns ``u`` (uint32) with the 16-bit integers ``r``: bf16 bit patterns, uint16"""
    u = np.asarray(u, dtype=np.uint32)
    special = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    moved = (u.astype(np.uint64) + np.asarray(r, dtype=np.uint64)) >> np.uint64(16)
    return np.where(special, u >> np.uint32(16), moved.astype(np.uint32)).astype(np.uint16)


def sr_bf16(x, i, seed, t):
    """bf16 bit patterns (uint16) of the fp32 values ``x`` stored at element positions ``i`` in update ``t``"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float32))
    return sr_bits(x.view(np.uint32), random16(i, seed, t))


def bf16_bits_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_bits_exact(x):
    """bit patterns of fp32 values that ARE bf16 values (asserted)"""
    u = np.atleast_1d(np.asarray(x, dtype=np.float32)).view(np.uint32)
    assert (u & np.uint32(0xFFFF) == 0).all(), "not a bf16 value"
    return (u >> np.uint32(16)).astype(np.uint16)

"""The dropout mask of the HIP engine restated in numpy (csrc/lgm_philox.h, include/lgm_hip.h): what
tests/test_dropout_host.py checks against known answers and statistics, and what tests/test_hip_dropout.py holds the kernels to.

Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, the key
bumped after each of the first nine rounds.  For an activation [B, HW, C] (C % 4 == 0) element n = (b HW + pix) C + c belongs
to quad q = n >> 2 (a 64-bit number); counter = (q & 0xffffffff, q >> 32, layer, pass), key = (key & 0xffffffff, key >> 32);
the four output words are channels c .. c + 3.  An element is kept iff its word >= thr = min(2^32 - 1, floor(p 2^32)); kept
values are multiplied by scale = float32(1 / (1 - p)), the division in double; dropped ones become +0."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) of one shape, key: two -> four uint64 arrays holding the 32-bit output words"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    m0, m1, lo = np.uint64(M0), np.uint64(M1), np.uint64(MASK32)
    for r in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                    # 32 x 32 -> 64 bit: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & lo, p1 >> np.uint64(32), p1 & lo
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        if r < 9:
            k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


def operands(p):
    """(thr, scale) of probability p, as the host computes them"""
    thr = min(2 ** 32 - 1, int(math.floor(float(p) * 2.0 ** 32)))
    return thr, np.float32(1.0 / (1.0 - float(p)))


def words(shape, key, layer, pass_=0):
    """uint64 [B, HW, C]: the Philox word of every element of an activation of ``shape`` = (B, HW, C)"""
    B, HW, C = shape
    assert C % 4 == 0
    q = np.arange(B * HW * C // 4, dtype=np.uint64)
    key = int(key) & (2 ** 64 - 1)
    w = philox4x32_10((q & np.uint64(MASK32), q >> np.uint64(32), layer, pass_), (key & MASK32, key >> 32))
    return np.stack(w, axis=1).reshape(B, HW, C)


def keep(shape, key, layer, pass_, p):
    """bool [B, HW, C]: which elements survive"""
    return words(shape, key, layer, pass_) >= np.uint64(operands(p)[0])


def apply(x, key, layer, pass_, p):
    """float32 [B, HW, C] -> kept ? fl32(x * scale) : +0"""
    x = np.asarray(x, dtype=np.float32)
    k = keep(x.shape, key, layer, pass_, p)
    return np.where(k, x * operands(p)[1], np.float32(0.0)).astype(np.float32)

"""Test-only numpy restatement of the generator include/lfm.h defines (Philox4x32-10 and
Box-Muller): element j of sample s from (seed, s, j) alone."""

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays holding 32-bit words; key: two ints. Returns four arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK)
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def randn(seed, sample0, nsamp, n):
    """[nsamp, n] normals: row r is sample sample0 + r."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    half = (n + 1) // 2
    p = np.tile(np.arange(half, dtype=np.uint64), (nsamp, 1))
    s = np.repeat((np.arange(nsamp, dtype=np.uint64) + np.uint64(sample0))[:, None], half, 1)
    w = philox4x32_10((p & MASK, p >> np.uint64(32), s & MASK, s >> np.uint64(32)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    a = (w[0] | w[1] << np.uint64(32)) >> np.uint64(11)
    b = (w[2] | w[3] << np.uint64(32)) >> np.uint64(11)
    u1 = (a + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (b + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    r, th = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    z = np.empty((nsamp, 2 * half))
    z[:, 0::2], z[:, 1::2] = r * np.cos(th), r * np.sin(th)
    return z[:, :n]

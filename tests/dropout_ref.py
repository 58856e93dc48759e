"""Reference of the dropout mask in numpy, independent of the package: Philox4x32-10 (Random123 constants) and
the mask definition of csrc/kernels/philox.h / ops/dropout.py.

  element e (row-major linear index, 64-bit): group g = e >> 3, counter (g & 0xffffffff, g >> 32, 0, 0),
  key (k0, k1) = (low, high) 32 bits of an int64; element j = e & 7 draws
  u = (w[j >> 1] >> (16 * (j & 1))) & 0xffff from the call's words w0..w3;
  thr = min(65535, round(p * 65536)); keep iff u >= thr; scale = 65536 / (65536 - thr) as fp32.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)

# Known answers for Philox4x32-10 (the Random123 distribution's kat_vectors): (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(c, k):
    """c: four uint64 arrays (or ints) holding 32-bit words, k: two; returns four uint64 arrays of 32-bit words.
    uint64 holds the full 32 x 32-bit products exactly."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in c)
    k0, k1 = (np.asarray(v, dtype=np.uint64) for v in k)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return c0, c1, c2, c3


def quantise(p):
    thr = min(65535, int(round(p * 65536)))
    return thr, np.float32(65536.0 / (65536 - thr))


def draws(numel, key):
    """uint16 draw of each of the elements 0..numel-1 under the int64 ``key`` (may be negative)."""
    k = int(key) & 0xFFFFFFFFFFFFFFFF
    e = np.arange(numel, dtype=np.uint64)      # the definition, element by element (one Philox call each)
    g, j = e >> np.uint64(3), e & np.uint64(7)
    zero = np.zeros_like(g)
    w = np.stack(philox4x32_10((g & MASK32, g >> np.uint64(32), zero, zero), (k & 0xFFFFFFFF, k >> 32)), axis=0)
    word = np.take_along_axis(w, (j >> np.uint64(1)).astype(np.int64)[None, :], axis=0)[0]
    return (word >> (np.uint64(16) * (j & np.uint64(1)))) & np.uint64(0xFFFF)


def keep_mask(numel, key, p):
    """bool[numel]: element e is kept."""
    return draws(numel, key) >= np.uint64(quantise(p)[0])

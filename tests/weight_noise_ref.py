"""Reference of the weight-noise draw (include/las_hip.h, las_weight_noise_apply), written from the definitions: a numpy
Philox4x32-10 and z(seed, step, i) -- the uniforms in fp32 (they are exact there), everything after them in float64.
Shared by test_weight_noise_cpu.py and test_weight_noise_gpu.py."""
import functools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
Z_MAX = float(np.sqrt(48.0 * np.log(2.0)))          # |z| <= sqrt(-2 ln 2^-24)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (anything that converts to uint64 words < 2^32) -> uint32 [..., 4]."""
    c = [np.asarray(ctr)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = (np.asarray(key)[..., k].astype(np.uint64) for k in range(2))
    mask, s32 = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # < 2^64: no wrap
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & mask, (p0 >> s32) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return np.stack(c, axis=-1).astype(np.uint32)


def words(seed, step, groups):
    """The four Philox words of each float4 group g: counter (g & 0xffffffff, g >> 32, step, 0), key (seed lo, seed hi)."""
    g = np.asarray(groups, dtype=np.uint64)
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & MASK
    ctr = np.stack([g & np.uint64(MASK), g >> np.uint64(32), np.full_like(g, step), np.zeros_like(g)], axis=-1)
    key = np.array([seed & MASK, seed >> 32], dtype=np.uint64)
    return philox4x32_10(ctr, np.broadcast_to(key, g.shape + (2,)))


def unit(x):
    """u(x) = ((x >> 9) + 0.5f) * 2^-23, formed in fp32 (exact)."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def z(seed, step, idx):
    """float64 z(seed, step, i) for an array of absolute flat indices i."""
    idx = np.asarray(idx, dtype=np.int64)
    g, inv = np.unique(idx >> 2, return_inverse=True)
    w = words(seed, step, g)
    u = unit(w).astype(np.float64)
    out = np.empty((g.size, 4), dtype=np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[:, a]))
        th = 2.0 * np.pi * u[:, a + 1]
        out[:, a], out[:, a + 1] = r * np.cos(th), r * np.sin(th)
    return out[inv.reshape(idx.shape), idx & 3]


def z_range(seed, step, start, count):
    return z(seed, step, np.arange(start, start + count, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def truncated_variance():
    """Variance of z on the exact grid of u: z = sqrt(-2 ln u_a) * cos|sin(2 pi u_b), u = (k + 0.5) * 2^-23, k < 2^23, both uniform
    on it and independent.  cos^2 and sin^2 average to exactly 1/2 over the equispaced u_b and the mean of z is 0 by symmetry, so
    var = mean_k(-ln u_k)  (= 1 - 24 ln2 2^-23 - ..., the integral of -ln over (0,1) by the midpoint rule), float64."""
    u = (np.arange(1 << 23, dtype=np.float64) + 0.5) * 2.0 ** -23
    return float(-np.log(u).mean())


KNOWN_ANSWERS = [        # (counter, key, output), Philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
MOMENT_CASES = [(0, 0), (0x100000007, 3)]            # (seed, step) of the moment tests, CPU and GPU
MOMENT_N = 1 << 20


def check_moments(zs):
    """The three conditions of the moment tests on n draws; returns (mean, var, max|z|) for printing."""
    zs = np.asarray(zs, dtype=np.float64)
    n = zs.size
    mean, var, big = float(zs.mean()), float(zs.var()), float(np.abs(zs).max())
    assert abs(mean) < 5.0 / np.sqrt(n), mean
    assert abs(var - truncated_variance()) < 5.0 * np.sqrt(2.0 / n), (var, truncated_variance())
    assert big <= 5.78, big
    return mean, var, big

"""Host reference of the device RNG (csrc/common.h vg_philox / vg_keep_block,
csrc/head.hip k_rng_fill): a vectorised numpy Philox4x32-10 (Salmon et al.,
SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
0xBB67AE85) and the project's counter layout on top of it.

Element t of a draw is lane ``t & 3`` of the block at counter
``(g lo, g hi, salt, iter lo)`` with ``g = t >> 2``, under key
``(seed lo, seed hi)``.  tests/test_philox_ref_cpu.py pins ``philox4x32_10`` to
the published known-answer vectors; tests/test_rng_gpu.py pins the kernels to
this module bit for bit.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (uint32 values, broadcast against each
    other) -> [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 -> 64 bits, no overflow
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def block(group, salt, iter, seed):
    """The four 32-bit words of element group(s) ``group`` (int or int array):
    counter (group lo, group hi, salt, iter lo), key (seed lo, seed hi)."""
    if isinstance(group, int):
        g = np.array([group & ((1 << 64) - 1)], dtype=np.uint64)
    else:
        g = np.atleast_1d(np.asarray(group, dtype=np.int64)).astype(np.uint64)
    ctr = np.empty(g.shape + (4,), dtype=np.uint64)
    ctr[..., 0] = g & _MASK
    ctr[..., 1] = g >> np.uint64(32)
    ctr[..., 2] = int(salt) & 0xFFFFFFFF
    ctr[..., 3] = int(iter) & 0xFFFFFFFF
    seed = int(seed) & ((1 << 64) - 1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox4x32_10(ctr, key)


def words(n, salt, iter, seed):
    """The first ``n`` 32-bit words of a draw, element order (uint32 [n])."""
    groups = (int(n) + 3) // 4
    return block(np.arange(groups, dtype=np.int64), salt, iter, seed).reshape(-1)[:int(n)]


def uniform(n, salt, iter, seed):
    """vg_rng_fill kind 1: (w >> 8) * 2^-24 in [0, 1), exact in float32."""
    return ((words(n, salt, iter, seed) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24))


def keep_mask(shape, p, salt, iter, seed):
    """vg_keep: Bernoulli(1 - p) / (1 - p) in float32 arithmetic, the float32
    ``1 - p`` formed from the float32 ``p`` as the kernel does."""
    n = int(np.prod(shape))
    u = uniform(n, salt, iter, seed)
    q = np.float32(1.0) - np.float32(p)
    inv = np.float32(1.0) / q
    return np.where(u < q, inv, np.float32(0.0)).astype(np.float32).reshape(shape)

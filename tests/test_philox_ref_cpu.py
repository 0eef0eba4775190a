"""tests/philox_ref.py against the published Philox4x32-10 known-answer vectors
(Random123 kat_vectors: counter || key -> output), and the counter layout,
lane order and float conversions the GPU tests rely on."""
import numpy as np
import pytest

import philox_ref

KAT = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _w(s):
    return [int(x, 16) for x in s.split()]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answer_vectors(ctr, key, want):
    got = philox_ref.philox4x32_10(_w(ctr), _w(key))
    assert [int(x) for x in got] == _w(want), " ".join(f"{int(x):08x}" for x in got)


def test_vectorised_equals_one_by_one():
    rs = np.random.RandomState(0)
    ctr = rs.randint(0, 1 << 32, size=(50, 4), dtype=np.uint64)
    key = rs.randint(0, 1 << 32, size=(50, 2), dtype=np.uint64)
    all_ = philox_ref.philox4x32_10(ctr, key)
    for i in range(50):
        assert np.array_equal(all_[i], philox_ref.philox4x32_10(ctr[i], key[i]))
    # the KAT rows through the batched path
    got = philox_ref.philox4x32_10([_w(c) for c, _, _ in KAT], [_w(k) for _, k, _ in KAT])
    assert got.tolist() == [_w(w) for _, _, w in KAT]


def test_block_counter_layout():
    """counter = (group lo, group hi, salt, iter lo), key = (seed lo, seed hi)."""
    seed, salt, it = 0x299F31D0A4093822, 0x13198A2E, 0x03707344
    g = (0x85A308D3 << 32) | 0x243F6A88
    assert [int(x) for x in philox_ref.block(g, salt, it, seed)[0]] == _w(KAT[2][2])
    # only the low word of the iteration counter enters
    assert np.array_equal(philox_ref.block(g, salt, it + (5 << 32), seed), philox_ref.block(g, salt, it, seed))
    # every field matters and no two are interchangeable
    base = philox_ref.block(3, 4, 5, 6)
    for other in (philox_ref.block(4, 4, 5, 6), philox_ref.block(3, 5, 5, 6), philox_ref.block(3, 4, 6, 6),
                  philox_ref.block(3, 4, 5, 7), philox_ref.block(3, 4, 5, 6 + (1 << 32)),
                  philox_ref.block(3, 5, 4, 6), philox_ref.block(3 + (1 << 32), 4, 5, 6)):
        assert not np.array_equal(base, other)


def test_words_and_uniform_lane_order():
    seed, salt, it = 0x123456789ABCDEF0, 0x40000001, 7
    w = philox_ref.words(11, salt, it, seed)
    assert w.dtype == np.uint32 and w.shape == (11,)
    for t in range(11):
        assert int(w[t]) == int(philox_ref.block(t >> 2, salt, it, seed)[0, t & 3])
    u = philox_ref.uniform(11, salt, it, seed)
    assert u.dtype == np.float32
    assert np.array_equal(u.astype(np.float64), (w >> 8).astype(np.float64) / 2.0 ** 24)  # exact in f32
    assert np.array_equal(philox_ref.uniform(5, salt, it, seed), u[:5])  # a prefix, whatever n


def test_keep_mask_values():
    shape, p = (257, 3), 0.2
    k = philox_ref.keep_mask(shape, p, 3, 1, 9)
    assert k.shape == shape and k.dtype == np.float32
    u = philox_ref.uniform(257 * 3, 3, 1, 9).reshape(shape)
    q = np.float32(1) - np.float32(p)
    assert np.array_equal(k != 0, u < q)
    assert set(np.unique(k).tolist()) == {0.0, float(np.float32(1) / q)}
    assert abs(float((k != 0).mean()) - 0.8) < 0.05

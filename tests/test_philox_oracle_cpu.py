"""The numpy Philox4x32-10 behind the dropout-mask oracle
(tests/philox_oracle.py) against the published known answers, plus the
stream addressing and mask conventions the GPU tests rely on."""

import numpy as np

import philox_oracle as po


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


# Random123's kat_vectors for philox4x32, 10 rounds
KNOWN = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF),
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
     (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def test_known_answers():
    for counter, key, want in KNOWN:
        assert _hex(po.philox4x32_10(counter, key)) == want


def test_array_counters_match_scalar_calls():
    rng = np.random.default_rng(0)
    cs = rng.integers(0, 2 ** 32, size=(4, 50), dtype=np.uint64)
    cs[:, 0] = KNOWN[2][0]
    out = po.philox4x32_10(tuple(cs), KNOWN[2][1])
    assert _hex([o[0] for o in out]) == KNOWN[2][2]
    for r in (1, 17, 49):
        one = po.philox4x32_10(tuple(int(c[r]) for c in cs), KNOWN[2][1])
        assert _hex([o[r] for o in out]) == _hex(one)


def test_stream_addressing():
    # seed = key (lo, hi); counter = {n lo, n hi, sub lo, sub hi}
    seed = 0x299F31D0A4093822
    sub = 0x0370734413198A2E
    n = 0x05A308D3243F6A88  # 4 n + 4 still fits 64 bits
    want = po.philox4x32_10((0x243F6A88, 0x05A308D3, 0x13198A2E, 0x03707344),
                            KNOWN[2][1])
    got = [po.stream_words(seed, sub, 4 * n + w) for w in range(4)]
    assert _hex(got) == _hex(want)
    # word 4 is the first word of the next counter
    nxt = po.philox4x32_10((0x243F6A89, 0x05A308D3, 0x13198A2E, 0x03707344),
                           KNOWN[2][1])
    assert int(po.stream_words(seed, sub, 4 * n + 4)) == int(nxt[0])
    # a 4-word draw at offset 1 straddles counters 0 and 1
    a = po.philox4x32_10((0, 0, 7, 0), (5, 0))
    b = po.philox4x32_10((1, 0, 7, 0), (5, 0))
    got = po.stream_words(5, np.full(4, 7), 1 + np.arange(4))
    assert [int(g) for g in got] == [int(a[1]), int(a[2]), int(a[3]),
                                     int(b[0])]


def test_uniform_is_float32_in_unit_interval():
    u = po.uniform(np.array([0, 1, 0x7FFFFFFF, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -32) and u[-1] == np.float32(1.0)
    assert (u > 0).all() and (u <= 1).all()
    # float32(v) rounds before the scale: 0x7fffffff -> 2^31 -> 0.5 + 2^-32
    # which float32 rounds to 0.5
    assert u[2] == np.float32(0.5)


def test_masks_shape_rate_and_keys():
    m2 = po.pool_mask(11, 0, 2, 0.25)
    m3 = po.fc1_mask(11, 0, 2, 0.5)
    assert m2.shape == (2, 64, 12, 12) and m2.dtype == np.uint8
    assert m3.shape == (2, 128) and m3.dtype == np.uint8
    assert abs(m2.mean() - 0.75) < 5 * np.sqrt(0.75 * 0.25 / m2.size)
    assert abs(m3.mean() - 0.5) < 5 * np.sqrt(0.25 / m3.size)
    # client-local indexing: a longer batch extends a shorter one
    assert np.array_equal(po.pool_mask(11, 0, 1, 0.25), m2[:1])
    assert np.array_equal(po.fc1_mask(11, 0, 1, 0.5), m3[:1])
    # batch index, seed (low and high word) all change the masks
    for other in (po.pool_mask(11, 1, 2, 0.25), po.pool_mask(12, 0, 2, 0.25),
                  po.pool_mask(11 + (1 << 32), 0, 2, 0.25)):
        assert not np.array_equal(other, m2)
    for other in (po.fc1_mask(11, 1, 2, 0.5), po.fc1_mask(12, 0, 2, 0.5),
                  po.fc1_mask(11 + (1 << 32), 0, 2, 0.5)):
        assert not np.array_equal(other, m3)
    # cell li reads lane li & 3 of draw (seed, li >> 2, t): batch t + 1
    # sees lanes 1..3 of batch t's counter in lanes 0..2
    w0 = po.stream_words(11, np.arange(8) >> 2, 0 + (np.arange(8) & 3))
    w1 = po.stream_words(11, np.arange(8) >> 2, 1 + (np.arange(8) & 3))
    assert np.array_equal(w0[1:4], w1[0:3]) and np.array_equal(w0[5:8],
                                                               w1[4:7])

"""Independent numpy oracle for the fused CNN's dropout masks.

Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2,
3", SC'11) and the two mask functions of csrc/fused_cnn.hip, written from
the documented contract of the device generator, not from the kernels:

* key = the 64-bit seed as (lo, hi);
* a generator initialised with ``(seed, subsequence, offset)`` yields the
  32-bit word stream of counters ``{n lo, n hi, subsequence lo,
  subsequence hi}``, n = 0, 1, ..., four words per counter, starting at
  word ``offset`` of that stream (counter ``offset // 4``, word
  ``offset % 4``; a 4-word draw runs on into the next counter);
* a word v becomes the uniform ``2^-32 + float32(v) * 2^-32`` in float32,
  i.e. a value in (0, 1];
* pool dropout: cell ``li`` (client-local index, row-major over
  [row, 64, 12, 12]) is kept iff lane ``li & 3`` of the 4-word draw
  ``(seed, li >> 2, t)`` is ``>= p1``;
* fc1 dropout: element ``li`` (row-major over [row, 128]) is kept iff the
  first word of ``(seed ^ 0x9e3779b97f4a7c15, li, t)`` is ``>= p2``;

with ``t`` the index of the batch within the client's epoch.
"""

import numpy as np

_M0 = np.uint64(0xD2511F53)
_M1 = np.uint64(0xCD9E8D57)
_W0 = 0x9E3779B9
_W1 = 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_GOLDEN = 0x9E3779B97F4A7C15
_TWO_POW_M32 = np.float32(2.0 ** -32)


def philox4x32_10(counter, key):
    """Ten Philox4x32 rounds.  ``counter`` is four integer arrays (or
    scalars) that broadcast together, ``key`` two Python ints.  Returns
    the four output words as uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(
        *[np.asarray(c, dtype=np.uint64) & _MASK32 for c in counter])
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = _M0 * c0          # < 2^64: both factors are below 2^32
        p1 = _M1 * c2
        hi0, lo0 = p0 >> _S32, p0 & _MASK32
        hi1, lo1 = p1 >> _S32, p1 & _MASK32
        c0, c1, c2, c3 = (hi1 ^ c1 ^ np.uint64(k0), lo1,
                          hi0 ^ c3 ^ np.uint64(k1), lo0)
        k0 = (k0 + _W0) & 0xFFFFFFFF
        k1 = (k1 + _W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def stream_words(seed, subsequence, position):
    """Word ``position`` of the stream ``(seed, subsequence)``;
    ``subsequence`` and ``position`` are non-negative integer arrays that
    broadcast together."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    sub = np.asarray(subsequence, dtype=np.uint64)
    pos = np.asarray(position, dtype=np.uint64)
    n = pos >> np.uint64(2)
    words = philox4x32_10((n & _MASK32, n >> _S32, sub & _MASK32,
                           sub >> _S32), (seed & 0xFFFFFFFF, seed >> 32))
    words = np.stack(np.broadcast_arrays(*words), axis=-1)
    lane = np.broadcast_to(pos & np.uint64(3), words.shape[:-1])
    return np.take_along_axis(words, lane[..., None].astype(np.int64),
                              axis=-1)[..., 0]


def uniform(words):
    """(0, 1] float32 uniforms of 32-bit words."""
    v = np.asarray(words, dtype=np.uint32).astype(np.float32)
    return _TWO_POW_M32 + v * _TWO_POW_M32


def pool_mask(seed, t, rows, p1):
    """Keep mask of the pool dropout, uint8 [rows, 64, 12, 12]."""
    li = np.arange(rows * 9216, dtype=np.uint64)
    u = uniform(stream_words(seed, li >> np.uint64(2),
                             np.uint64(t) + (li & np.uint64(3))))
    return (u >= np.float32(p1)).astype(np.uint8).reshape(rows, 64, 12, 12)


def epoch_masks(seed, p1, p2):
    """``masks(t, rows) -> (pool mask, fc1 mask)`` of one client epoch."""
    return lambda t, rows: (pool_mask(seed, t, rows, p1),
                            fc1_mask(seed, t, rows, p2))


def fc1_mask(seed, t, rows, p2):
    """Keep mask of the fc1 dropout, uint8 [rows, 128]."""
    li = np.arange(rows * 128, dtype=np.uint64)
    u = uniform(stream_words((int(seed) & 0xFFFFFFFFFFFFFFFF) ^ _GOLDEN,
                             li, np.uint64(t)))
    return (u >= np.float32(p2)).astype(np.uint8).reshape(rows, 128)

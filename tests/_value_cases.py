"""The input values that tests/test_values_cpu.py and tests/test_gpu_values.py
share: degenerate symbol classes, degenerate vectors for the transforms,
erasure patterns, and the spellings of a presence flag.  Pure numpy; loads no
library at import, so both modules test exactly the same bytes.

A symbol is 16 bits, stored high byte first (`be_bytes`), as the payload and the
shard rows hold it.  A symbol matrix is (positions, columns): position j of
column c is data position j of the c-th chunk of k symbols of a payload
(`payload_bytes`), or symbol c of row j of a shard buffer (`row_bytes`)."""
import numpy as np

CLASSES = ("zero", "ff", "sparse", "zero-tile", "zero-rows", "zero-columns")
SPARSE_VALUES = (0x0001, 0x8000, 0xFFFF, 0x0100)
TILE = 256  # columns per tile of the fast, small and resident kernels

VECTORS = ("zero", "ffff", "one", "first", "middle", "last", "half-zero")
ERASURES = ("random", "systematic-erased", "last-k-kept")

SPELLINGS = ("01", "ff", "80", "02", "mixed")


def zero_tile_columns(cols):
    """The columns the `zero-tile` class clears: the first tile, or the first
    64 columns where the rows hold a single tile."""
    return TILE if cols > TILE else min(64, cols)


def zero_column_index(cols):
    """The columns the `zero-columns` class clears."""
    return np.arange(0, cols, 7)


def symbols(name, rng, positions, cols):
    """A (positions, cols) uint16 matrix of class `name`; `zero-rows` clears
    every second position (1, 3, ...)."""
    if name == "zero":
        return np.zeros((positions, cols), np.uint16)
    if name == "ff":
        return np.full((positions, cols), 0xFFFF, np.uint16)
    if name == "sparse":
        m = np.zeros((positions, cols), np.uint16)
        c = np.arange(cols)
        m[c % positions, c] = np.asarray(SPARSE_VALUES, np.uint16)[c % len(SPARSE_VALUES)]
        return m
    m = rng.integers(0, 65536, (positions, cols), dtype=np.uint16)
    if name == "zero-tile":
        m[:, :zero_tile_columns(cols)] = 0
    elif name == "zero-rows":
        m[1::2] = 0
    elif name == "zero-columns":
        m[:, zero_column_index(cols)] = 0
    else:
        raise ValueError(name)
    return m


def be_bytes(m):
    """uint16 array -> uint8 array, last axis doubled, high byte first."""
    m = np.ascontiguousarray(m, dtype=np.uint16)
    return np.ascontiguousarray(m.astype(">u2")).view(np.uint8).reshape(m.shape[:-1] + (2 * m.shape[-1],))


def payload_bytes(m):
    """The payload whose data position j of column c is m[j, c]: cols * 2k bytes."""
    return be_bytes(np.ascontiguousarray(m.T)).reshape(-1)


def payload(name, rng, k, cols):
    return payload_bytes(symbols(name, rng, k, cols))


def received_rows(name, rng, n, cols, present):
    """(n, 2 * cols) bytes: the present rows carry class `name` (position j is
    the j-th present row), the absent rows random bytes that no decode may read."""
    idx = np.flatnonzero(present)
    rows = rng.integers(0, 256, (n, 2 * cols), dtype=np.uint8)
    if idx.size:
        rows[idx] = be_bytes(symbols(name, rng, idx.size, cols))
    return rows


def vector(name, rng, size):
    """A uint16 vector of `size` entries for the transforms and the codec hooks."""
    v = np.zeros(size, np.uint16)
    if name == "zero":
        return v
    if name == "ffff":
        v[:] = 0xFFFF
    elif name == "one":
        v[:] = 1
    elif name == "first":
        v[0] = 0x8001
    elif name == "middle":
        v[size // 2] = 0x0100
    elif name == "last":
        v[size - 1] = 0xFFFF
    elif name == "half-zero":
        v[size // 2:] = rng.integers(0, 65536, size - size // 2, dtype=np.uint16)
    else:
        raise ValueError(name)
    return v


def erasure(name, rng, n, k):
    """n flags, 1 = erased, at least k rows kept; None where the pattern does
    not exist for (n, k)."""
    er = np.zeros(n, np.uint8)
    if name == "random":
        er[rng.choice(n, int(rng.integers(1, n - k + 1)), replace=False)] = 1
    elif name == "systematic-erased":
        if n - k < k:
            return None
        er[:k] = 1
    elif name == "last-k-kept":
        er[:n - k] = 1
    else:
        raise ValueError(name)
    return er


def masks(rng, n, k, wn):
    """[(name, n flags 0/1)]: the five presence masks of one batch; rows at and
    above wanted_n stay 0."""
    def without(absent):
        p = np.zeros(n, np.uint8)
        p[:wn] = 1
        p[np.asarray(absent, dtype=np.int64)] = 0
        return p

    return [("more-than-k", without(rng.choice(wn, min((n - k) // 2, wn - k - 1), replace=False))),
            ("exactly-k", without(rng.choice(wn, wn - k, replace=False))),
            ("k-1", without(rng.choice(wn, wn - k + 1, replace=False))),
            ("one-systematic-absent", without([int(rng.integers(0, k))])),
            ("all-present", without([]))]


def spell(mask01, name):
    """The (batch, n) 0/1 mask with every present flag written as `name` says."""
    m = np.asarray(mask01, dtype=np.uint8)
    assert m.ndim == 2 and set(np.unique(m).tolist()) <= {0, 1}
    if name == "01":
        val = np.ones(m.shape, np.int64)
    elif name == "ff":
        val = np.full(m.shape, 0xFF, np.int64)
    elif name == "80":
        val = np.full(m.shape, 0x80, np.int64)
    elif name == "02":
        val = np.full(m.shape, 2, np.int64)
    elif name == "mixed":
        b, v = np.indices(m.shape)
        val = (37 * v + b) % 255 + 1
    else:
        raise ValueError(name)
    return np.where(m != 0, val, 0).astype(np.uint8)

"""The oracle on degenerate input values (tests/_value_cases.py), on the CPU.
tests/test_gpu_values.py compares the kernels with the oracle on these values,
and tests/test_oracle.py pins the oracle to the reference's C only on random
vectors, so the oracle is pinned here first:

- against the reference's own C build (`refc`) on zero, 0xFFFF, 1, one-hot and
  half-zero vectors through every transform and codec stage, under random
  erasures, every systematic row erased and only the last k rows kept;
- alone on every symbol class: a zero payload encodes to zeros, zero rows
  decode to zeros, and encode and reconstruct are GF(2)-linear -- the fact
  the sparse cases rest on (one symbol per column is one column of the code's
  matrix)."""
import numpy as np
import pytest

import _value_cases as vc

SIZES = tuple(1 << m for m in range(1, 13))  # 2 .. 4096
CODES = ((2, 1), (16, 8), (256, 64), (1024, 256), (4096, 256))
API_SHAPES = ((16, 8), (256, 64), (1024, 256))
COLS = 300


def test_oracle_vs_reference_c_degenerate(oracle, refc):
    rng = np.random.default_rng(287)
    cases = 0
    for size in SIZES:
        for name in vc.VECTORS:
            x = vc.vector(name, rng, size)
            for index in (0, size, 65536 - size):
                tag = (name, size, index)
                assert np.array_equal(oracle.afft(x, size, index), refc.afft(x, size, index)), tag
                assert np.array_equal(oracle.inverse_afft(x, size, index), refc.inverse_afft(x, size, index)), tag
                cases += 1
            assert np.array_equal(oracle.walsh(x), refc.walsh(x)), (name, size)
            assert np.array_equal(oracle.formal_derivative(x), refc.formal_derivative(x)), (name, size)
    for n, k in CODES:
        for name in vc.VECTORS:
            d = vc.vector(name, rng, k)
            cw = oracle.encode_low(d, k, n)
            assert np.array_equal(cw, refc.encode_low(d, k, n)), (name, n, k)
            if name == "zero":
                assert not cw.any(), (n, k)
            for pattern in vc.ERASURES:
                er = vc.erasure(pattern, rng, n, k)
                if er is None:
                    continue
                tag = (name, pattern, n, k)
                loc = oracle.eval_error_polynomial(er)
                assert np.array_equal(loc, refc.eval_error_polynomial(er)), tag
                # the received word: the codeword, and the degenerate vector itself (no codeword)
                for word in (cw, vc.vector(name, rng, n)):
                    c = word.copy()
                    c[er == 1] = 0
                    assert np.array_equal(oracle.decode_main(c, k, er, loc), refc.decode_main(c, k, er, loc)), tag
                cases += 1
    assert cases >= 287


def _masks(rng, n, k):
    out = []
    for name, pr in vc.masks(rng, n, k, n):
        if name != "k-1":
            out.append((name, pr))
    gone = np.ones(n, np.uint8)
    if n - k >= k:
        gone[:k] = 0
        out.append(("systematic-absent", gone))
    return out


def _recv(rows, pr):
    return [rows[v].tobytes() if pr[v] else None for v in range(len(pr))]


@pytest.mark.parametrize("n,k", API_SHAPES)
def test_zero_in_zero_out(oracle, n, k):
    rng = np.random.default_rng(n + k)
    st, shards = oracle.encode(bytes(vc.payload("zero", rng, k, COLS)), n, k, n)
    assert st == 0 and len(shards) == n and all(s == bytes(2 * COLS) for s in shards)
    for name, pr in _masks(rng, n, k):
        st, pay = oracle.reconstruct(_recv(vc.received_rows("zero", rng, n, COLS, pr), pr), n, k)
        assert st == 0 and pay == bytes(COLS * 2 * k), name


@pytest.mark.parametrize("n,k", API_SHAPES)
def test_encode_and_reconstruct_are_linear(oracle, n, k):
    rng = np.random.default_rng(3 * n + k)
    base = rng.integers(0, 256, COLS * 2 * k, dtype=np.uint8)
    st, enc_base = oracle.encode(bytes(base), n, k, n)
    assert st == 0
    enc_base = np.frombuffer(b"".join(enc_base), np.uint8)
    msk = _masks(rng, n, k)
    for i, name in enumerate(vc.CLASSES):
        a = vc.payload(name, rng, k, COLS)
        st, ea = oracle.encode(bytes(a), n, k, n)
        st2, ex = oracle.encode(bytes(a ^ base), n, k, n)
        assert st == 0 and st2 == 0
        ea, ex = (np.frombuffer(b"".join(e), np.uint8) for e in (ea, ex))
        assert np.array_equal(ex, ea ^ enc_base), name
        if name == "zero":
            assert not ea.any()
        mname, pr = msk[i % len(msk)]
        ra = vc.received_rows(name, rng, n, COLS, pr)
        rb = rng.integers(0, 256, ra.shape, dtype=np.uint8)
        pays = []
        for rows in (ra, rb, ra ^ rb):
            st, pay = oracle.reconstruct(_recv(rows, pr), n, k)
            assert st == 0
            pays.append(np.frombuffer(pay, np.uint8))
        assert np.array_equal(pays[2], pays[0] ^ pays[1]), (name, mname)
        if name == "zero":
            assert not pays[0].any()

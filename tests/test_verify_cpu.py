"""CPU tests of the shard-verifying entry points (np_verify_shards_batch_dev,
np_rs_verify_shards).

The first part states, on the oracle, the three facts the semantics of verify
rest on (include/novelpoly.h), so that the inputs of tests/test_gpu_verify.py
mean what that file says: with E = encode(reconstruct(received)),
 1. a present systematic row never differs from E;
 2. with exactly k present rows no row differs from E, random bytes included;
 3. with at least k + 1 present rows of a codeword, one altered symbol of a
    present row makes at least one present row differ from E.
The second part: the library exports the entry points, their validation runs
before any HIP call, and the header, the Rust binding and the Python wrappers
declare them (no GPU compute here)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import novelpoly_amd as npa
from _rs_front import CTX, N, check_front, outcome, params, poison, received

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("np_verify_shards_batch_dev", "np_rs_verify_shards")
SHAPES = [(256, 86), (600, 256), (60, 20), (16, 8), (1024, 512), (10, 4)]
SL = 2 * 5


def _mismatching(oracle, rows, pres, n, k, wn):
    recv = [rows[v].tobytes() if pres[v] else None for v in range(n)]
    st, pay = oracle.reconstruct(recv, n, k)
    assert st == 0
    st, enc = oracle.encode(pay, n, k, wn)
    assert st == 0 and len(enc[0]) == SL
    return [v for v in range(wn) if pres[v] and enc[v] != recv[v]]


def _codeword(oracle, rng, n, k, wn):
    st, shards = oracle.encode(rng.integers(0, 256, (SL // 2) * 2 * k - 1, dtype=np.uint8).tobytes(), n, k, wn)
    assert st == 0 and len(shards[0]) == SL
    rows = np.zeros((n, SL), np.uint8)
    rows[:wn] = np.stack([np.frombuffer(s, np.uint8) for s in shards])
    return rows


def _presence(rng, n, wn, count):
    p = np.zeros(n, np.uint8)
    p[rng.choice(wn, count, replace=False)] = 1
    return p


@pytest.mark.parametrize("nw,kw", SHAPES)
def test_exactly_k_rows_are_always_consistent(oracle, nw, kw):
    p = npa.CodeParams.derive_parameters(nw, kw)
    n, k, wn = p.n(), p.k(), p.wanted_n
    rng = np.random.default_rng(11 * nw + kw)
    for _ in range(3):
        rows = rng.integers(0, 256, (n, SL), dtype=np.uint8)
        assert _mismatching(oracle, rows, _presence(rng, n, wn, k), n, k, wn) == []


@pytest.mark.parametrize("nw,kw", SHAPES)
def test_systematic_rows_never_mismatch(oracle, nw, kw):
    """Random bytes with more than k rows present: many rows differ from the
    re-encoding, none of them below k."""
    p = npa.CodeParams.derive_parameters(nw, kw)
    n, k, wn = p.n(), p.k(), p.wanted_n
    rng = np.random.default_rng(13 * nw + kw)
    for count in (k + 1, (k + wn + 1) // 2, wn):
        rows = rng.integers(0, 256, (n, SL), dtype=np.uint8)
        bad = _mismatching(oracle, rows, _presence(rng, n, wn, count), n, k, wn)
        assert bad and all(v >= k for v in bad), (count, bad[:8])


@pytest.mark.parametrize("nw,kw", SHAPES)
def test_one_altered_symbol_shows_with_k_plus_1_rows(oracle, nw, kw):
    p = npa.CodeParams.derive_parameters(nw, kw)
    n, k, wn = p.n(), p.k(), p.wanted_n
    rng = np.random.default_rng(17 * nw + kw)
    code = _codeword(oracle, rng, n, k, wn)
    for count in (k + 1, k + 1, (k + wn + 1) // 2, wn):
        pres = _presence(rng, n, wn, count)
        assert _mismatching(oracle, code, pres, n, k, wn) == []
        for v in (int(rng.choice(np.flatnonzero(pres))), int(np.flatnonzero(pres)[0]), int(np.flatnonzero(pres)[-1])):
            rows = code.copy()
            rows[v, int(rng.integers(0, SL))] ^= np.uint8(1 << int(rng.integers(0, 8)))
            bad = _mismatching(oracle, rows, pres, n, k, wn)
            assert bad and all(r >= k for r in bad), (count, v, bad[:8])


def test_copy_mode_marks_exactly_the_altered_parity_rows(oracle):
    p = npa.CodeParams.derive_parameters(256, 86)
    n, k, wn = p.n(), p.k(), p.wanted_n
    rng = np.random.default_rng(19)
    rows = _codeword(oracle, rng, n, k, wn)
    pres = np.zeros(n, np.uint8)
    pres[:k] = 1
    pres[k + rng.choice(wn - k, (wn - k) // 2, replace=False)] = 1
    two = sorted(int(v) for v in rng.choice(np.flatnonzero(pres[k:]) + k, 2, replace=False))
    for v in two:
        rows[v, 3] ^= 0x40
    assert _mismatching(oracle, rows, pres, n, k, wn) == two


# ------------------------------------------------------------ the interface ----
def test_library_exports_the_verify_symbols():
    L = npa.lib()
    for name in NAMES:
        f = getattr(L, name)
        assert f.restype is C.c_int and f.argtypes, name
    assert len(L.np_verify_shards_batch_dev.argtypes) == 11 and len(L.np_rs_verify_shards.argtypes) == 7


def test_validation_runs_before_any_device_call():
    L = npa.lib()
    p = npa._Params(1024, 256, 1024)
    assert L.np_verify_shards_batch_dev(None, C.byref(p), None, 600, 1024 * 600, None, 1, None, None, None, None) == 100
    ptrs, lens, bad = (C.c_void_p * 1)(), (C.c_size_t * 1)(), C.c_size_t(0)
    assert L.np_rs_verify_shards(None, C.byref(p), ptrs, lens, 0, C.byref(bad), None) == 100
    with pytest.raises(npa.InvalidArgument):
        npa._raise(100)


def _dev(p, shards, present, bad, shard_len=600, stride=1024 * 600, mismatch=None, status=None):
    poison()
    return outcome(npa.lib().np_verify_shards_batch_dev(CTX, C.byref(p) if p is not None else None, shards, shard_len,
                                                        stride, present, 1, bad, mismatch, status, None))


def test_device_call_validation_order():
    """Every case returns before the context (a zero-filled stand-in) is touched;
    where two faults are present the earlier check's is reported."""
    buf = CTX
    p = npa._Params(1024, 256, 1024)
    inv = (100, (0, 0, 0))
    # the code: before a bad shard length and before NULL buffers
    assert _dev(None, buf, buf, buf) == inv
    assert _dev(npa._Params(1000, 300, 1000), None, None, None, shard_len=0) \
        == (npa.ParamterMustBePowerOf2.code, (1000, 300, 0))
    assert _dev(npa._Params(1024, 768, 1024), None, None, None, shard_len=0) == (100, (1024, 768, 1024))  # 2k > n
    assert _dev(npa._Params(1024, 256, 1025), buf, buf, buf, shard_len=601) == (100, (1024, 256, 1025))
    # a zero or odd shard length: before NULL buffers (the counts among them) and a short stride
    assert _dev(p, None, None, None, shard_len=0) == (npa.EmptyShard.code, (0, 0, 0))
    assert _dev(p, buf, buf, None, shard_len=601, stride=0) == (npa.EmptyShard.code, (0, 0, 0))
    # NULL buffers, a stride below n rows
    assert _dev(p, None, buf, buf) == inv
    assert _dev(p, buf, None, buf) == inv
    assert _dev(p, buf, buf, None) == inv
    assert _dev(p, buf, buf, None, mismatch=buf, status=buf) == inv
    assert _dev(p, buf, buf, buf, stride=1024 * 600 - 1) == inv


def _host(p, ptrs, lens, n_received, bad="count", mismatch=None):
    if bad == "count":
        bad = C.byref(C.c_size_t())
    return npa.lib().np_rs_verify_shards(CTX, C.byref(p) if p is not None else None, ptrs, lens, n_received, bad,
                                         mismatch)


def test_host_call_validates_the_received_set():
    check_front(_host)
    check_front(lambda *a: _host(*a, mismatch=CTX))


def test_host_call_rejects_null_bad_rows_first():
    """Before the code and before the count of the received shards."""
    ptrs, lens = received()
    for p, rx in ((params(), (ptrs, lens, N)), (params(12, 3, 12), (ptrs, lens, N)), (params(), (None, None, 0)),
                  (params(64, 16, 65), (ptrs, lens, N))):
        for mismatch in (None, CTX):
            poison()
            assert outcome(_host(p, *rx, bad=None, mismatch=mismatch)) == (100, (0, 0, 0))


def test_header_and_rust_binding_declare_them():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "novelpoly.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "rust", "novelpoly-mi355x", "src", "sys.rs")).read()
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "novelpoly-mi355x", "src", "lib.rs")).read()
    m = re.search(r"int np_verify_shards_batch_dev\(([^;]*?)\);", hdr, flags=re.S)
    assert m and "const uint8_t* d_shards" in m.group(1) and "uint32_t* d_bad_rows" in m.group(1)
    assert [a.split()[-1] for a in m.group(1).split(",")] == [
        "ctx", "params", "d_shards", "shard_len", "batch_stride", "d_present", "batch", "d_bad_rows", "d_mismatch",
        "d_status", "stream"]
    m = re.search(r"int np_rs_verify_shards\(([^;]*?)\);", hdr, flags=re.S)
    assert m and [a.split()[-1] for a in m.group(1).split(",")] == [
        "ctx", "params", "shards", "shard_lens", "n_received", "bad_rows", "mismatch"]
    for name in NAMES:
        assert f"pub fn {name}(" in rs, name
    assert "d_shards: *const u8" in rs[rs.index("pub fn np_verify_shards_batch_dev("):][:400]
    assert "pub fn verify<" in lib_rs and "pub fn mismatched_shards<" in lib_rs


def test_python_wrappers_exist():
    sig = inspect.signature(npa.verify_shards_batch_dev)
    assert list(sig.parameters) == ["params", "d_shards", "shard_len", "batch_stride", "d_present", "batch",
                                    "d_bad_rows", "ctx", "stream", "d_mismatch", "d_status"]
    assert list(inspect.signature(npa.ReedSolomon.verify).parameters) == ["self", "received"]
    assert list(inspect.signature(npa.ReedSolomon.mismatched_shards).parameters) == ["self", "received"]
    assert list(inspect.signature(npa.verify).parameters) == ["received", "validator_count", "ctx"]

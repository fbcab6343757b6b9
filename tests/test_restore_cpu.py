"""CPU tests of the shard-restoring entry points (np_restore_shards_batch_dev,
np_rs_restore_shards): the library exports them, their validation runs before
any HIP call, and the Python wrappers exist (no GPU compute here)."""
import ctypes as C
import inspect

import pytest

import novelpoly_amd as npa
from _rs_front import CTX, K, LEN, N, check_front, outcome, params, poison, received

NAMES = ("np_restore_shards_batch_dev", "np_rs_restore_shards")
SL, DN, DK = 600, 1024, 256  # the device call's cases


def _params(n, k, wanted_n):
    return npa._Params(n, k, wanted_n)


def test_library_exports_the_restore_symbols():
    L = npa.lib()
    for name in NAMES:
        f = getattr(L, name)
        assert f.restype is C.c_int and f.argtypes, name


def test_null_context_is_an_invalid_argument():
    L = npa.lib()
    p = _params(1024, 256, 1024)
    assert L.np_restore_shards_batch_dev(None, C.byref(p), None, 600, 1024 * 600, None, 1, None, None) == 100
    ptrs, lens = (C.c_void_p * 1)(), (C.c_size_t * 1)()
    outs = (C.c_void_p * 1)()
    assert L.np_rs_restore_shards(None, C.byref(p), ptrs, lens, 0, outs, 0) == 100
    with pytest.raises(npa.InvalidArgument):
        npa._raise(100)


def _dev(p, shards, present, shard_len=SL, stride=DN * SL, status=None):
    poison()
    return outcome(npa.lib().np_restore_shards_batch_dev(CTX, C.byref(p) if p is not None else None, shards, shard_len,
                                                         stride, present, 1, status, None))


def test_device_call_validation_order():
    """Every case returns before the context (a zero-filled stand-in) is touched;
    where two faults are present the earlier check's is reported."""
    buf = CTX
    p = _params(DN, DK, DN)
    inv = (100, (0, 0, 0))
    # the code: before a bad shard length and before NULL buffers
    assert _dev(None, buf, buf) == inv
    assert _dev(_params(1000, 300, 1000), None, None, shard_len=0) == (npa.ParamterMustBePowerOf2.code, (1000, 300, 0))
    assert _dev(_params(1024, 768, 1024), None, None, shard_len=0) == (100, (1024, 768, 1024))  # 2k > n
    assert _dev(_params(1024, 256, 1025), buf, buf, shard_len=SL + 1) == (100, (1024, 256, 1025))
    # a zero or odd shard length: before NULL buffers and a short stride
    assert _dev(p, None, None, shard_len=0) == (npa.EmptyShard.code, (0, 0, 0))
    assert _dev(p, buf, buf, shard_len=SL + 1, stride=0) == (npa.EmptyShard.code, (0, 0, 0))
    # NULL buffers, a stride below n rows
    assert _dev(p, None, buf) == inv
    assert _dev(p, buf, None) == inv
    assert _dev(p, buf, buf, stride=DN * SL - 1) == inv
    assert _dev(p, buf, buf, stride=DN * SL - 1, status=buf) == inv


def _host(p, ptrs, lens, n_received, restored="rows", restored_len=LEN):
    if restored == "rows":
        restored = (C.c_void_p * N)()
    return npa.lib().np_rs_restore_shards(CTX, C.byref(p) if p is not None else None, ptrs, lens, n_received, restored,
                                          restored_len)


def test_host_call_validates_the_received_set():
    check_front(_host)


def test_host_call_checks_its_rows_after_the_code():
    """NULL `restored` or a `restored_len` below the padded shard length: detail
    (that length), after the received set and the code."""
    ptrs, lens = received()
    for kw in (dict(restored=None), dict(restored_len=LEN - 1), dict(restored=None, restored_len=0)):
        poison()
        assert outcome(_host(params(), ptrs, lens, N, **kw)) == (100, (LEN, 0, 0)), kw
        poison()
        assert outcome(_host(params(64, 16, 65), ptrs, lens, N, **kw)) == (100, (64, 16, 65)), kw
        poison()
        assert outcome(_host(params(), *received(K - 1), N, **kw)) == (npa.NeedMoreShards.code, (K - 1, K, N)), kw
    # the padded length: LEN - 1 received bytes still ask for LEN
    ptrs, lens = received()
    for i in range(K):
        lens[i] = LEN - 1
    poison()
    assert outcome(_host(params(), ptrs, lens, N, restored_len=LEN - 1)) == (100, (LEN, 0, 0))


def test_python_wrappers_exist():
    sig = inspect.signature(npa.restore_shards_batch_dev)
    assert list(sig.parameters) == ["params", "d_shards", "shard_len", "batch_stride", "d_present", "batch", "ctx",
                                    "stream", "d_status"]
    assert list(inspect.signature(npa.ReedSolomon.restore_shards).parameters) == ["self", "received"]
    assert list(inspect.signature(npa.restore_shards).parameters) == ["received", "validator_count", "ctx"]

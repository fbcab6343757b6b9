"""CPU tests of the shard-restoring entry points (np_restore_shards_batch_dev,
np_rs_restore_shards): the library exports them, their validation runs before
any HIP call, and the Python wrappers exist (no GPU compute here)."""
import ctypes as C
import inspect

import pytest

import novelpoly_amd as npa

NAMES = ("np_restore_shards_batch_dev", "np_rs_restore_shards")


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


def test_python_wrappers_exist():
    sig = inspect.signature(npa.restore_shards_batch_dev)
    assert list(sig.parameters) == ["params", "d_shards", "shard_len", "batch_stride", "d_present", "batch", "ctx",
                                    "stream", "d_status"]
    assert list(inspect.signature(npa.ReedSolomon.restore_shards).parameters) == ["self", "received"]
    assert list(inspect.signature(npa.restore_shards).parameters) == ["received", "validator_count", "ctx"]

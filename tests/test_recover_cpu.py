"""CPU tests of the recover entry points (np_recover_batch_dev, np_rs_recover):
the library exports them, their validation runs before any HIP call, and the
Python wrappers exist (no GPU compute here).

The validation cases run against a zero-filled stand-in for the context: every
one of them returns before the context is touched, which is what they check."""
import ctypes as C
import inspect

import pytest

import novelpoly_amd as npa

NAMES = ("np_recover_batch_dev", "np_rs_recover")
SL, N, K = 600, 1024, 256
PAY = (SL // 2) * 2 * K


def _params(n=N, k=K, wanted_n=N):
    return npa._Params(n, k, wanted_n)


@pytest.fixture(scope="module")
def fake():
    """Non-NULL pointers that validation must not follow: (context, device buffer)."""
    ctx = C.create_string_buffer(1 << 16)
    buf = C.create_string_buffer(64)
    return C.cast(ctx, C.c_void_p), C.cast(buf, C.c_void_p)


def _call(ctx, p, shards, present, batch=1, shard_len=SL, stride=N * SL, out=None, out_stride=0, restore=0,
          bad=None, mismatch=None, status=None):
    return npa.lib().np_recover_batch_dev(ctx, C.byref(p), shards, shard_len, stride, present, batch, out, out_stride,
                                          restore, bad, mismatch, status, None)


def test_library_exports_the_recover_symbols():
    L = npa.lib()
    for name in NAMES:
        f = getattr(L, name)
        assert f.restype is C.c_int and f.argtypes, name
    assert len(L.np_recover_batch_dev.argtypes) == 14
    assert len(L.np_rs_recover.argtypes) == 12


def test_version_minor_is_bumped():
    major, minor = (int(x) for x in npa.version().split()[1].split(".")[:2])
    assert (major, minor) >= (0, 5)


def test_null_context_is_an_invalid_argument():
    L = npa.lib()
    p = _params()
    assert _call(None, p, None, None, restore=1) == 100
    ptrs, lens = (C.c_void_p * 1)(), (C.c_size_t * 1)()
    outs = (C.c_void_p * 1)()
    assert L.np_rs_recover(None, C.byref(p), ptrs, lens, 0, None, 0, None, outs, 0, None, None) == 100
    with pytest.raises(npa.InvalidArgument):
        npa._raise(100)


def test_device_call_validation_runs_before_any_launch(fake):
    ctx, buf = fake
    p = _params()
    # nothing requested
    assert _call(ctx, p, buf, buf) == 100
    # the map without the counts
    assert _call(ctx, p, buf, buf, mismatch=buf) == 100
    assert _call(ctx, p, buf, buf, restore=1, mismatch=buf) == 100
    # d_out with a stride below (shard_len / 2) * 2k
    assert _call(ctx, p, buf, buf, out=buf, out_stride=PAY - 1) == 100
    # the rest as np_restore_shards_batch_dev, in its order
    assert _call(ctx, p, buf, buf, restore=1, shard_len=0) == npa.EmptyShard.code
    assert _call(ctx, p, buf, buf, restore=1, shard_len=SL + 1) == npa.EmptyShard.code
    assert _call(ctx, p, None, buf, restore=1) == 100
    assert _call(ctx, p, buf, None, restore=1) == 100
    assert _call(ctx, p, buf, buf, restore=1, stride=N * SL - 1) == 100
    assert _call(ctx, _params(1024, 768, 1024), buf, buf, restore=1) == 100  # 2k > n
    # a bad code is reported before a bad shard length, as by the sibling calls
    assert _call(ctx, _params(1000, 300, 1000), buf, buf, restore=1, shard_len=0) == npa.ParamterMustBePowerOf2.code


def test_an_empty_batch_is_ok_and_launches_nothing(fake):
    ctx, buf = fake
    p = _params()
    for kw in (dict(restore=1), dict(out=buf, out_stride=PAY), dict(bad=buf), dict(bad=buf, mismatch=buf),
               dict(out=buf, out_stride=PAY, restore=1, bad=buf, mismatch=buf, status=buf)):
        assert _call(ctx, p, buf, buf, batch=0, **kw) == 0, kw
    # an empty batch is still validated
    assert _call(ctx, p, buf, buf, batch=0) == 100


def test_host_call_validation(fake):
    ctx, _ = fake
    L = npa.lib()
    p = _params(64, 16, 60)
    n, k = 64, 16
    row = C.create_string_buffer(b"\x01" * 10)
    ptrs, lens = (C.c_void_p * n)(), (C.c_size_t * n)()
    for i in range(k):
        ptrs[i], lens[i] = C.cast(row, C.c_void_p), 10
    out, olen, bad = C.create_string_buffer(10 * k), C.c_size_t(), C.c_size_t()
    outs = (C.c_void_p * n)()
    flags = C.create_string_buffer(n)
    pf = C.cast(flags, C.c_void_p)
    po = C.cast(out, C.c_void_p)
    # nothing requested; the map without the count
    assert L.np_rs_recover(ctx, C.byref(p), ptrs, lens, n, None, 0, None, None, 0, None, None) == 100
    assert L.np_rs_recover(ctx, C.byref(p), ptrs, lens, n, po, 10 * k, C.byref(olen), None, 0, None, pf) == 100
    # as np_rs_reconstruct: k - 1 shards, an empty shard, unequal lengths
    ptrs[k - 1] = None
    assert L.np_rs_recover(ctx, C.byref(p), ptrs, lens, n, None, 0, None, None, 0, C.byref(bad), None) == npa.NeedMoreShards.code
    ptrs[k - 1] = C.cast(row, C.c_void_p)
    lens[0] = 0
    assert L.np_rs_recover(ctx, C.byref(p), ptrs, lens, n, None, 0, None, None, 0, C.byref(bad), None) == npa.EmptyShard.code
    lens[0], lens[1] = 10, 6
    assert L.np_rs_recover(ctx, C.byref(p), ptrs, lens, n, None, 0, None, None, 0, C.byref(bad), None) \
        == npa.InconsistentShardLengths.code
    lens[1] = 10
    # the payload's capacity and length pointer, the restored rows' capacity
    assert L.np_rs_recover(ctx, C.byref(p), ptrs, lens, n, po, 10 * k - 1, C.byref(olen), None, 0, None, None) == 100
    assert L.np_rs_recover(ctx, C.byref(p), ptrs, lens, n, po, 10 * k, None, None, 0, None, None) == 100
    assert L.np_rs_recover(ctx, C.byref(p), ptrs, lens, n, None, 0, None, outs, 9, None, None) == 100


def test_python_wrappers_exist():
    sig = inspect.signature(npa.recover_batch_dev)
    assert list(sig.parameters) == ["params", "d_shards", "shard_len", "batch_stride", "d_present", "batch", "ctx",
                                    "stream", "d_out", "out_stride", "restore", "d_bad_rows", "d_mismatch", "d_status"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(ctx=None, stream=0, d_out=0, out_stride=0, restore=False, d_bad_rows=0, d_mismatch=0,
                            d_status=0)
    assert list(inspect.signature(npa.ReedSolomon.recover).parameters) == ["self", "received"]
    assert list(inspect.signature(npa.recover).parameters) == ["received", "validator_count", "ctx"]

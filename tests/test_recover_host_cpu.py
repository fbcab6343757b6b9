"""CPU tests of the host-memory recover entry points (np_recover_batch_host,
np_recover_batch_multi, np_recover_batch_host_multi): the library exports
them, their validation runs in the documented order before any HIP call, and
the Python wrappers exist (no GPU compute here).

The validation cases run against a zero-filled stand-in for the context: every
one of them returns before the context is touched, which is what they check."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import novelpoly_amd as npa

SL, N, K = 600, 1024, 256
PAY = (SL // 2) * 2 * K


def _params(n=N, k=K, wanted_n=N):
    return npa._Params(n, k, wanted_n)


@pytest.fixture(scope="module")
def fake():
    """Non-NULL pointers that validation must not follow: (context, host buffer)."""
    ctx = C.create_string_buffer(1 << 16)
    buf = C.create_string_buffer(64)
    return C.cast(ctx, C.c_void_p), C.cast(buf, C.c_void_p)


def _call(ctx, p, shards, present, batch=1, shard_len=SL, stride=N * SL, out=None, out_stride=0, restore=0,
          bad=None, mismatch=None, status=None):
    return npa.lib().np_recover_batch_host(ctx, C.byref(p) if p is not None else None, shards, shard_len, stride, present, batch, out, out_stride,
                                           restore, bad, mismatch, status)


def _detail():
    det = (C.c_size_t * 3)()
    npa.lib().np_last_error_detail(det)
    return tuple(det)


def test_library_exports_the_host_recover_symbols():
    """The parameter counts are those of the prototypes in include/novelpoly.h."""
    L = npa.lib()
    for name, count in (("np_recover_batch_host", 13), ("np_recover_batch_multi", 14),
                        ("np_recover_batch_host_multi", 14)):
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == count, name


def test_rust_crate_declares_the_calls():
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "integration", "rust", "novelpoly-mi355x", "src")
    sys_rs, lib_rs = open(os.path.join(src, "sys.rs")).read(), open(os.path.join(src, "lib.rs")).read()
    for name in ("np_recover_batch_host", "np_recover_batch_multi", "np_recover_batch_host_multi"):
        assert re.search(r"pub fn %s\s*\(" % name, sys_rs), name
    assert re.search(r"pub fn recover_batch_host\s*\(", lib_rs) and "sys::np_recover_batch_host(" in lib_rs


def test_version_minor_is_bumped():
    major, minor = (int(x) for x in npa.version().split()[1].split(".")[:2])
    assert (major, minor) >= (0, 7)


def test_validation_order(fake):
    ctx, buf = fake
    p = _params()
    # 1. a NULL context, whatever else is wrong
    assert _call(None, _params(1000, 300, 1000), None, None, shard_len=0) == 100
    # 2. the code: before a bad shard length, before NULL buffers
    assert _call(ctx, _params(1000, 300, 1000), buf, buf, restore=1, shard_len=0) == npa.ParamterMustBePowerOf2.code
    assert _call(ctx, _params(1024, 768, 1024), None, None, restore=1, shard_len=0) == 100  # 2k > n
    assert _call(ctx, None, buf, buf, restore=1) == 100
    # 3. a zero or odd shard length: before NULL buffers and before an empty request
    assert _call(ctx, p, None, None, shard_len=0) == npa.EmptyShard.code
    assert _call(ctx, p, buf, buf, restore=1, shard_len=SL + 1) == npa.EmptyShard.code
    # 4. NULL shards or present, a stride below n rows: before the request checks
    assert _call(ctx, p, None, buf, restore=1) == 100
    assert _call(ctx, p, buf, None, restore=1) == 100
    assert _call(ctx, p, buf, buf, restore=1, stride=N * SL - 1) == 100
    # 5. nothing requested; the map without the counts; out with a short stride
    assert _call(ctx, p, buf, buf) == 100
    assert _call(ctx, p, buf, buf, status=buf) == 100
    assert _call(ctx, p, buf, buf, mismatch=buf) == 100
    assert _call(ctx, p, buf, buf, restore=1, mismatch=buf) == 100
    assert _call(ctx, p, buf, buf, out=buf, out_stride=PAY - 1) == 100
    assert _call(ctx, p, buf, buf, out=buf, out_stride=PAY - 1, restore=1, bad=buf) == 100
    with pytest.raises(npa.InvalidArgument):
        npa._raise(100)


def test_an_empty_batch_is_ok_and_touches_nothing(fake):
    ctx, buf = fake
    p = _params()
    for kw in (dict(restore=1), dict(out=buf, out_stride=PAY), dict(bad=buf), dict(bad=buf, mismatch=buf),
               dict(out=buf, out_stride=PAY, restore=1, bad=buf, mismatch=buf, status=buf)):
        assert _call(ctx, p, buf, buf, batch=0, **kw) == 0, kw
    # an empty batch is still validated
    assert _call(ctx, p, buf, buf, batch=0) == 100


def test_short_payload_without_status_fails_up_front(fake):
    """status == NULL: the first payload with fewer than k present rows is the
    call's error, detail (have, k, n), before the context is touched."""
    ctx, buf = fake
    p = _params()
    pres = np.ones((3, N), np.uint8)
    pres[1, :N - K + 1] = 0  # k - 1 present
    pres[2, :N - K + 5] = 0  # a later, shorter one: not the one reported
    assert _call(ctx, p, buf, C.c_void_p(pres.ctypes.data), batch=3, restore=1) == npa.NeedMoreShards.code
    assert _detail() == (K - 1, K, N)
    with pytest.raises(npa.NeedMoreShards) as ei:
        npa._raise(npa.NeedMoreShards.code)
    assert ei.value == npa.NeedMoreShards(K - 1, K, N)
    # the request checks come first
    assert _call(ctx, p, buf, C.c_void_p(pres.ctypes.data), batch=3) == 100


def test_multi_forms_validate_their_contexts(fake):
    ctx, buf = fake
    L = npa.lib()
    p = _params()
    one = (C.c_void_p * 1)(buf.value)
    ctxs = (C.c_void_p * 1)(ctx.value)
    pres = np.ones((1, N), np.uint8)
    ppres = C.c_void_p(pres.ctypes.data)
    for c, nctx in ((None, 1), (ctxs, 0), (None, 0)):
        assert L.np_recover_batch_multi(c, nctx, C.byref(p), one, SL, N * SL, one, 1, None, 0, 1, None, None,
                                        None) == 100
        assert L.np_recover_batch_host_multi(c, nctx, C.byref(p), buf, SL, N * SL, ppres, 1, None, 0, 1, None, None,
                                             None) == 100
    # a NULL entry in the context array
    null_ctx = (C.c_void_p * 1)(None)
    assert L.np_recover_batch_multi(null_ctx, 1, C.byref(p), one, SL, N * SL, one, 1, None, 0, 1, None, None,
                                    None) == 100
    # the code is checked first, also at batch == 0
    bad = _params(1000, 300, 1000)
    assert L.np_recover_batch_multi(ctxs, 1, C.byref(bad), one, SL, N * SL, one, 0, None, 0, 1, None, None,
                                    None) == npa.ParamterMustBePowerOf2.code
    assert L.np_recover_batch_host_multi(ctxs, 1, C.byref(bad), buf, SL, N * SL, ppres, 0, None, 0, 1, None, None,
                                         None) == npa.ParamterMustBePowerOf2.code
    # the host form's mask check runs once over the whole batch, before any worker starts
    pres2 = np.ones((2, N), np.uint8)
    pres2[1, :N - K + 1] = 0
    assert L.np_recover_batch_host_multi(ctxs, 1, C.byref(p), buf, SL, N * SL, C.c_void_p(pres2.ctypes.data), 2, None,
                                         0, 1, None, None, None) == npa.NeedMoreShards.code
    assert _detail() == (K - 1, K, N)


def test_python_wrappers_exist():
    sig = inspect.signature(npa.recover_batch_host)
    assert list(sig.parameters) == ["params", "shards", "shard_len", "batch_stride", "present", "batch", "ctx", "out",
                                    "out_stride", "restore", "bad_rows", "mismatch", "status"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(ctx=None, out=0, out_stride=0, restore=False, bad_rows=0, mismatch=0, status=0)
    sig = inspect.signature(npa.recover_batch_multi)
    assert list(sig.parameters) == ["ctxs", "params", "d_shards", "shard_len", "batch_stride", "d_present", "batch",
                                    "d_out", "out_stride", "restore", "d_bad_rows", "d_mismatch", "d_status"]
    sig = inspect.signature(npa.recover_batch_host_multi)
    assert list(sig.parameters) == ["ctxs", "params", "shards", "shard_len", "batch_stride", "present", "batch", "out",
                                    "out_stride", "restore", "bad_rows", "mismatch", "status"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(out=0, out_stride=0, restore=False, bad_rows=0, mismatch=0, status=0)

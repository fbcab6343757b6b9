"""np_recover_ragged_dev on the host (no GPU): the library exports it, the
Python wrapper and the Rust declaration exist, and every status of its
validation is reached in the documented order (include/novelpoly.h): params and
items before the context (a NULL context reaches them), then the NULL context,
then the request, batch == 0 and the NULL buffers, which run against a
zero-filled stand-in for the context that none of them may touch.  With d_out
the items are np_reconstruct_ragged_dev's, without it payload_off and
payload_len hold garbage."""
import ctypes as C
import inspect
import os
import re

import pytest

import novelpoly_amd as npa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = npa.InvalidArgument.code

# n1024 k256, n128 k64, and a shape of the fallback path (k = 20 -> n64 k16)
SHAPES = [(1024, 342), (128, 64), (60, 20)]


@pytest.fixture(scope="module")
def fake():
    """Non-NULL pointers that validation must not follow: (context, device buffer)."""
    ctx = C.create_string_buffer(1 << 16)
    buf = C.create_string_buffer(64)
    return C.cast(ctx, C.c_void_p), C.cast(buf, C.c_void_p)


def _call(ctx, p, items, shards_size, shards=None, present=None, out=None, out_size=0, restore=0, bad=None,
          mismatch=None, status=None, batch=None):
    arr = None if items is None else npa._ragged_array(items)
    params = p if isinstance(p, npa._Params) else p._c()
    return npa.lib().np_recover_ragged_dev(ctx, C.byref(params), shards, shards_size, present, out, out_size, arr,
                                           len(items or ()) if batch is None else batch, restore, bad, mismatch,
                                           status, None)


def _one(p, **kw):
    """One valid item (300 columns, all n rows, output at offset 3) with fields
    replaced by `kw`; returns (items, shards_size, out_size), the sizes exact
    for the valid item."""
    it = dict(payload_off=3, payload_len=300 * 2 * p.k() - 5, shards_off=2, shard_len=600)
    ssize, osize = 2 + p.n() * 600, 3 + 300 * 2 * p.k()
    it.update(kw)
    return [(it["payload_off"], it["payload_len"], it["shards_off"], it["shard_len"])], ssize, osize


def test_symbol_wrapper_and_rust_declaration_exist():
    f = npa.lib().np_recover_ragged_dev
    assert f.restype is C.c_int and len(f.argtypes) == 14
    sig = inspect.signature(npa.recover_ragged_dev)
    assert list(sig.parameters) == ["params", "d_shards", "shards_size", "d_present", "items", "d_out", "out_size",
                                    "restore", "d_bad_rows", "d_mismatch", "d_status", "ctx", "stream"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(d_out=0, out_size=0, restore=False, d_bad_rows=0, d_mismatch=0, d_status=0, ctx=None,
                            stream=0)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "novelpoly-mi355x", "src", "sys.rs")).read()
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "novelpoly-mi355x", "src", "lib.rs")).read()
    assert re.search(r"pub fn np_recover_ragged_dev\s*\(", sys_rs)
    assert re.search(r"pub unsafe fn recover_ragged_dev\s*\(", lib_rs) and "sys::np_recover_ragged_dev(" in lib_rs


def test_version_minor_is_bumped():
    major, minor = (int(x) for x in npa.version().split()[1].split(".")[:2])
    assert (major, minor) >= (0, 6)


@pytest.mark.parametrize("with_out", [False, True])
@pytest.mark.parametrize("nw,kw", SHAPES)
def test_item_validation_through_a_null_context(fake, nw, kw, with_out):
    """ragged_masked_validate's statuses without d_out, np_reconstruct_ragged_dev's with it."""
    _, buf = fake
    p = npa.CodeParams.derive_parameters(nw, kw)

    def call(items, ss, osize=None, batch=None):
        if with_out:
            return _call(None, p, items, ss, out=buf, out_size=_one(p)[2] if osize is None else osize, restore=1,
                         batch=batch)
        return _call(None, p, items, ss, restore=1, batch=batch)

    # the extents exactly at the buffers' ends: the items pass, the NULL context is next
    items, ss, _ = _one(p)
    assert call(items, ss) == INVALID
    for sl in (0, 599, 1):
        assert call(_one(p, shard_len=sl)[0], ss) == npa.EmptyShard.code, sl
    good = _one(p)[0]
    odd = _one(p, shards_off=3)[0]
    bad_len = _one(p, shard_len=0)[0]
    # an odd shards_off (with room for it); told apart from the NULL context by the EmptyShard item around it:
    # items are validated in order, before the context and before batch == 0 is looked at
    assert call(odd, ss + 2) == INVALID
    assert call(good + odd + bad_len, ss + 2) == INVALID
    assert call(good + bad_len + odd, ss + 2) == npa.EmptyShard.code
    # one byte past the end of the shards; the rows counted are all n, not wanted_n
    for size in (ss - 1, 0) + ((2 + p.wanted_n * 600,) if p.wanted_n < p.n() else ()):
        assert call(good + bad_len, size) == INVALID, size  # not the second item's EmptyShard
    # offsets and lengths that wrap
    for kw_ in (dict(shards_off=2 ** 64 - 2), dict(shards_off=2 ** 63), dict(shard_len=2 ** 63),
                dict(shard_len=2 ** 64 - 2), dict(shard_len=2 ** 33 + 2)):
        assert call(_one(p, **kw_)[0] + bad_len, ss) == INVALID, kw_
    # no item array for a batch
    assert call(None, 0, batch=1) == INVALID


@pytest.mark.parametrize("nw,kw", SHAPES)
def test_payload_fields(fake, nw, kw):
    """Without d_out payload_off and payload_len are garbage; with it payload_off
    + (shard_len / 2) * 2k is checked against out_size and payload_len is still ignored."""
    _, buf = fake
    p = npa.CodeParams.derive_parameters(nw, kw)
    good, ss, osize = _one(p)
    bad_len = _one(p, shard_len=0)[0]  # behind a refused item it is never reached
    for poff, plen in ((2 ** 64 - 1, 2 ** 64 - 1), (0, 0), (2 ** 63 + 1, 5), (osize, 300 * 2 * p.k() + 77)):
        garbage = _one(p, payload_off=poff, payload_len=plen)[0]
        # accepted: the EmptyShard item behind it is reached
        assert _call(None, p, garbage + bad_len, ss, restore=1) == npa.EmptyShard.code, (poff, plen)
        assert _call(None, p, garbage, ss, bad=buf) == INVALID  # the NULL context
        if poff:
            assert _call(None, p, garbage + bad_len, ss, out=buf, out_size=osize, restore=1) == INVALID, (poff, plen)
    # payload_len alone is garbage with d_out too
    for plen in (0, 2 ** 64 - 1, 2 ** 63 + 1):
        items = _one(p, payload_len=plen)[0]
        assert _call(None, p, items + bad_len, ss, out=buf, out_size=osize) == npa.EmptyShard.code, plen
    # the output extent: exact, one byte short, an offset past out_size, an offset that wraps
    assert _call(None, p, good + bad_len, ss, out=buf, out_size=osize) == npa.EmptyShard.code
    assert _call(None, p, good + bad_len, ss, out=buf, out_size=osize - 1) == INVALID
    assert _call(None, p, _one(p, payload_off=osize + 1)[0] + bad_len, ss, out=buf, out_size=osize) == INVALID
    assert _call(None, p, _one(p, payload_off=2 ** 64 - 2)[0] + bad_len, ss, out=buf, out_size=osize) == INVALID
    # the same items without d_out: the output extent is not looked at
    assert _call(None, p, _one(p, payload_off=osize + 1)[0] + bad_len, ss, restore=1) == npa.EmptyShard.code


def test_validation_order(fake):
    """params, items, the context, the request, batch == 0, the buffers."""
    ctx, buf = fake
    p = npa.CodeParams.derive_parameters(1024, 342)
    bad = npa.CodeParams.derive_parameters(1024, 342)._c()
    bad.n, bad.k = 1000, 100  # neither a power of two
    empty = _one(p, shard_len=0)[0]
    good, ss, osize = _one(p)
    for kw in (dict(), dict(out=buf, out_size=osize)):
        # 1: params before items, items before everything else (NULL context, nothing requested, NULL buffers)
        assert _call(None, bad, empty, 0, **kw) == npa.ParamterMustBePowerOf2.code
        assert _call(None, p, empty, 0, **kw) == npa.EmptyShard.code
        assert _call(ctx, p, empty, 0, **kw) == npa.EmptyShard.code
        # 2: the NULL context before the request and before batch == 0's NP_OK
        assert _call(None, p, good, ss, shards=buf, present=buf, restore=1, **kw) == INVALID
        assert _call(None, p, [], 0, shards=buf, present=buf, restore=1, **kw) == INVALID
    # 3: nothing requested, the map without the counts -- at batch == 0 too, before its NP_OK
    for items, size in ((good, ss), ([], 0)):
        assert _call(ctx, p, items, size, shards=buf, present=buf) == INVALID
        assert _call(ctx, p, items, size, shards=buf, present=buf, mismatch=buf) == INVALID
        assert _call(ctx, p, items, size, shards=buf, present=buf, restore=1, mismatch=buf) == INVALID
        assert _call(ctx, p, items, size, shards=buf, present=buf, out=buf, out_size=osize, mismatch=buf) == INVALID
    # 4: batch == 0 with a valid request is NP_OK, before the NULL buffers are looked at
    for kw in (dict(restore=1), dict(out=buf, out_size=osize), dict(bad=buf), dict(bad=buf, mismatch=buf),
               dict(out=buf, out_size=0), dict(out=buf, out_size=osize, restore=1, bad=buf, mismatch=buf, status=buf)):
        assert _call(ctx, p, [], 0, **kw) == 0, kw
        assert _call(ctx, p, None, 0, batch=0, **kw) == 0, kw
    # 5: NULL d_shards or d_present
    for kw in (dict(restore=1), dict(bad=buf), dict(out=buf, out_size=osize)):
        assert _call(ctx, p, good, ss, shards=None, present=buf, **kw) == INVALID, kw
        assert _call(ctx, p, good, ss, shards=buf, present=None, **kw) == INVALID, kw


def test_wrapper_raises_the_validation_errors():
    p = npa.CodeParams.derive_parameters(1024, 342)
    good, ss, osize = _one(p)

    class NullCtx:
        handle = None

    with pytest.raises(npa.EmptyShard):
        npa.recover_ragged_dev(p, 0, ss, 0, _one(p, shard_len=0)[0], restore=True, ctx=NullCtx())
    with pytest.raises(npa.InvalidArgument):
        npa.recover_ragged_dev(p, 0, ss, 0, good, restore=True, ctx=NullCtx())

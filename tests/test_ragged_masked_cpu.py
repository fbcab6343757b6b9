"""np_restore_shards_ragged_dev / np_verify_shards_ragged_dev on the host (no
GPU): both calls validate the parameters and the items before they look at the
context, so every status of the validation is reached with a NULL context; a
valid item array then fails with the NULL context's NP_ERR_INVALID_ARGUMENT
(include/novelpoly.h).  payload_off and payload_len are not looked at."""
import ctypes as C
import os
import re

import pytest

import novelpoly_amd as npa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK_THEN_NULL_CTX = npa.InvalidArgument.code

# n1024 k256, n128 k64, and a shape of the fallback path (k = 20 -> n64 k16)
SHAPES = [(1024, 342), (128, 64), (60, 20)]


def _restore(p, items, shards_size, batch=None):
    arr = None if items is None else npa._ragged_array(items)
    return npa.lib().np_restore_shards_ragged_dev(None, C.byref(p._c()), None, shards_size, None, arr,
                                                  len(items or ()) if batch is None else batch, None, None)


def _verify(p, items, shards_size, batch=None):
    arr = None if items is None else npa._ragged_array(items)
    return npa.lib().np_verify_shards_ragged_dev(None, C.byref(p._c()), None, shards_size, None, arr,
                                                 len(items or ()) if batch is None else batch, None, None, None, None)


CALLS = [_restore, _verify]


def _one(p, **kw):
    """One valid item (300 columns, all n rows) with fields replaced by `kw`;
    returns (items, shards_size), the size exact for the valid item."""
    it = dict(payload_off=3, payload_len=300 * 2 * p.k() - 5, shards_off=2, shard_len=600)
    ssize = 2 + p.n() * 600
    it.update(kw)
    return [(it["payload_off"], it["payload_len"], it["shards_off"], it["shard_len"])], ssize


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("nw,kw", SHAPES)
def test_validation(nw, kw, call):
    p = npa.CodeParams.derive_parameters(nw, kw)
    # the extent exactly at the buffer's end: the items pass, the NULL context is next
    items, ss = _one(p)
    assert call(p, items, ss) == OK_THEN_NULL_CTX
    for sl in (0, 599, 1):
        items, ss = _one(p, shard_len=sl)
        assert call(p, items, ss) == npa.EmptyShard.code, sl
    # an odd shards_off (with room for it)
    items, ss = _one(p, shards_off=3)
    assert call(p, items, ss + 2) == npa.InvalidArgument.code
    # (the NULL context gives the same code: the two are told apart below, with a valid second item)
    good, ss = _one(p)
    odd, _ = _one(p, shards_off=3)
    bad_len, _ = _one(p, shard_len=0)
    # items are validated before the context and before batch == 0 is looked at: an EmptyShard item behind an
    # odd offset is never reached, one in front of it is
    assert call(p, good + odd + bad_len, ss + 2) == npa.InvalidArgument.code
    assert call(p, good + bad_len + odd, ss + 2) == npa.EmptyShard.code
    # one byte past the end; the rows counted are all n, not wanted_n
    items, ss = _one(p)
    for size in (ss - 1, 0) + ((2 + p.wanted_n * 600,) if p.wanted_n < p.n() else ()):
        assert call(p, items + bad_len, size) == npa.InvalidArgument.code, size  # not the second item's EmptyShard
    # offsets and lengths that wrap
    for kw_ in (dict(shards_off=2 ** 64 - 2), dict(shards_off=2 ** 63), dict(shard_len=2 ** 63),
                dict(shard_len=2 ** 64 - 2), dict(shard_len=2 ** 33 + 2)):
        items, ss = _one(p, **kw_)
        assert call(p, items + bad_len, ss) == npa.InvalidArgument.code, kw_
    # no item array for a batch
    assert call(p, None, 0, batch=1) == npa.InvalidArgument.code


@pytest.mark.parametrize("call", CALLS)
def test_validation_order(call):
    """params, then items, then the context, then batch == 0."""
    p = npa.CodeParams.derive_parameters(1024, 342)
    bad = npa.CodeParams.derive_parameters(1024, 342)._c()
    bad.n, bad.k = 1000, 100  # neither a power of two
    arr = npa._ragged_array(_one(p, shard_len=0)[0])
    L = npa.lib()
    if call is _restore:
        st = L.np_restore_shards_ragged_dev(None, C.byref(bad), None, 0, None, arr, 1, None, None)
    else:
        st = L.np_verify_shards_ragged_dev(None, C.byref(bad), None, 0, None, arr, 1, None, None, None, None)
    assert st == npa.ParamterMustBePowerOf2.code  # before the item's EmptyShard
    assert call(p, _one(p, shard_len=0)[0], 0) == npa.EmptyShard.code  # before the NULL context
    assert call(p, [], 0) == npa.InvalidArgument.code  # the NULL context, before batch == 0's NP_OK


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("nw,kw", SHAPES)
def test_payload_fields_are_ignored(nw, kw, call):
    """The encode's item array serves as it is, and so does one with garbage in
    payload_off / payload_len: both reach the NULL context."""
    p = npa.CodeParams.derive_parameters(nw, kw)
    k, n = p.k(), p.n()
    cols = [1, 300, 513]
    items, soff = [], 0
    for c in cols:
        items.append((7 * c, c * 2 * k - 1, soff, 2 * c))
        soff += n * 2 * c + 6
    ssize = soff - 6
    assert npa.ragged_plan(p, items, False, 7 * 513 + 513 * 2 * k, ssize)  # valid for the encode
    assert call(p, items, ssize) == OK_THEN_NULL_CTX
    for poff, plen in ((2 ** 64 - 1, 2 ** 64 - 1), (0, 0), (2 ** 63 + 1, 5), (1, 300 * 2 * k + 77)):
        garbage = [(poff, plen, so, sl) for (_, _, so, sl) in items]
        assert call(p, garbage, ssize) == OK_THEN_NULL_CTX, (poff, plen)
        with pytest.raises(npa.Error):  # the encode does look at them
            npa.ragged_plan(p, garbage, False, 7 * 513 + 513 * 2 * k, ssize)


def test_wrappers_and_rust_declarations_exist():
    assert callable(npa.restore_shards_ragged_dev) and callable(npa.verify_shards_ragged_dev)
    L = npa.lib()
    assert len(L.np_restore_shards_ragged_dev.argtypes) == 9
    assert len(L.np_verify_shards_ragged_dev.argtypes) == 11
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "novelpoly-mi355x", "src", "sys.rs")).read()
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "novelpoly-mi355x", "src", "lib.rs")).read()
    for name in ("np_restore_shards_ragged_dev", "np_verify_shards_ragged_dev"):
        assert re.search(r"pub fn " + name + r"\s*\(", sys_rs), name
        assert "sys::" + name + "(" in lib_rs, name

"""np_ragged_plan on the host (no GPU): the launch plan of the ragged direct
path and the validation that np_encode_ragged_dev / np_reconstruct_ragged_dev
share with it (include/novelpoly.h)."""
import numpy as np
import pytest

import novelpoly_amd as npa

TILE = 256


def _items(p, cols, recon, gap=6):
    """Items with `cols` columns each, packed with `gap` spare bytes between
    them; returns (items, payloads_size, shards_size), the sizes exact."""
    k, rows = p.k(), (p.n() if recon else p.wanted_n)
    items, poff, soff = [], 0, 0
    for c in cols:
        plen, sl = c * 2 * k, 2 * c
        items.append((poff, plen, soff, sl))
        poff += plen + gap + 1  # odd payload offsets too
        soff += rows * sl + gap
    last = items[-1]
    return items, last[0] + last[1], last[2] + rows * last[3]


# n1024 k256, n128 k64, and a shape of the fallback path (k = 20 -> n64 k16)
SHAPES = [(1024, 342), (128, 64), (60, 20)]


@pytest.mark.parametrize("nw,kw", SHAPES)
@pytest.mark.parametrize("recon", [False, True])
def test_plan(nw, kw, recon):
    p = npa.CodeParams.derive_parameters(nw, kw)
    rng = np.random.default_rng(nw + kw)
    cols = [1, 2, 255, 256, 257, 300, 512, 513, 4096, 700, 700] + [int(c) for c in rng.integers(1, 3000, 40)]
    items, psize, ssize = _items(p, cols, recon)
    plan = npa.ragged_plan(p, items, recon, psize, ssize)
    tiles = [(c + TILE - 1) // TILE for c in cols]
    real = [(i, it, t) for i, (it, t) in enumerate(plan) if it != npa.NO_ITEM]
    # every (item, tile) exactly once
    assert sorted((it, t) for _, it, t in real) == [(b, t) for b in range(len(cols)) for t in range(tiles[b])]
    # all blocks of an item on one residue mod 8
    res = {}
    for i, it, _ in real:
        res.setdefault(it, set()).add(i % 8)
    assert all(len(r) == 1 for r in res.values())
    # no-op blocks only as padding: behind the last real block of their residue
    last = {}
    for i, _, _ in real:
        last[i % 8] = max(last.get(i % 8, -1), i)
    for i, (it, _) in enumerate(plan):
        if it == npa.NO_ITEM:
            assert i > last.get(i % 8, -1), i
    assert plan[-1][0] != npa.NO_ITEM
    assert len(plan) <= sum(tiles) + 8 * max(tiles)
    # longest first onto the emptiest residue: the residues' loads differ by at most one item
    load = [0] * 8
    for i, _, _ in real:
        load[i % 8] += 1
    assert max(load) - min(load) <= max(tiles)


def test_plan_counts_without_tables():
    p = npa.CodeParams.derive_parameters(1024, 342)
    items, psize, ssize = _items(p, [300, 1, 513], False)
    arr = npa._ragged_array(items)
    import ctypes as C

    nb = C.c_size_t(0)
    st = npa.lib().np_ragged_plan(C.byref(p._c()), arr, 3, 0, psize, ssize, None, None, 0, C.byref(nb))
    assert st == 0 and nb.value == len(npa.ragged_plan(p, items, False, psize, ssize))
    bi = (C.c_uint32 * 2)()
    st = npa.lib().np_ragged_plan(C.byref(p._c()), arr, 3, 0, psize, ssize, bi, bi, 2, C.byref(nb))
    assert st == npa.InvalidArgument.code  # tables too small


def test_batch_zero():
    p = npa.CodeParams.derive_parameters(1024, 342)
    for recon in (False, True):
        assert npa.ragged_plan(p, [], recon, 0, 0) == []


def _real(plan):
    return sum(1 for it, _ in plan if it != npa.NO_ITEM)


def _one(p, recon, **kw):
    """One valid item (300 columns) with fields replaced by `kw`; returns
    (items, payloads_size, shards_size) with the sizes exact for the valid item."""
    k, rows = p.k(), (p.n() if recon else p.wanted_n)
    it = dict(payload_off=3, payload_len=300 * 2 * k - 5, shards_off=2, shard_len=600)
    psize = 3 + (300 * 2 * k if recon else it["payload_len"])
    ssize = 2 + rows * 600
    it.update(kw)
    return [(it["payload_off"], it["payload_len"], it["shards_off"], it["shard_len"])], psize, ssize


@pytest.mark.parametrize("nw,kw", SHAPES)
def test_validation(nw, kw):
    p = npa.CodeParams.derive_parameters(nw, kw)
    k = p.k()

    def plan1(recon, **kw):
        items, ps, ss = _one(p, recon, **kw)
        return npa.ragged_plan(p, items, recon, ps, ss)

    for recon in (False, True):
        # extents exactly at the buffer ends: accepted
        items, ps, ss = _one(p, recon)
        assert _real(npa.ragged_plan(p, items, recon, ps, ss)) == 2
        # one byte past either end: rejected
        with pytest.raises(npa.InvalidArgument):
            npa.ragged_plan(p, items, recon, ps - 1, ss)
        with pytest.raises(npa.InvalidArgument):
            npa.ragged_plan(p, items, recon, ps, ss - 1)
        with pytest.raises(npa.InvalidArgument):
            plan1(recon, payload_off=4)
        with pytest.raises(npa.InvalidArgument):
            plan1(recon, shards_off=4)
        # offsets that wrap
        with pytest.raises(npa.InvalidArgument):
            plan1(recon, payload_off=2 ** 64 - 1)
        with pytest.raises(npa.InvalidArgument):
            plan1(recon, shards_off=2 ** 64 - 2)
        # odd shards_off
        with pytest.raises(npa.InvalidArgument):
            plan1(recon, shards_off=1)
        # odd or zero shard_len
        for sl in (0, 599):
            with pytest.raises(npa.EmptyShard):
                plan1(recon, shard_len=sl)
        # the second item is validated too
        good, ps, ss = _one(p, recon)
        bad, _, _ = _one(p, recon, shard_len=0)
        with pytest.raises(npa.EmptyShard):
            npa.ragged_plan(p, good + bad, recon, ps, ss)
    # encode only: payload_len
    with pytest.raises(npa.PayloadSizeIsZero):
        plan1(False, payload_len=0)
    for plen in (300 * 2 * k + 1, 299 * 2 * k):  # shard_len does not match
        with pytest.raises(npa.InvalidArgument):
            items, ps, ss = _one(p, False, payload_len=plen)
            npa.ragged_plan(p, items, False, ps + 2 * k, ss)
    # reconstruct: payload_len is ignored
    items, ps, ss = _one(p, True, payload_len=0)
    assert _real(npa.ragged_plan(p, items, True, ps, ss)) == 2
    # any payload_off, odd ones included, is fine
    items, ps, ss = _one(p, False, payload_off=0)
    assert _real(npa.ragged_plan(p, items, False, ps, ss)) == 2


def test_calls_validate_before_any_device_work():
    """Without a context the ragged calls fail before they touch a device."""
    import ctypes as C

    p = npa.CodeParams.derive_parameters(1024, 342)
    L = npa.lib()
    assert L.np_encode_ragged_dev(None, C.byref(p._c()), None, 0, None, 0, None, 0, None) == npa.InvalidArgument.code
    assert L.np_reconstruct_ragged_dev(None, C.byref(p._c()), None, 0, None, None, 0, None, 0, None,
                                       None) == npa.InvalidArgument.code

"""np_restore_shards_ragged_dev / np_verify_shards_ragged_dev: restore and
verify on a batch whose items differ in length and sit anywhere in the caller's
shard buffer.  Every item must equal the uniform call on that item alone, which
is the reference's ReedSolomon::encode(ReedSolomon::reconstruct(received))
(mod.rs:117-157 after mod.rs:162-239): the absent rows below wanted_n, and the
present rows that differ from it, byte for byte against the oracle.  The
buffers are pre-filled with 0x5A and compared whole.

The batches are those of tests/test_gpu_ragged.py (items of 1, 2, 255, 256, 257,
300, 512 and 513 columns, out of order, gaps of 2 / 6 / 64 bytes, shard offsets
2 mod 16 or 128-aligned; batches of 8, 11 and 1).  Item i carries pattern
(i + rot) mod the number of patterns, the patterns being those of
tests/test_gpu_restore.py and tests/test_gpu_verify.py; rot 0 and 3 pair the
partial-tile items with different plans.  Direct shapes (k in {64, 128, 256},
n / k in {2, 4, 8}) run the ragged kernels, the others runs of the uniform
launches; the payload fields of the items are overwritten with garbage, which
both calls ignore."""
import functools

import numpy as np
import pytest

import novelpoly_amd as npa
from test_gpu_ragged import BATCHES, DIRECT, FALLBACK, FILL, SMALL_COLS, Case, _case, _diff, _encode, _host, _stream
from test_gpu_restore import _expected_rows
from test_gpu_verify import GUARD, UNDECODABLE, _expected_flags, _flip

pytestmark = pytest.mark.gpu

WIDE = (1024, 64)  # n1024 k64, n / k = 16: the masked encodes serve it, the ragged reconstruct does not
SHAPES = DIRECT + FALLBACK + [WIDE]
ROTS = [0, 3]


def _dev(a):
    """A device copy of `a` (the shared cases are read only: copied first)."""
    import torch

    return torch.from_numpy(np.array(a, copy=True)).cuda()


@functools.lru_cache(maxsize=None)
def _mcase(oracle, nw, kw, batch):
    if (nw, kw) != WIDE:
        return _case(oracle, nw, kw, batch)
    base = SMALL_COLS[(4096, 1366)]
    cols = {1: [base[5]], 8: list(base), 11: list(base) + [base[5], base[5], base[1]]}[batch]
    return Case(oracle, nw, kw, batch, cols=cols)


def _items(c):
    """The case's items with garbage in the payload fields."""
    return [(2 ** 64 - 1 - 3 * i, (2 ** 63 + i) if i % 2 else 0, so, sl) for i, (_, _, so, sl) in enumerate(c.items)]


def _codeword(c, i):
    """The oracle's encode of item i: rows below wanted_n, FILL above."""
    return c.item_rows(c.shards, i).copy()


def _pres_without(c, absent):
    p = np.zeros(c.n, np.uint8)
    p[:c.wn] = 1
    p[np.asarray(absent, dtype=np.int64)] = 0
    return p


def _segment_rows(c, rng, q):
    """Half of the rows (at least one) of segment q below wanted_n."""
    rows = np.arange(q * c.k, min((q + 1) * c.k, c.wn))
    return rng.choice(rows, max(1, len(rows) // 2), replace=False)


RESTORE_PATTERNS = ["random", "last-row", "one-segment", "two-segments", "systematic-few", "copy-mode", "exactly-k",
                    "k-1", "none-absent"]


def _restore_pattern(c, rng, i, name):
    """(rows n x sl, present n) of tests/test_gpu_restore.py::_patterns' pattern `name` for item i."""
    n, k, wn, sl = c.n, c.k, c.wn, c.items[i][3]
    last_seg = (wn - 1) // k  # the last segment with a row below wanted_n (>= 1)

    def rand_rows():
        return rng.integers(0, 256, (n, sl), dtype=np.uint8)

    if name == "random":
        return rand_rows(), _pres_without(c, rng.choice(wn, min((n - k) // 2, wn - k), replace=False))
    if name == "last-row":
        return _codeword(c, i), _pres_without(c, [wn - 1])
    if name == "one-segment":
        return _codeword(c, i), _pres_without(c, _segment_rows(c, rng, last_seg))
    if name == "two-segments":
        qs = [1, last_seg] if last_seg > 1 else [1]
        return _codeword(c, i), _pres_without(c, np.concatenate([_segment_rows(c, rng, q) for q in qs]))
    if name == "systematic-few":
        return _codeword(c, i), _pres_without(c, rng.choice(k, min(3, k), replace=False))
    if name == "copy-mode":  # all systematic rows present, the other present rows random
        rows = _codeword(c, i)
        rows[k:] = rng.integers(0, 256, (n - k, sl), dtype=np.uint8)
        return rows, _pres_without(c, k + rng.choice(wn - k, max(1, (wn - k) // 2), replace=False))
    if name == "exactly-k":
        return rand_rows(), _pres_without(c, rng.choice(wn, wn - k, replace=False))
    if name == "k-1":
        return rand_rows(), _pres_without(c, rng.choice(wn, wn - k + 1, replace=False))
    assert name == "none-absent"
    return rand_rows(), _pres_without(c, [])


VERIFY_PATTERNS = ["codeword", "last-symbol", "first-symbol", "tile-boundary", "copy-mode", "systematic-flip",
                   "random-exactly-k", "random", "k-1", "all-present"]


def _verify_pattern(c, rng, i, name):
    """(rows n x sl, present n) of tests/test_gpu_verify.py::_patterns' pattern `name` for item i."""
    n, k, wn, sl = c.n, c.k, c.wn, c.items[i][3]
    syms = sl // 2

    def rand_rows():
        return rng.integers(0, 256, (n, sl), dtype=np.uint8)

    def parity(p):  # present parity rows
        return np.flatnonzero(p[k:wn]) + k

    pres1 = _pres_without(c, rng.choice(wn, min((n - k) // 2, wn - k - 1), replace=False))
    rows = _codeword(c, i)
    if name == "codeword":
        return rows, pres1
    if name == "last-symbol":
        _flip(rows, int(rng.choice(parity(pres1))), syms - 1, rng)
        return rows, pres1
    if name == "first-symbol":
        _flip(rows, int(parity(pres1)[0]), 0, rng)
        return rows, pres1
    if name == "tile-boundary":  # columns 255 and 256 of two rows; narrower items: their last two columns
        two = rng.choice(parity(pres1), 2, replace=False)
        a, b = (255, 256) if syms > 256 else (max(0, syms - 2), syms - 1)
        _flip(rows, int(two[0]), a, rng)
        _flip(rows, int(two[1]), b, rng)
        return rows, pres1
    if name == "copy-mode":  # every systematic row, half of the parity rows, two of them altered
        pres = _pres_without(c, k + rng.choice(wn - k, (wn - k) // 2, replace=False))
        two = rng.choice(parity(pres), 2, replace=False)
        _flip(rows, int(two[0]), int(rng.integers(0, syms)), rng)
        _flip(rows, int(two[1]), int(rng.integers(0, syms)), rng)
        return rows, pres
    if name == "systematic-flip":  # a present systematic row altered while others are absent
        gone = rng.choice(k, min(3, k - 1), replace=False)
        _flip(rows, int(rng.choice(np.setdiff1d(np.arange(k), gone))), int(rng.integers(0, syms)), rng)
        return rows, _pres_without(c, gone)
    if name == "random-exactly-k":
        return rand_rows(), _pres_without(c, rng.choice(wn, wn - k, replace=False))
    if name == "random":
        return rand_rows(), pres1
    if name == "k-1":
        return rand_rows(), _pres_without(c, rng.choice(wn, wn - k + 1, replace=False))
    assert name == "all-present"
    return rows, _pres_without(c, [])


def _stage(c, per_item):
    """The shard buffer holding the present rows of `per_item` [(rows, present)], and the present flags."""
    buf = np.full(c.ssize, FILL, np.uint8)
    pres = np.stack([pr for _, pr in per_item])
    for i, (rows, pr) in enumerate(per_item):
        c.item_rows(buf, i)[pr != 0] = rows[pr != 0]
    return buf, pres


@functools.lru_cache(maxsize=None)
def _restore_case(oracle, nw, kw, batch, rot):
    """(names, shard buffer before, present, buffer after, [(status, have)]), computed once (read only)."""
    c = _mcase(oracle, nw, kw, batch)
    rng = np.random.default_rng(1000 * nw + kw + 13 * batch + rot)
    names = [RESTORE_PATTERNS[(i + rot) % len(RESTORE_PATTERNS)] for i in range(len(c.items))]
    per_item = [_restore_pattern(c, rng, i, names[i]) for i in range(len(c.items))]
    before, pres = _stage(c, per_item)
    want = before.copy()  # every byte but the restored rows stays as it was
    status = []
    for i, (rows, pr) in enumerate(per_item):
        exp = _expected_rows(oracle, rows, pr, c.n, c.k, c.wn, c.items[i][3])
        assert (exp is None) == (names[i] == "k-1"), names[i]
        status.append((npa.NeedMoreShards.code if exp is None else 0, int(pr.sum())))
        view = c.item_rows(want, i)
        for v, data in (exp or {}).items():
            view[v] = np.frombuffer(data, np.uint8)
    for a in (before, pres, want):
        a.setflags(write=False)
    return names, before, pres, want, status


def _check_restore(c, names, got, want, tag):
    for i, (_, _, so, sl) in enumerate(c.items):
        _diff(got[so:so + c.n * sl], want[so:so + c.n * sl], f"{tag}: item {i} ({c.cols[i]} columns, {names[i]})")
    _diff(got, want, f"{tag}: bytes outside the items")


@pytest.mark.parametrize("rot", ROTS)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("nw,kw", SHAPES)
def test_restore(gpu, oracle, nw, kw, batch, rot):
    import torch

    c = _mcase(oracle, nw, kw, batch)
    names, before, pres, want, status = _restore_case(oracle, nw, kw, batch, rot)
    dpres = _dev(pres)
    for with_status in (True, False):
        buf = _dev(before)
        st_d = torch.full((len(c.items), 2), -1, dtype=torch.int32, device="cuda")
        npa.restore_shards_ragged_dev(c.p, buf.data_ptr(), c.ssize, dpres.data_ptr(), _items(c), ctx=gpu,
                                      stream=_stream(), d_status=st_d.data_ptr() if with_status else 0)
        _check_restore(c, names, _host(buf), want, f"status buffer {with_status}")
        if with_status:
            stat = _host(st_d)
            assert [tuple(int(x) for x in r) for r in stat] == status
            errs = npa.payload_errors(c.p, stat)
            for i, (code, have) in enumerate(status):
                assert errs[i] == (npa.NeedMoreShards(have, c.k, c.n) if code else None), i
        else:
            assert bool((st_d == -1).all())


@functools.lru_cache(maxsize=None)
def _verify_case(oracle, nw, kw, batch, rot):
    """(names, shard buffer, present, flags batch x n, counts, [(status, have)]), computed once (read only)."""
    c = _mcase(oracle, nw, kw, batch)
    rng = np.random.default_rng(1000 * nw + kw + 17 * batch + rot)
    names = [VERIFY_PATTERNS[(i + rot) % len(VERIFY_PATTERNS)] for i in range(len(c.items))]
    per_item = [_verify_pattern(c, rng, i, names[i]) for i in range(len(c.items))]
    buf, pres = _stage(c, per_item)
    flags = np.zeros((len(c.items), c.n), np.uint8)
    counts, status = [], []
    for i, (rows, pr) in enumerate(per_item):
        exp = _expected_flags(oracle, rows, pr, c.n, c.k, c.wn, c.items[i][3])
        assert (exp is None) == (names[i] == "k-1"), names[i]
        if exp is None:
            counts.append(UNDECODABLE)
            status.append((npa.NeedMoreShards.code, int(pr.sum())))
            continue
        if names[i] in ("codeword", "random-exactly-k", "all-present"):
            assert not exp.any(), names[i]
        elif names[i] != "random":
            assert exp.any(), names[i]  # an altered symbol with > k rows present shows
        flags[i] = exp
        counts.append(int(exp.sum()))
        status.append((0, int(pr.sum())))
    for a in (buf, pres, flags):
        a.setflags(write=False)
    return names, buf, pres, flags, np.asarray(counts, np.uint32), status


def _run_verify(gpu, c, items, dbuf, dpres, with_status, with_map):
    """One call; returns (counts, map or None, status or None) after checking the guards around the results."""
    import torch

    batch = len(c.items)
    st_d = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
    cnt_d = torch.full((64 + 4 * batch + 64,), GUARD, dtype=torch.uint8, device="cuda")
    map_d = torch.full((64 + batch * c.n + 64,), GUARD, dtype=torch.uint8, device="cuda")
    npa.verify_shards_ragged_dev(c.p, dbuf.data_ptr(), c.ssize, dpres.data_ptr(), items, cnt_d.data_ptr() + 64, ctx=gpu,
                                 stream=_stream(), d_mismatch=map_d.data_ptr() + 64 if with_map else 0,
                                 d_status=st_d.data_ptr() if with_status else 0)
    cnt, mp, stat = _host(cnt_d), _host(map_d), _host(st_d)
    assert (cnt[:64] == GUARD).all() and (cnt[-64:] == GUARD).all()
    if with_map:
        assert (mp[:64] == GUARD).all() and (mp[-64:] == GUARD).all()
    else:
        assert (mp == GUARD).all()
    if not with_status:
        assert (stat == -1).all()
    return (cnt[64:-64].copy().view(np.uint32), mp[64:-64].reshape(batch, c.n) if with_map else None,
            stat if with_status else None)


@pytest.mark.parametrize("rot", ROTS)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("nw,kw", SHAPES)
def test_verify(gpu, oracle, nw, kw, batch, rot):
    c = _mcase(oracle, nw, kw, batch)
    names, buf, pres, want_flags, want_counts, status = _verify_case(oracle, nw, kw, batch, rot)
    dbuf, dpres = _dev(buf), _dev(pres)
    for with_status, with_map in ((True, True), (False, True), (True, False), (False, False)):
        tag = f"status {with_status}, map {with_map}"
        counts, mp, stat = _run_verify(gpu, c, _items(c), dbuf, dpres, with_status, with_map)
        wrong = [(int(i), names[i]) for i in np.flatnonzero(counts != want_counts)]
        assert counts.tolist() == want_counts.tolist(), (tag, "items whose count differs", wrong)
        if with_map:
            for i in range(len(c.items)):
                assert np.array_equal(mp[i], want_flags[i]), \
                    (tag, i, names[i], np.flatnonzero(mp[i]).tolist()[:8], np.flatnonzero(want_flags[i]).tolist()[:8])
        if with_status:
            assert [tuple(int(x) for x in r) for r in stat] == status, tag
            errs = npa.payload_errors(c.p, stat)
            for i, (code, have) in enumerate(status):
                assert errs[i] == (npa.NeedMoreShards(have, c.k, c.n) if code else None), (tag, i)
    _diff(_host(dbuf), buf, "the shard buffer is only read")


@pytest.mark.parametrize("nw,kw", SHAPES)
def test_round_trip(gpu, oracle, nw, kw):
    """The ragged encode, rows erased, the ragged restore with the encode's item
    array: the encode's output is back.  The ragged verify then finds nothing,
    and after one flipped byte what the oracle finds."""
    c = _mcase(oracle, nw, kw, 11)
    batch = len(c.items)
    enc = _encode(gpu, c)
    _diff(_host(enc), c.shards, "encode")
    rng = np.random.default_rng(3 * nw + kw)
    pres = np.zeros((batch, c.n), np.uint8)
    erased = c.shards.copy()
    for i in range(batch):
        pres[i, rng.choice(c.wn, c.k + int(rng.integers(0, c.wn - c.k + 1)), replace=False)] = 1
        c.item_rows(erased, i)[:c.wn][pres[i, :c.wn] == 0] = FILL
    buf = _dev(erased)
    npa.restore_shards_ragged_dev(c.p, buf.data_ptr(), c.ssize, _dev(pres).data_ptr(), c.items, ctx=gpu,
                                  stream=_stream())
    _diff(_host(buf), c.shards, "restore after the encode")
    allp = np.zeros((batch, c.n), np.uint8)
    allp[:, :c.wn] = 1
    dall = _dev(allp)
    counts, mp, stat = _run_verify(gpu, c, c.items, buf, dall, True, True)
    assert not counts.any() and not mp.any() and not stat[:, 0].any()
    # one byte of a parity row of an item with a partial second tile, and of the one-column item
    bad = c.shards.copy()
    want = np.zeros((batch, c.n), np.uint8)
    for i in (int(np.argmax(c.cols)), int(np.argmin(c.cols))):
        rows = c.item_rows(bad, i)
        v = int(rng.integers(c.k, c.wn))
        rows[v, int(rng.integers(0, rows.shape[1]))] ^= np.uint8(0x40)
        want[i] = _expected_flags(oracle, rows, allp[i], c.n, c.k, c.wn, rows.shape[1])
        assert want[i].any()
    counts, mp, _ = _run_verify(gpu, c, c.items, _dev(bad), dall, False, True)
    assert np.array_equal(mp, want) and counts.tolist() == want.sum(axis=1).tolist()


@pytest.mark.parametrize("nw,kw", [(1024, 342), (128, 64), (60, 20), (1024, 512)])
def test_equal_lengths_match_the_uniform_calls(gpu, nw, kw):
    """All lengths equal at a constant spacing: the bytes of np_restore_shards_batch_dev
    and np_verify_shards_batch_dev."""
    import torch

    p = npa.CodeParams.derive_parameters(nw, kw)
    n, k, wn = p.n(), p.k(), p.wanted_n
    batch, cols = 9, 300
    sl = 2 * cols
    bstride = n * sl + 2
    rng = np.random.default_rng(nw * kw + 1)
    # random bytes everywhere: absent rows and rows >= wanted_n hold ordinary bytes that must stay
    recv = _dev(rng.integers(0, 256, batch * bstride, dtype=np.uint8))
    pres = np.zeros((batch, n), np.uint8)
    for b in range(batch):
        pres[b, rng.choice(wn, min(wn, k - 1 + (b % 4) * (wn - k) // 3), replace=False)] = 1
    pres[1, :] = 0
    pres[1, :k] = 1  # copy mode
    pres[1, k + rng.choice(wn - k, (wn - k) // 2, replace=False)] = 1
    dpres = _dev(pres)
    items = [(0, 0, b * bstride, sl) for b in range(batch)]
    s = _stream()
    ra, rb = recv.clone(), recv.clone()
    sa = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
    sb = sa.clone()
    npa.restore_shards_batch_dev(p, ra.data_ptr(), sl, bstride, dpres.data_ptr(), batch, ctx=gpu, stream=s,
                                 d_status=sa.data_ptr())
    npa.restore_shards_ragged_dev(p, rb.data_ptr(), batch * bstride, dpres.data_ptr(), items, ctx=gpu, stream=s,
                                  d_status=sb.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(ra, rb) and torch.equal(sa, sb)
    assert not torch.equal(ra, recv)  # rows were restored
    assert int((sa[:, 0] != 0).sum()) >= 2  # the batch holds undecodable payloads too
    ca = torch.full((batch,), 7, dtype=torch.int32, device="cuda")
    cb = ca.clone()
    ma = torch.full((batch, n), GUARD, dtype=torch.uint8, device="cuda")
    mb = ma.clone()
    sa.fill_(-1)
    sb.fill_(-1)
    npa.verify_shards_batch_dev(p, recv.data_ptr(), sl, bstride, dpres.data_ptr(), batch, ca.data_ptr(), ctx=gpu,
                                stream=s, d_mismatch=ma.data_ptr(), d_status=sa.data_ptr())
    before = recv.clone()
    npa.verify_shards_ragged_dev(p, recv.data_ptr(), batch * bstride, dpres.data_ptr(), items, cb.data_ptr(), ctx=gpu,
                                 stream=s, d_mismatch=mb.data_ptr(), d_status=sb.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(ca, cb) and torch.equal(ma, mb) and torch.equal(sa, sb) and torch.equal(recv, before)
    assert bool(ma.any()) and int((ca == -1).sum()) >= 2  # mismatches, and UINT32_MAX for the undecodable ones


@pytest.mark.parametrize("nw,kw", [(1024, 342), (60, 20)])
def test_back_to_back_calls_keep_their_plans(gpu, oracle, nw, kw):
    """Two restores, then two verifies, queued on one stream with different
    items and no synchronisation in between: each call's plan, records and
    scratch must outlive the next call's."""
    import torch

    c1, c2 = _mcase(oracle, nw, kw, 11), _mcase(oracle, nw, kw, 8)
    r1, r2 = _restore_case(oracle, nw, kw, 11, 0), _restore_case(oracle, nw, kw, 8, 3)
    v1, v2 = _verify_case(oracle, nw, kw, 11, 0), _verify_case(oracle, nw, kw, 8, 3)
    s = _stream()
    b1, b2, p1, p2 = _dev(r1[1]), _dev(r2[1]), _dev(r1[2]), _dev(r2[2])
    w1, w2, q1, q2 = _dev(v1[1]), _dev(v2[1]), _dev(v1[2]), _dev(v2[2])
    n1 = torch.full((len(c1.items),), 7, dtype=torch.int32, device="cuda")
    n2 = torch.full((len(c2.items),), 7, dtype=torch.int32, device="cuda")
    m1 = torch.full((len(c1.items), c1.n), GUARD, dtype=torch.uint8, device="cuda")
    m2 = torch.full((len(c2.items), c2.n), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    npa.restore_shards_ragged_dev(c1.p, b1.data_ptr(), c1.ssize, p1.data_ptr(), _items(c1), ctx=gpu, stream=s)
    npa.restore_shards_ragged_dev(c2.p, b2.data_ptr(), c2.ssize, p2.data_ptr(), _items(c2), ctx=gpu, stream=s)
    npa.verify_shards_ragged_dev(c1.p, w1.data_ptr(), c1.ssize, q1.data_ptr(), _items(c1), n1.data_ptr(), ctx=gpu,
                                 stream=s, d_mismatch=m1.data_ptr())
    npa.verify_shards_ragged_dev(c2.p, w2.data_ptr(), c2.ssize, q2.data_ptr(), _items(c2), n2.data_ptr(), ctx=gpu,
                                 stream=s, d_mismatch=m2.data_ptr())
    _check_restore(c1, r1[0], _host(b1), r1[3], "first restore")
    _check_restore(c2, r2[0], _host(b2), r2[3], "second restore")
    assert _host(n1).view(np.uint32).tolist() == v1[4].tolist() and np.array_equal(_host(m1), v1[3]), "first verify"
    assert _host(n2).view(np.uint32).tolist() == v2[4].tolist() and np.array_equal(_host(m2), v2[3]), "second verify"


def test_batch_zero_and_null_pointers_on_the_device_calls(gpu):
    p = npa.CodeParams.derive_parameters(1024, 342)
    s = _stream()
    npa.restore_shards_ragged_dev(p, 0, 0, 0, [], ctx=gpu, stream=s)
    npa.verify_shards_ragged_dev(p, 0, 0, 0, [], 0, ctx=gpu, stream=s)
    size = p.n() * 2
    buf = _dev(np.full(size, FILL, np.uint8))
    pres = _dev(np.ones(p.n(), np.uint8))
    cnt = _dev(np.full(4, FILL, np.uint8))
    one = [(0, 0, 0, 2)]
    d, pr, ct = buf.data_ptr(), pres.data_ptr(), cnt.data_ptr()
    for args in ((0, size, pr), (d, size, 0)):
        with pytest.raises(npa.InvalidArgument):
            npa.restore_shards_ragged_dev(p, *args, one, ctx=gpu, stream=s)
    for args in ((0, size, pr, one, ct), (d, size, 0, one, ct), (d, size, pr, one, 0)):
        with pytest.raises(npa.InvalidArgument):
            npa.verify_shards_ragged_dev(p, *args, ctx=gpu, stream=s)
    with pytest.raises(npa.InvalidArgument):  # the shard extent ends one byte past the buffer
        npa.restore_shards_ragged_dev(p, d, size - 1, pr, one, ctx=gpu, stream=s)
    with pytest.raises(npa.EmptyShard):
        npa.verify_shards_ragged_dev(p, d, size, pr, [(0, 0, 0, 3)], ct, ctx=gpu, stream=s)
    # none of the refused calls wrote anything
    assert bool((buf == FILL).all()) and bool((cnt == FILL).all())
    # the same buffers in a valid call: every row present, d_shards only read; the fill is no codeword, so only the
    # count's range (present parity rows) is known
    npa.verify_shards_ragged_dev(p, d, size, pr, one, ct, ctx=gpu, stream=s)
    assert int(_host(cnt).view(np.uint32)[0]) <= p.wanted_n - p.k()
    assert bool((buf == FILL).all())

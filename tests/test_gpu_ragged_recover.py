"""np_recover_ragged_dev: the payload, the absent rows and the verdict of a
ragged batch from one decode.  Every requested output of item i must equal,
byte for byte, the reference's ReedSolomon::reconstruct (mod.rs:162-239) and
ReedSolomon::encode(reconstruct(received)) (mod.rs:117-157) on that item alone,
against the oracle: the payload at d_out + payload_off, the absent rows below
wanted_n, the flags of the present rows that differ and their count.  All
buffers are pre-filled and compared whole: an output that was not requested
keeps its fill, and without the restore the shard buffer is unchanged.

The batches are those of tests/test_gpu_ragged.py (items of 1, 2, 255, 256, 257,
300, 512 and 513 columns, out of order, with gaps, odd payload offsets, shard
offsets 2 mod 16 or 128-aligned; batches of 8, 11 and 1), the shapes those of
tests/test_gpu_ragged_masked.py.  Item i carries pattern (i + rot) mod
len(PATTERNS), drawn from the restore and verify pattern lists of that module,
each holding absent rows and altered present rows together where the pattern
allows it; rot 0 and 3 pair the partial-tile items with different plans.
Without d_out the payload fields of the items hold garbage; with it only
payload_len does."""
import functools
import itertools

import numpy as np
import pytest

import novelpoly_amd as npa
from _stream_gate import Gate, run_gated
from test_gpu_ragged import BATCHES, FILL, _diff, _host, _stream
from test_gpu_ragged_masked import (ROTS, SHAPES, _dev, _items, _mcase, _restore_pattern, _stage, _verify_pattern)
from test_gpu_verify import GUARD, UNDECODABLE, _flip

pytestmark = pytest.mark.gpu

# (list, name): "r" of RESTORE_PATTERNS, "v" of VERIFY_PATTERNS.  The first four serve every batch of 8 at rot 0.
PATTERNS = [("v", "last-symbol"), ("r", "copy-mode"), ("r", "exactly-k"), ("r", "k-1"), ("v", "tile-boundary"),
            ("r", "one-segment"), ("v", "copy-mode"), ("v", "systematic-flip"), ("r", "random"), ("v", "first-symbol"),
            ("r", "two-segments"), ("v", "random"), ("r", "last-row"), ("v", "codeword"), ("r", "systematic-few"),
            ("v", "random-exactly-k"), ("r", "none-absent"), ("v", "all-present"), ("v", "k-1")]
CODEWORD_RESTORES = ("last-row", "one-segment", "two-segments", "systematic-few")  # present rows intact: one is altered

# (d_out, restore, verify): the seven non-empty requests
COMBOS = [c for c in itertools.product((False, True), repeat=3) if any(c)]


def _pattern(c, rng, i, which, name):
    if which == "v":
        return _verify_pattern(c, rng, i, name)
    rows, pres = _restore_pattern(c, rng, i, name)
    parity = np.flatnonzero(pres[c.k:c.wn]) + c.k
    if name in CODEWORD_RESTORES and parity.size:
        _flip(rows, int(rng.choice(parity)), int(rng.integers(0, c.items[i][3] // 2)), rng)
    return rows, pres


def _out_items(c):
    """The case's items with garbage in payload_len alone."""
    return [(po, (2 ** 63 + i) if i % 2 else 0, so, sl) for i, (po, _, so, sl) in enumerate(c.items)]


class Expected:
    pass


def expected_items(oracle, c, names, per_item):
    """The staged buffers of the items `per_item` [(rows, present)] of case `c`
    and the oracle's answer for each item alone."""
    n, k, wn = c.n, c.k, c.wn
    e = Expected()
    e.names = names
    e.before, e.pres = _stage(c, per_item)
    e.restored = e.before.copy()  # every byte but the restored rows stays as it was
    e.out = np.full(c.psize, GUARD, np.uint8)
    e.flags = np.zeros((len(c.items), n), np.uint8)
    counts, e.status = [], []
    for i, (rows, pr) in enumerate(per_item):
        po, _, _, sl = c.items[i]
        recv = [rows[v].tobytes() if pr[v] else None for v in range(n)]
        st, pay = oracle.reconstruct(recv, n, k)
        assert (st != 0) == (int(pr.sum()) < k), names[i]
        if st:
            assert st == npa.NeedMoreShards.code
            counts.append(UNDECODABLE)
            e.status.append((st, int(pr.sum())))
            continue
        assert len(pay) == (sl // 2) * 2 * k
        e.out[po:po + len(pay)] = np.frombuffer(pay, np.uint8)
        st, enc = oracle.encode(pay, n, k, wn)
        assert st == 0 and len(enc) == wn and all(len(row) == sl for row in enc)
        view = c.item_rows(e.restored, i)
        for v in range(wn):
            if not pr[v]:
                view[v] = np.frombuffer(enc[v], np.uint8)
            elif enc[v] != recv[v]:
                e.flags[i, v] = 1
        counts.append(int(e.flags[i].sum()))
        e.status.append((0, int(pr.sum())))
    e.counts = np.asarray(counts, np.uint32)
    return e


@functools.lru_cache(maxsize=None)
def _recover_case(oracle, nw, kw, batch, rot):
    """The staged buffers and the oracle's answers, computed once (read only)."""
    c = _mcase(oracle, nw, kw, batch)
    rng = np.random.default_rng(1000 * nw + kw + 19 * batch + rot)
    names = [PATTERNS[(i + rot) % len(PATTERNS)] for i in range(len(c.items))]
    e = expected_items(oracle, c, names, [_pattern(c, rng, i, *names[i]) for i in range(len(c.items))])
    for name, (st, _) in zip(names, e.status):
        assert (st != 0) == (name[1] == "k-1"), name
    for a in (e.before, e.pres, e.restored, e.out, e.flags):
        a.setflags(write=False)
    return e


def _call(gpu, c, dbefore, dpres, with_out, restore, verify, with_status, with_map):
    """One call on a copy of `dbefore`; returns (shards, out, counts, map, status) on the host, guards checked."""
    import torch

    batch = len(c.items)
    buf = dbefore.clone()
    st_d = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
    cnt_d = torch.full((64 + 4 * batch + 64,), GUARD, dtype=torch.uint8, device="cuda")
    map_d = torch.full((64 + batch * c.n + 64,), GUARD, dtype=torch.uint8, device="cuda")
    out_d = torch.full((64 + c.psize + 64,), GUARD, dtype=torch.uint8, device="cuda")
    npa.recover_ragged_dev(c.p, buf.data_ptr(), c.ssize, dpres.data_ptr(), _out_items(c) if with_out else _items(c),
                           d_out=out_d.data_ptr() + 64 if with_out else 0, out_size=c.psize if with_out else 0,
                           restore=restore, d_bad_rows=cnt_d.data_ptr() + 64 if verify else 0,
                           d_mismatch=map_d.data_ptr() + 64 if with_map else 0,
                           d_status=st_d.data_ptr() if with_status else 0, ctx=gpu, stream=_stream())
    got, out, cnt, mp, stat = _host(buf), _host(out_d), _host(cnt_d), _host(map_d), _host(st_d)
    for a in (out, cnt, mp):
        assert (a[:64] == GUARD).all() and (a[-64:] == GUARD).all()
    return got, out[64:-64], cnt[64:-64].copy(), mp[64:-64].reshape(batch, c.n), stat


def _check(c, e, res, with_out, restore, verify, with_status, with_map, tag):
    got, out, cnt, mp, stat = res
    want = e.restored if restore else e.before
    for i, (_, _, so, sl) in enumerate(c.items):
        _diff(got[so:so + c.n * sl], want[so:so + c.n * sl], f"{tag}: item {i} ({c.cols[i]} columns, {e.names[i]})")
    _diff(got, want, f"{tag}: shard bytes outside the items")
    if with_out:
        for i, (po, _, _, sl) in enumerate(c.items):
            ln = (sl // 2) * 2 * c.k
            _diff(out[po:po + ln], e.out[po:po + ln], f"{tag}: payload {i} ({c.cols[i]} columns, {e.names[i]})")
        _diff(out, e.out, f"{tag}: output bytes outside the items")
    else:
        assert (out == GUARD).all(), tag
    if verify:
        counts = cnt.view(np.uint32)
        wrong = [(int(i), e.names[i]) for i in np.flatnonzero(counts != e.counts)]
        assert counts.tolist() == e.counts.tolist(), (tag, "items whose count differs", wrong)
    else:
        assert (cnt == GUARD).all(), tag
    if with_map:
        for i in range(len(c.items)):
            assert np.array_equal(mp[i], e.flags[i]), \
                (tag, i, e.names[i], np.flatnonzero(mp[i]).tolist()[:8], np.flatnonzero(e.flags[i]).tolist()[:8])
    else:
        assert (mp == GUARD).all(), tag
    if with_status:
        assert [tuple(int(x) for x in r) for r in stat] == e.status, tag
        errs = npa.payload_errors(c.p, stat)
        for i, (code, have) in enumerate(e.status):
            assert errs[i] == (npa.NeedMoreShards(have, c.k, c.n) if code else None), (tag, i)
    else:
        assert (stat == -1).all(), tag


@pytest.mark.parametrize("rot", ROTS)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("nw,kw", SHAPES)
def test_recover(gpu, oracle, nw, kw, batch, rot):
    c = _mcase(oracle, nw, kw, batch)
    e = _recover_case(oracle, nw, kw, batch, rot)
    dbefore, dpres = _dev(e.before), _dev(e.pres)
    for (with_out, restore, verify), with_status, with_map in itertools.product(COMBOS, (True, False), (True, False)):
        if with_map and not verify:
            continue
        tag = f"out {with_out}, restore {restore}, verify {verify}, status {with_status}, map {with_map}"
        res = _call(gpu, c, dbefore, dpres, with_out, restore, verify, with_status, with_map)
        _check(c, e, res, with_out, restore, verify, with_status, with_map, tag)
    _diff(_host(dbefore), e.before, "the staged buffer")


def test_patterns_cover_the_special_items(oracle):
    """Every batch of 8 holds a copy-mode, an exactly-k and a NeedMoreShards item at rot 0."""
    head = [name for _, name in PATTERNS[:8]]
    assert {"copy-mode", "exactly-k", "k-1"} <= set(head)
    e = _recover_case(oracle, 128, 64, 8, 0)
    assert (e.counts == UNDECODABLE).sum() == 1 and e.flags.any() and not np.array_equal(e.restored, e.before)


@pytest.mark.parametrize("nw,kw", [(1024, 342), (128, 64), (60, 20), (1024, 512)])
def test_equal_lengths_match_the_uniform_call(gpu, nw, kw):
    """All lengths equal at constant spacings: the bytes of np_recover_batch_dev."""
    import torch

    p = npa.CodeParams.derive_parameters(nw, kw)
    n, k, wn = p.n(), p.k(), p.wanted_n
    batch, cols = 9, 300
    sl = 2 * cols
    bstride = n * sl + 2
    pay_len = cols * 2 * k
    ostride = pay_len + 3  # odd output addresses
    rng = np.random.default_rng(nw * kw + 2)
    recv = _dev(rng.integers(0, 256, batch * bstride, dtype=np.uint8))
    pres = np.zeros((batch, n), np.uint8)
    for b in range(batch):
        pres[b, rng.choice(wn, min(wn, k - 1 + (b % 4) * (wn - k) // 3), replace=False)] = 1
    pres[1, :] = 0
    pres[1, :k] = 1  # copy mode
    pres[1, k + rng.choice(wn - k, (wn - k) // 2, replace=False)] = 1
    dpres = _dev(pres)
    items = [(1 + b * ostride, 0, b * bstride, sl) for b in range(batch)]
    s = _stream()

    def outputs():
        return (recv.clone(), torch.full((1 + batch * ostride,), GUARD, dtype=torch.uint8, device="cuda"),
                torch.full((batch,), 7, dtype=torch.int32, device="cuda"),
                torch.full((batch, n), GUARD, dtype=torch.uint8, device="cuda"),
                torch.full((batch, 2), -1, dtype=torch.int32, device="cuda"))

    for with_out, restore, verify in COMBOS:
        ba, oa, ca, ma, sa = outputs()
        bb, ob, cb, mb, sb = outputs()
        npa.recover_batch_dev(p, ba.data_ptr(), sl, bstride, dpres.data_ptr(), batch, ctx=gpu, stream=s,
                              d_out=oa.data_ptr() + 1 if with_out else 0, out_stride=ostride if with_out else 0,
                              restore=restore, d_bad_rows=ca.data_ptr() if verify else 0,
                              d_mismatch=ma.data_ptr() if verify else 0, d_status=sa.data_ptr())
        npa.recover_ragged_dev(p, bb.data_ptr(), batch * bstride, dpres.data_ptr(), items,
                               d_out=ob.data_ptr() if with_out else 0, out_size=1 + batch * ostride if with_out else 0,
                               restore=restore, d_bad_rows=cb.data_ptr() if verify else 0,
                               d_mismatch=mb.data_ptr() if verify else 0, d_status=sb.data_ptr(), ctx=gpu, stream=s)
        torch.cuda.synchronize()
        tag = (with_out, restore, verify)
        assert torch.equal(ba, bb) and torch.equal(oa, ob) and torch.equal(sa, sb), tag
        assert torch.equal(ca, cb) and torch.equal(ma, mb), tag
        assert torch.equal(ba, recv) != restore, tag  # rows were restored exactly when asked
        assert bool((oa == GUARD).all()) != with_out, tag
        assert int((sa[:, 0] != 0).sum()) >= 2, tag  # the batch holds undecodable payloads too
        if verify:
            assert bool(ma.any()) and int((ca == -1).sum()) >= 2, tag


@pytest.mark.parametrize("nw,kw", [(1024, 342), (512, 64), (60, 20)])
def test_equals_the_three_ragged_calls(gpu, oracle, nw, kw):
    """Random, non-codeword bytes in every row: np_reconstruct_ragged_dev,
    np_restore_shards_ragged_dev and np_verify_shards_ragged_dev on copies of the
    buffer give exactly the new call's outputs."""
    import torch

    c = _mcase(oracle, nw, kw, 11)
    batch, n, k, wn = len(c.items), c.n, c.k, c.wn
    rng = np.random.default_rng(7 * nw + kw)
    before = _dev(rng.integers(0, 256, c.ssize, dtype=np.uint8))
    pres = np.zeros((batch, n), np.uint8)
    for b in range(batch):
        pres[b, rng.choice(wn, k + int(rng.integers(0, wn - k + 1)) if b != 4 else k - 1, replace=False)] = 1
    pres[2, :] = 0
    pres[2, :k] = 1  # copy mode
    pres[2, k + rng.choice(wn - k, (wn - k) // 2, replace=False)] = 1
    dpres = _dev(pres)
    s = _stream()

    def outputs():
        return (torch.full((c.psize,), GUARD, dtype=torch.uint8, device="cuda"),
                torch.full((batch,), 7, dtype=torch.int32, device="cuda"),
                torch.full((batch, n), GUARD, dtype=torch.uint8, device="cuda"),
                torch.full((batch, 2), -1, dtype=torch.int32, device="cuda"))

    out_a, cnt_a, map_a, st_a = outputs()
    st_r, st_v = st_a.clone(), st_a.clone()
    buf_r = before.clone()
    npa.reconstruct_ragged_dev(c.p, before.data_ptr(), c.ssize, dpres.data_ptr(), out_a.data_ptr(), c.psize, c.items,
                               ctx=gpu, stream=s, d_status=st_a.data_ptr())
    npa.verify_shards_ragged_dev(c.p, before.data_ptr(), c.ssize, dpres.data_ptr(), c.items, cnt_a.data_ptr(), ctx=gpu,
                                 stream=s, d_mismatch=map_a.data_ptr(), d_status=st_v.data_ptr())
    npa.restore_shards_ragged_dev(c.p, buf_r.data_ptr(), c.ssize, dpres.data_ptr(), c.items, ctx=gpu, stream=s,
                                  d_status=st_r.data_ptr())
    out_b, cnt_b, map_b, st_b = outputs()
    buf_b = before.clone()
    npa.recover_ragged_dev(c.p, buf_b.data_ptr(), c.ssize, dpres.data_ptr(), c.items, d_out=out_b.data_ptr(),
                           out_size=c.psize, restore=True, d_bad_rows=cnt_b.data_ptr(), d_mismatch=map_b.data_ptr(),
                           d_status=st_b.data_ptr(), ctx=gpu, stream=s)
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b) and torch.equal(buf_r, buf_b)
    assert torch.equal(cnt_a, cnt_b) and torch.equal(map_a, map_b)
    assert torch.equal(st_a, st_b) and torch.equal(st_r, st_b) and torch.equal(st_v, st_b)
    # the batch is not trivial: rows were written, rows mismatch, one item is undecodable
    assert not torch.equal(buf_b, before) and bool(map_b.any()) and int(cnt_b[4]) == -1
    assert int((st_b[:, 0] != 0).sum()) == 1 and not bool((out_b == GUARD).all())


@pytest.mark.parametrize("nw,kw", [(1024, 342), (60, 20)])
def test_back_to_back_calls_keep_their_plans(gpu, oracle, nw, kw):
    """Four calls with different requests and items queued on one stream with no
    synchronisation in between: each call's plan, records and scratch must
    outlive the next call's.  A gate in front (tests/_stream_gate.py) keeps the
    first call from starting before the last one is enqueued."""
    import torch

    c1, c2 = _mcase(oracle, nw, kw, 11), _mcase(oracle, nw, kw, 8)
    e1, e2 = _recover_case(oracle, nw, kw, 11, 0), _recover_case(oracle, nw, kw, 8, 3)
    s = _stream()
    requests = [(c1, e1, True, True, True), (c2, e2, False, True, True), (c1, e1, True, False, True),
                (c2, e2, True, True, False)]

    def case(gate_ms):
        held = []
        for c, e, with_out, restore, verify in requests:
            batch = len(c.items)
            held.append((_dev(e.before), _dev(e.pres), torch.full((c.psize,), GUARD, dtype=torch.uint8, device="cuda"),
                         torch.full((4 * batch,), GUARD, dtype=torch.uint8, device="cuda"),
                         torch.full((batch, c.n), GUARD, dtype=torch.uint8, device="cuda"),
                         torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")))
        torch.cuda.synchronize()
        g = Gate(torch.cuda.current_stream(), gate_ms)
        for (c, e, with_out, restore, verify), (buf, pr, out, cnt, mp, st) in zip(requests, held):
            npa.recover_ragged_dev(c.p, buf.data_ptr(), c.ssize, pr.data_ptr(), _out_items(c) if with_out else _items(c),
                                   d_out=out.data_ptr() if with_out else 0, out_size=c.psize if with_out else 0,
                                   restore=restore, d_bad_rows=cnt.data_ptr() if verify else 0,
                                   d_mismatch=mp.data_ptr() if verify else 0, d_status=st.data_ptr(), ctx=gpu, stream=s)
        ms, premise = g.host_ms(), g.open()
        for j, ((c, e, with_out, restore, verify), (buf, pr, out, cnt, mp, st)) in enumerate(zip(requests, held)):
            res = (_host(buf), _host(out), _host(cnt), _host(mp), _host(st))
            _check(c, e, res, with_out, restore, verify, True, verify, f"call {j}")
        return premise, ms

    run_gated(case, label=f"ragged recover back to back {nw},{kw}")


def test_batch_zero_and_null_pointers_on_the_device_call(gpu):
    p = npa.CodeParams.derive_parameters(1024, 342)
    s = _stream()
    size = p.n() * 2
    osize = 2 * p.k()
    buf = _dev(np.full(size, FILL, np.uint8))
    pres = _dev(np.ones(p.n(), np.uint8))
    cnt = _dev(np.full(4, FILL, np.uint8))
    mp = _dev(np.full(p.n(), FILL, np.uint8))
    out = _dev(np.full(osize, FILL, np.uint8))
    d, pr, ct, m, o = buf.data_ptr(), pres.data_ptr(), cnt.data_ptr(), mp.data_ptr(), out.data_ptr()
    one = [(0, 0, 0, 2)]
    # batch 0: NP_OK with a request, refused without one
    npa.recover_ragged_dev(p, 0, 0, 0, [], restore=True, ctx=gpu, stream=s)
    npa.recover_ragged_dev(p, 0, 0, 0, [], d_bad_rows=ct, ctx=gpu, stream=s)
    npa.recover_ragged_dev(p, 0, 0, 0, [], d_out=o, out_size=osize, ctx=gpu, stream=s)
    with pytest.raises(npa.InvalidArgument):
        npa.recover_ragged_dev(p, 0, 0, 0, [], ctx=gpu, stream=s)
    with pytest.raises(npa.InvalidArgument):
        npa.recover_ragged_dev(p, 0, 0, 0, [], restore=True, d_mismatch=m, ctx=gpu, stream=s)
    # NULL d_shards / d_present, nothing requested, the map without the counts
    for kw in (dict(d_shards=0, d_present=pr, restore=True), dict(d_shards=d, d_present=0, restore=True),
               dict(d_shards=d, d_present=pr), dict(d_shards=d, d_present=pr, d_out=o, out_size=osize, d_mismatch=m)):
        with pytest.raises(npa.InvalidArgument):
            npa.recover_ragged_dev(p, kw.pop("d_shards"), size, kw.pop("d_present"), one, ctx=gpu, stream=s, **kw)
    with pytest.raises(npa.InvalidArgument):  # the shard extent ends one byte past the buffer
        npa.recover_ragged_dev(p, d, size - 1, pr, one, restore=True, ctx=gpu, stream=s)
    with pytest.raises(npa.InvalidArgument):  # the output extent ends one byte past the buffer
        npa.recover_ragged_dev(p, d, size, pr, one, d_out=o, out_size=osize - 1, restore=True, ctx=gpu, stream=s)
    with pytest.raises(npa.EmptyShard):
        npa.recover_ragged_dev(p, d, size, pr, [(0, 0, 0, 3)], d_bad_rows=ct, ctx=gpu, stream=s)
    # none of the refused calls wrote anything
    for t in (buf, cnt, mp, out):
        assert bool((t == FILL).all())
    # the same buffers in a valid call: every row present, so nothing is restored; the fill is no codeword, so
    # only the count's range (present parity rows) is known
    npa.recover_ragged_dev(p, d, size, pr, one, d_out=o, out_size=osize, restore=True, d_bad_rows=ct, ctx=gpu, stream=s)
    assert int(_host(cnt).view(np.uint32)[0]) <= p.wanted_n - p.k()
    assert bool((buf == FILL).all()) and bool((mp == FILL).all())
    assert bool((out == FILL).all())  # copy mode: the payload is the systematic rows

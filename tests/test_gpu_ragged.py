"""np_encode_ragged_dev / np_reconstruct_ragged_dev: one call for a batch whose
items differ in length and sit anywhere in the caller's buffers.  Every item
must equal the reference's ReedSolomon::encode (mod.rs:117-157) /
ReedSolomon::reconstruct (mod.rs:162-239) on that item alone, byte for byte
against the oracle, and no other byte of the buffers may change: they are
pre-filled with 0x5A and compared whole.

Items: 1, 2, 255, 256, 257, 300, 512 and 513 columns (a column is one symbol of
every shard: 2k payload bytes), payload lengths cols * 2k minus 0, 1 and
2k - 1.  They sit in the buffers in another order than in the batch, with gaps
of 2, 6 and 64 bytes; payload offsets are odd for some items; shard offsets are
2 mod 16 for some and 128-aligned, with rows of whole 128-byte lines (the
streaming-store path), for the items of 256 and 512 columns.  Batches of 11
and 1 add a pair of equal neighbours at a constant spacing (one run of the
fallback path).  Direct shapes (k in {64, 128, 256}) run the ragged kernels,
the others runs of the uniform launches."""
import functools

import numpy as np
import pytest

import novelpoly_amd as npa
from _stream_gate import Gate, run_gated

pytestmark = pytest.mark.gpu

FILL = 0x5A
COLS = [1, 2, 255, 256, 257, 300, 512, 513]
GAPS = [2, 6, 64]

# (n_wanted, k_wanted)
DIRECT = [(128, 64),     # n128 k64
          (512, 128),    # n512 k128
          (1024, 342),   # n1024 k256
          (600, 256),    # n1024 k256, wanted_n inside segment 2
          (512, 64)]     # n512 k64: n = 8k, the runtime shift loop
FALLBACK = [(60, 20), (1024, 512), (4096, 1366)]
SMALL_COLS = {(4096, 1366): [1, 2, 31, 32, 33, 64, 65, 70]}  # at most 70 columns
BATCHES = [8, 11, 1]


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _up(x, a):
    return (x + a - 1) // a * a


class Case:
    """One ragged batch under `p`: the items, the payloads in their buffer and
    the oracle's shard rows in theirs (everything else FILL)."""

    def __init__(self, oracle, nw, kw, batch, seed=0, cols=None):
        p = npa.CodeParams.derive_parameters(nw, kw)
        n, k, wn = p.n(), p.k(), p.wanted_n
        rng = np.random.default_rng(1000 * nw + kw + 7 * batch + seed)
        base = SMALL_COLS.get((nw, kw), COLS)
        if cols is None:
            if batch == 1:
                cols = [base[5]]
            elif batch == 8:
                cols = list(base)
            else:  # 11: items 8 and 9 are equal neighbours
                cols = list(base) + [base[5], base[5], base[1]]
        trims = [[0, 1, 2 * k - 1][i % 3] for i in range(len(cols))]
        if len(cols) == 11:
            trims[9] = trims[8]
        self.p, self.n, self.k, self.wn, self.cols = p, n, k, wn, cols
        self.plens = [c * 2 * k - t for c, t in zip(cols, trims)]
        # placement order in the buffers: not the batch order, but items 8 and 9 stay neighbours
        order = list(range(len(cols)))
        head = order[:8]
        order = head[::-1][1::2] + head[::-1][0::2] + order[8:]
        poff, soff = 1, 0
        place = {}
        for j, i in enumerate(order):
            sl = 2 * cols[i]
            gap = GAPS[j % 3]
            if sl % 128 == 0:
                soff = _up(soff, 128)  # rows of whole 128-byte lines
            elif j % 2 == 0:
                soff = _up(soff, 16) + 2
            if len(cols) == 11 and i == 9:  # the run: both strides constant and no smaller than the extents
                poff = place[8][0] + cols[8] * 2 * k + 64
                soff = place[8][1] + n * sl + 64
            place[i] = (poff, soff)
            poff += cols[i] * 2 * k + gap + (1 if j % 2 else 0)  # room for the reconstruct's padded output
            soff += n * sl + gap
        self.items = [(place[i][0], self.plens[i], place[i][1], 2 * cols[i]) for i in range(len(cols))]
        self.psize, self.ssize = poff + 64, soff + 64
        self.payloads = np.full(self.psize, FILL, np.uint8)
        self.shards = np.full(self.ssize, FILL, np.uint8)  # expected after the encode
        self.pay = []
        for (po, pl, so, sl) in self.items:
            data = rng.integers(0, 256, pl, dtype=np.uint8)
            self.pay.append(data.tobytes())
            self.payloads[po:po + pl] = data
            st, rows = oracle.encode(data.tobytes(), n, k, wn)
            assert st == 0 and len(rows) == wn and len(rows[0]) == sl
            self.shards[so:so + wn * sl] = np.frombuffer(b"".join(rows), np.uint8)
        assert any(it[0] & 1 for it in self.items) or len(cols) == 1
        self.rng = rng

    def item_rows(self, buf, i):
        _, _, so, sl = self.items[i]
        return buf[so:so + self.n * sl].reshape(self.n, sl)


@functools.lru_cache(maxsize=None)
def _case(oracle, nw, kw, batch):
    return Case(oracle, nw, kw, batch)


def _diff(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[:8].tolist()}")


def _encode(gpu, c):
    pay = _dev(c.payloads)
    out = _dev(np.full(c.ssize, FILL, np.uint8))
    npa.encode_ragged_dev(c.p, pay.data_ptr(), c.psize, out.data_ptr(), c.ssize, c.items, ctx=gpu, stream=_stream())
    return out


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("nw,kw", DIRECT + FALLBACK)
def test_encode(gpu, oracle, nw, kw, batch):
    c = _case(oracle, nw, kw, batch)
    got = _host(_encode(gpu, c))
    for i, (po, pl, so, sl) in enumerate(c.items):
        _diff(got[so:so + c.n * sl], c.shards[so:so + c.n * sl], f"item {i} ({c.cols[i]} columns)")
    _diff(got, c.shards, "bytes outside the items")


def _received(oracle, c):
    """Per item a presence pattern and received rows; returns (shard buffer,
    present batch x n, expected output buffer, expected status)."""
    n, k = c.n, c.k
    rng = np.random.default_rng(len(c.items) + n + k)
    buf = np.full(c.ssize, FILL, np.uint8)
    pres = np.zeros((len(c.items), n), np.uint8)
    want = np.full(c.psize, FILL, np.uint8)
    status = []
    for i, (po, pl, so, sl) in enumerate(c.items):
        kind = i % 5
        rows = rng.integers(0, 256, (n, sl), dtype=np.uint8)
        pr = np.zeros(n, np.uint8)
        if kind == 0:    # random bytes, random absences
            pr[rng.choice(n, int(rng.integers(k, n + 1)), replace=False)] = 1
        elif kind == 1:  # every systematic row present: copy mode
            pr[:k] = 1
            pr[k + rng.choice(n - k, (n - k) // 3, replace=False)] = 1
        elif kind == 2:  # exactly k present
            pr[rng.choice(n, k, replace=False)] = 1
        elif kind == 3:  # k - 1 present: NeedMoreShards, output untouched
            pr[rng.choice(n, k - 1, replace=False)] = 1
        else:            # decodable from the first 2k rows alone, one systematic row absent
            pick = rng.choice(np.arange(1, 2 * k), k + 2, replace=False)
            pr[pick] = 1
            if n > 2 * k:
                pr[2 * k + rng.choice(n - 2 * k, 3, replace=False)] = 1
        view = c.item_rows(buf, i)
        view[pr != 0] = rows[pr != 0]
        pres[i] = pr
        st, out = oracle.reconstruct([rows[v].tobytes() if pr[v] else None for v in range(n)], n, k)
        if kind == 3:
            assert st == npa.NeedMoreShards.code
            status.append((npa.NeedMoreShards.code, k - 1))
        else:
            assert st == 0 and len(out) == (sl // 2) * 2 * k
            want[po:po + len(out)] = np.frombuffer(out, np.uint8)
            status.append((0, int(pr.sum())))
    return buf, pres, want, status


@functools.lru_cache(maxsize=None)
def _recv_case(oracle, nw, kw, batch):
    return _received(oracle, _case(oracle, nw, kw, batch))


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("nw,kw", DIRECT + FALLBACK)
def test_reconstruct(gpu, oracle, nw, kw, batch):
    import torch

    c = _case(oracle, nw, kw, batch)
    buf, pres, want, status = _recv_case(oracle, nw, kw, batch)
    dbuf, dpres = _dev(buf), _dev(pres)
    for with_status in (True, False):
        out = _dev(np.full(c.psize, FILL, np.uint8))
        st_d = torch.full((len(c.items), 2), -1, dtype=torch.int32, device="cuda")
        npa.reconstruct_ragged_dev(c.p, dbuf.data_ptr(), c.ssize, dpres.data_ptr(), out.data_ptr(), c.psize, c.items,
                                   ctx=gpu, stream=_stream(), d_status=st_d.data_ptr() if with_status else 0)
        got = _host(out)
        for i, (po, pl, so, sl) in enumerate(c.items):
            ext = (sl // 2) * 2 * c.k
            _diff(got[po:po + ext], want[po:po + ext],
                  f"item {i} ({c.cols[i]} columns, pattern {i % 5}), status buffer {with_status}")
        _diff(got, want, "bytes outside the items")
        if with_status:
            stat = _host(st_d)
            assert [tuple(int(x) for x in r) for r in stat] == status
            errs = npa.payload_errors(c.p, stat)
            for i, (code, have) in enumerate(status):
                assert errs[i] == (npa.NeedMoreShards(have, c.k, c.n) if code else None), i
    _diff(_host(dbuf), buf, "the shard buffer is only read")


@pytest.mark.parametrize("batch", [11])
@pytest.mark.parametrize("nw,kw", DIRECT + FALLBACK)
def test_round_trip(gpu, oracle, nw, kw, batch):
    """Encode, drop rows, reconstruct with the same items array: the payloads
    come back, zero padded to whole columns."""
    import torch

    c = _case(oracle, nw, kw, batch)
    enc = _encode(gpu, c)
    rng = np.random.default_rng(nw + kw)
    pres = np.zeros((len(c.items), c.n), np.uint8)
    for i in range(len(c.items)):
        pres[i, rng.choice(c.wn, c.k + int(rng.integers(0, c.wn - c.k + 1)), replace=False)] = 1
    out = _dev(np.full(c.psize, FILL, np.uint8))
    st_d = torch.full((len(c.items), 2), -1, dtype=torch.int32, device="cuda")
    npa.reconstruct_ragged_dev(c.p, enc.data_ptr(), c.ssize, _dev(pres).data_ptr(), out.data_ptr(), c.psize, c.items,
                               ctx=gpu, stream=_stream(), d_status=st_d.data_ptr())
    got = _host(out)
    want = np.full(c.psize, FILL, np.uint8)
    for (po, pl, so, sl), data in zip(c.items, c.pay):
        ext = (sl // 2) * 2 * c.k
        want[po:po + ext] = 0
        want[po:po + pl] = np.frombuffer(data, np.uint8)
    _diff(got, want, "round trip")
    assert bool((st_d[:, 0] == 0).all())


@pytest.mark.parametrize("nw,kw", [(1024, 342), (128, 64), (512, 64), (60, 20), (1024, 512)])
def test_equal_lengths_match_the_uniform_calls(gpu, nw, kw):
    """All lengths equal at a constant spacing: the bytes of np_encode_batch_dev
    and np_reconstruct_batch_dev3."""
    import torch

    p = npa.CodeParams.derive_parameters(nw, kw)
    n, k, wn = p.n(), p.k(), p.wanted_n
    batch, cols = 9, 300
    plen, sl = cols * 2 * k - 3, 2 * cols
    pstride, bstride, ostride = cols * 2 * k + 6, n * sl + 2, cols * 2 * k + 6
    rng = np.random.default_rng(nw * kw)
    pay = _dev(rng.integers(0, 256, batch * pstride, dtype=np.uint8))
    items = [(b * pstride, plen, b * bstride, sl) for b in range(batch)]
    s = _stream()
    a = torch.full((batch * bstride,), FILL, dtype=torch.uint8, device="cuda")
    b_ = a.clone()
    npa.encode_batch_dev(p, pay.data_ptr(), plen, pstride, batch, a.data_ptr(), bstride, ctx=gpu, stream=s)
    npa.encode_ragged_dev(p, pay.data_ptr(), batch * pstride, b_.data_ptr(), batch * bstride, items, ctx=gpu, stream=s)
    torch.cuda.synchronize()
    assert torch.equal(a, b_)
    # the received rows: random bytes everywhere, so rows >= wanted_n are ordinary rows
    recv = _dev(rng.integers(0, 256, batch * bstride, dtype=np.uint8))
    pres = np.zeros((batch, n), np.uint8)
    for b in range(batch):
        pres[b, rng.choice(n, k - 1 + (b % 4) * (n - k) // 3, replace=False)] = 1
    pres[1, :k] = 1  # copy mode
    dpres = _dev(pres)
    oa = torch.full((batch * ostride,), FILL, dtype=torch.uint8, device="cuda")
    ob = oa.clone()
    sa = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
    sb = sa.clone()
    npa.reconstruct_batch_dev2(p, recv.data_ptr(), sl, bstride, dpres.data_ptr(), 0, batch, oa.data_ptr(), ostride,
                               ctx=gpu, stream=s, d_status=sa.data_ptr())
    npa.reconstruct_ragged_dev(p, recv.data_ptr(), batch * bstride, dpres.data_ptr(), ob.data_ptr(), batch * ostride,
                               items, ctx=gpu, stream=s, d_status=sb.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(oa, ob) and torch.equal(sa, sb)
    assert int((sa[:, 0] != 0).sum()) >= 2  # the batch holds undecodable payloads too


@pytest.mark.parametrize("nw,kw", [(1024, 342), (60, 20)])
def test_back_to_back_calls_keep_their_plans(gpu, oracle, nw, kw):
    """Two encodes and two reconstructs queued on one stream with different
    items and no synchronisation in between: each call's plan must outlive the
    next call's upload.  A gate in front (tests/_stream_gate.py) keeps the first
    call from starting before the last one is enqueued."""
    import torch

    c1 = _case(oracle, nw, kw, 11)
    c2 = _case(oracle, nw, kw, 8)
    r1 = _recv_case(oracle, nw, kw, 11)
    r2 = _recv_case(oracle, nw, kw, 8)
    s = _stream()

    def case(gate_ms):
        pay1, pay2 = _dev(c1.payloads), _dev(c2.payloads)
        e1, e2 = _dev(np.full(c1.ssize, FILL, np.uint8)), _dev(np.full(c2.ssize, FILL, np.uint8))
        b1, b2, p1, p2 = _dev(r1[0]), _dev(r2[0]), _dev(r1[1]), _dev(r2[1])
        o1, o2 = _dev(np.full(c1.psize, FILL, np.uint8)), _dev(np.full(c2.psize, FILL, np.uint8))
        g = Gate(torch.cuda.current_stream(), gate_ms)
        npa.encode_ragged_dev(c1.p, pay1.data_ptr(), c1.psize, e1.data_ptr(), c1.ssize, c1.items, ctx=gpu, stream=s)
        npa.encode_ragged_dev(c2.p, pay2.data_ptr(), c2.psize, e2.data_ptr(), c2.ssize, c2.items, ctx=gpu, stream=s)
        npa.reconstruct_ragged_dev(c1.p, b1.data_ptr(), c1.ssize, p1.data_ptr(), o1.data_ptr(), c1.psize, c1.items,
                                   ctx=gpu, stream=s)
        npa.reconstruct_ragged_dev(c2.p, b2.data_ptr(), c2.ssize, p2.data_ptr(), o2.data_ptr(), c2.psize, c2.items,
                                   ctx=gpu, stream=s)
        ms, held = g.host_ms(), g.open()
        _diff(_host(e1), c1.shards, "first encode")
        _diff(_host(e2), c2.shards, "second encode")
        _diff(_host(o1), r1[2], "first reconstruct")
        _diff(_host(o2), r2[2], "second reconstruct")
        return held, ms

    run_gated(case, label=f"ragged back to back {nw},{kw}")


def test_batch_zero_and_validation_on_the_device_calls(gpu):
    p = npa.CodeParams.derive_parameters(1024, 342)
    npa.encode_ragged_dev(p, 0, 0, 0, 0, [], ctx=gpu, stream=_stream())
    npa.reconstruct_ragged_dev(p, 0, 0, 0, 0, 0, [], ctx=gpu, stream=_stream())
    buf = _dev(np.full(4096, FILL, np.uint8))
    k = p.k()
    with pytest.raises(npa.InvalidArgument):  # the shard extent ends one byte past the buffer
        npa.encode_ragged_dev(p, buf.data_ptr(), 4096, buf.data_ptr(), 2 * p.wanted_n - 1, [(0, 2 * k, 0, 2)], ctx=gpu,
                              stream=_stream())
    with pytest.raises(npa.PayloadSizeIsZero):
        npa.encode_ragged_dev(p, buf.data_ptr(), 4096, buf.data_ptr(), 4096, [(0, 0, 0, 2)], ctx=gpu, stream=_stream())
    with pytest.raises(npa.EmptyShard):
        npa.reconstruct_ragged_dev(p, buf.data_ptr(), 4096, buf.data_ptr(), buf.data_ptr(), 4096, [(0, 0, 0, 3)],
                                   ctx=gpu, stream=_stream())
    assert bool((buf == FILL).all())

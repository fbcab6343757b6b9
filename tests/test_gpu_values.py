"""The input-value contract of every kernel family, in one place
(tests/_value_cases.py holds the values; tests/test_values_cpu.py pins the
oracle on them first).  The other GPU modules draw uniformly random symbols and
write presence flags as 0 or 1 only; here:

(a) degenerate symbols -- all zero, all 0xFF, one nonzero symbol per column, a
    zero tile next to a random partial one, zero rows, zero columns -- through
    the encode, the reconstruct (with and without caller locators, three
    masks), the recover calls and the low-level hooks, byte for byte against
    the oracle with fills around every buffer.  A zero symbol takes the
    `a == 0` return of gf_mul_log (device_common.hpp) on the generic decode
    shape (1024, 64); zero inputs and zero columns must give zero outputs,
    asserted on the device over whole buffers.
(b) presence bytes -- the header promises "nonzero = present".  Each shape's
    batch of five masks (more than k present, exactly k, k - 1, one systematic
    row absent, all present) is written as 0/1, 0xFF, 0x80, 2 and
    ((37 v + b) % 255) + 1; every output of every entry point under a nonzero
    spelling is byte-identical to the 0/1 call's, whole buffers with their
    fills, and the 0/1 call's equals the oracle's.  On the resident shapes the
    device-mask calls run again with d_present one byte past an aligned base
    (the byte path of res_common.hpp lane_rows_present).
(c) every bit position of the verify -- one payload per byte of a row, one bit
    of that byte flipped in one parity row, so a lane's piece, a half of a
    word or the tail of the partial tile that a compare skipped shows at its
    own payload.

Open point, recorded and not probed here: the flag reads of the sub-transform
and big decodes (kernels_huge.hip k_huge_records, the RowView word reads of
kernels_big.hip) fetch the flags as dwords with no byte path, and
include/novelpoly.h states no alignment for d_present.  These tests pass an
aligned d_present on those shapes.

Each case first asserts npa.kernel_family for its shape and direction, so a
change of dispatch fails there and not silently on other kernels."""
import ctypes as C
import functools

import numpy as np
import pytest

import _value_cases as vc
import novelpoly_amd as npa
from test_gpu_recover import run_recover

pytestmark = pytest.mark.gpu

FILL = 0x5A
GUARD = 0xA5
UNDECODABLE = 0xFFFFFFFF
SL, SL_RES, SL_SUB = 2 * 300, 2 * 260, 2 * 70
OUT_SLACK = 32

GENERIC, SMALL, FAST, RES, BIG, HUGE = (npa.FAMILY_GENERIC, npa.FAMILY_SMALL, npa.FAMILY_FAST, npa.FAMILY_RES,
                                        npa.FAMILY_BIG, npa.FAMILY_HUGE)
# (n_wanted, k_wanted, shard_len, encode family, reconstruct family)
SHAPES = [(16, 8, SL, SMALL, SMALL), (100, 34, SL, SMALL, SMALL),
          (256, 86, SL, FAST, FAST), (512, 128, SL, FAST, FAST), (512, 256, SL, FAST, FAST),
          (1024, 342, SL, FAST, FAST), (2048, 256, SL, FAST, FAST), (600, 256, SL, FAST, FAST),
          (1024, 512, SL_RES, RES, RES), (4096, 1366, SL_RES, RES, RES),
          (7000, 2334, SL_RES, BIG, BIG),
          (16384, 5462, SL_SUB, HUGE, HUGE),
          (1024, 64, SL, FAST, GENERIC)]
RESIDENT = [s for s in SHAPES if s[4] == RES]
RAGGED = [s for s in SHAPES if s[:2] in ((256, 86), (1024, 342))]
LARGE_N = 8192  # from here on a decode batch carries each class once, the masks in turn
shapes = pytest.mark.parametrize("nw,kw,sl,enc_family,rec_family", SHAPES)


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the cached cases are read only


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _full(shape, value, dtype=None):
    import torch

    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype or torch.uint8, device="cuda")


def _params(nw, kw, sl, enc_family, rec_family):
    p = npa.CodeParams.derive_parameters(nw, kw)
    assert (npa.kernel_family(p, sl, False), npa.kernel_family(p, sl, True)) == (enc_family, rec_family), \
        f"({nw}, {kw}) at rows of {sl} bytes left its kernel family"
    return p


def _recv(rows, pr):
    return [rows[v].tobytes() if pr[v] else None for v in range(len(pr))]


def _as_u16(t):
    return _host(t).view(np.uint16)


# ------------------------------------------------------------- the oracle ----
def _expected_one(oracle, n, k, wn, rows, pr):
    """(payload or None, {absent row below wanted_n: bytes} or None, n flags)
    of one payload: the oracle's reconstruct and encode(reconstruct)."""
    recv = _recv(rows, pr)
    st, pay = oracle.reconstruct(recv, n, k)
    flags = np.zeros(n, np.uint8)
    if st:
        assert st == npa.NeedMoreShards.code and int((pr != 0).sum()) < k
        return None, None, flags
    st, enc = oracle.encode(pay, n, k, wn)
    assert st == 0 and len(enc) == wn and len(enc[0]) == rows.shape[1]
    absent = {}
    for v in range(wn):
        if not pr[v]:
            absent[v] = enc[v]
        elif enc[v] != recv[v]:
            flags[v] = 1
    assert not flags[:k].any()  # systematic rows never mismatch
    return pay, absent, flags


def _expected(oracle, p, pats):
    """The oracle's answers for [(name, rows, present)] in the form of
    test_gpu_recover.expected_recover: (rows, (flags, counts, status), payloads)."""
    n, k, wn = p.n(), p.k(), p.wanted_n
    rows_l, pays, counts, status = [], [], [], []
    flags = np.zeros((len(pats), n), np.uint8)
    for b, (name, rows, pr) in enumerate(pats):
        pay, absent, fl = _expected_one(oracle, n, k, wn, rows, pr)
        pays.append(pay)
        rows_l.append(absent)
        flags[b] = fl
        counts.append(UNDECODABLE if pay is None else int(fl.sum()))
        status.append((npa.NeedMoreShards.code if pay is None else 0, int((pr != 0).sum())))
    flags.setflags(write=False)
    return rows_l, (flags, np.asarray(counts, np.uint32), status), pays


def _decode_masks(rng, n, k, wn):
    """The three masks of (a): k random rows, every systematic row absent (all
    rows of [k, wanted_n) present), every systematic row present with half of
    the parity rows."""
    assert wn - k >= k, "every shape of this module keeps k parity rows"
    a = np.zeros(n, np.uint8)
    a[rng.choice(wn, k, replace=False)] = 1
    b = np.zeros(n, np.uint8)
    b[k:wn] = 1
    c = np.zeros(n, np.uint8)
    c[:k] = 1
    c[k + rng.choice(wn - k, (wn - k + 1) // 2, replace=False)] = 1
    return [("k-random", a), ("systematic-absent", b), ("systematic-present", c)]


# -------------------------------------------------- (a) degenerate symbols ----
@functools.lru_cache(maxsize=None)
def _encode_case(oracle, n, k, wn, sl):
    rng = np.random.default_rng(7 * n + k + wn + sl)
    pays = np.stack([vc.payload(name, rng, k, sl // 2) for name in vc.CLASSES])
    want = np.empty((len(vc.CLASSES), wn, sl), np.uint8)
    for b in range(len(vc.CLASSES)):
        st, enc = oracle.encode(pays[b].tobytes(), n, k, wn)
        assert st == 0 and len(enc[0]) == sl
        want[b] = np.frombuffer(b"".join(enc), np.uint8).reshape(wn, sl)
    for a in (pays, want):
        a.setflags(write=False)
    return pays, want


@shapes
def test_encode_values(gpu, oracle, nw, kw, sl, enc_family, rec_family):
    """np_encode_batch_dev, one batch holding every class."""
    import torch

    p = _params(nw, kw, sl, enc_family, rec_family)
    n, k, wn, cols = p.n(), p.k(), p.wanted_n, sl // 2
    pays, want = _encode_case(oracle, n, k, wn, sl)
    batch, plen, stride = len(vc.CLASSES), cols * 2 * k, n * sl + 64
    dpay = _dev(pays)
    buf = _full(64 + batch * stride + 64, FILL)
    npa.encode_batch_dev(p, dpay.data_ptr(), plen, plen, batch, buf.data_ptr() + 64, stride, ctx=gpu, stream=_stream())
    exp = np.full(64 + batch * stride + 64, FILL, np.uint8)
    for b in range(batch):
        exp[64 + b * stride: 64 + b * stride + wn * sl] = want[b].reshape(-1)
    got = _host(buf)
    for b, name in enumerate(vc.CLASSES):
        lo, hi = 64 + b * stride, 64 + (b + 1) * stride
        bad = np.flatnonzero(got[lo:hi] != exp[lo:hi])
        assert bad.size == 0, (name, bad.size, "rows", sorted(set((bad // sl).tolist()))[:8])
    assert np.array_equal(got, exp)
    assert torch.equal(dpay, _dev(pays))
    # no oracle: a zero payload and a zero column encode to zeros, over the whole rows
    shards = buf[64:64 + batch * stride].view(batch, stride)[:, :wn * sl].reshape(batch, wn, cols, 2)
    assert not bool(shards[vc.CLASSES.index("zero")].any())
    zc = torch.from_numpy(vc.zero_column_index(cols)).cuda()
    assert not bool(shards[vc.CLASSES.index("zero-columns")][:, zc].any())
    assert not bool(shards[vc.CLASSES.index("zero-tile")][:, :vc.zero_tile_columns(cols)].any())


@functools.lru_cache(maxsize=None)
def _decode_case(oracle, n, k, wn, sl, every):
    """[(class/mask, rows, present)] and the oracle's answers: every class under
    every mask, or (every = False) each class once with the masks in turn."""
    rng = np.random.default_rng(11 * n + k + wn + sl)
    masks = _decode_masks(rng, n, k, wn)
    pats = []
    for i, name in enumerate(vc.CLASSES):
        for j, (mname, pr) in enumerate(masks):
            if every or j == i % len(masks):
                pats.append((f"{name}/{mname}", vc.received_rows(name, rng, n, sl // 2, pr), pr))
    return pats, _expected(oracle, npa.CodeParams(n, k, wn), pats)


def _stage(pats, n, sl, stride, offset=0):
    """The shard buffer of a batch: present rows, FILL in absent rows and gaps."""
    before = np.full(offset + len(pats) * stride + 64, FILL, np.uint8)
    for b, (_, rows, pr) in enumerate(pats):
        view = before[offset + b * stride: offset + b * stride + n * sl].reshape(n, sl)
        view[pr != 0] = rows[pr != 0]
    return before


def _want_out(pays, pay_len, ostride):
    want = np.full(64 + len(pays) * ostride + 64, GUARD, np.uint8)
    for b, pay in enumerate(pays):
        if pay is not None:
            assert len(pay) == pay_len
            want[64 + b * ostride: 64 + b * ostride + pay_len] = np.frombuffer(pay, np.uint8)
    return want


def _assert_out(got, want, names, ostride, tag):
    for b, name in enumerate(names):
        lo, hi = 64 + b * ostride, 64 + (b + 1) * ostride
        bad = np.flatnonzero(got[lo:hi] != want[lo:hi])
        assert bad.size == 0, (tag, b, name, bad.size, "first byte", int(bad[0]))
    assert np.array_equal(got, want), (tag, "guards")


@shapes
def test_reconstruct_values(gpu, oracle, nw, kw, sl, enc_family, rec_family):
    """np_reconstruct_batch_dev3 with d_locators = NULL and with the locators of
    np_error_locator_dev, on received rows of every class (no codewords)."""
    import torch

    p = _params(nw, kw, sl, enc_family, rec_family)
    n, k, wn, cols = p.n(), p.k(), p.wanted_n, sl // 2
    pats, (_, (_, _, status), pays) = _decode_case(oracle, n, k, wn, sl, n < LARGE_N)
    names = [name for name, _, _ in pats]
    batch, stride, pay_len = len(pats), n * sl + 64, cols * 2 * k
    ostride = pay_len + OUT_SLACK
    before = _stage(pats, n, sl, stride)
    want = _want_out(pays, pay_len, ostride)
    dbuf, dpres = _dev(before), _dev(np.stack([pr for _, _, pr in pats]))
    loc = _full((batch, n), 0, torch.int16)
    npa.error_locator_dev(n, dpres.data_ptr(), batch, loc.data_ptr(), ctx=gpu, stream=_stream())
    zc = torch.from_numpy(vc.zero_column_index(cols)).cuda()
    for with_loc in (False, True):
        out = _full(64 + batch * ostride + 64, GUARD)
        st = _full((batch, 2), -1, torch.int32)
        npa.reconstruct_batch_dev2(p, dbuf.data_ptr(), sl, stride, dpres.data_ptr(), loc.data_ptr() if with_loc else 0,
                                   batch, out.data_ptr() + 64, ostride, ctx=gpu, stream=_stream(),
                                   d_status=st.data_ptr())
        _assert_out(_host(out), want, names, ostride, f"locators {with_loc}")
        assert [tuple(int(x) for x in r) for r in _host(st)] == status, with_loc
        o = out[64:64 + batch * ostride].view(batch, ostride)[:, :pay_len].reshape(batch, cols, 2 * k)
        for b, name in enumerate(names):
            if name.startswith("zero/"):
                assert not bool(o[b].any()), (name, with_loc)
            elif name.startswith("zero-columns/"):
                assert not bool(o[b][zc].any()), (name, with_loc)
            elif name.startswith("zero-tile/"):
                assert not bool(o[b][:vc.zero_tile_columns(cols)].any()), (name, with_loc)
    assert np.array_equal(_host(dbuf), before)


@functools.lru_cache(maxsize=None)
def _recover_case(oracle, n, k, wn, sl):
    pats, _ = _decode_case(oracle, n, k, wn, sl, False)
    # one more received row per k-random payload, so that its verdict compares a row
    rng = np.random.default_rng(n + k)
    pats = list(pats)
    for i, (name, rows, pr) in enumerate(pats):
        if name.endswith("/k-random"):
            pr = pr.copy()
            extra = int(rng.choice(np.flatnonzero(pr[k:wn] == 0))) + k
            pr[extra] = 1
            rows = rows.copy()
            rows[extra] = 0 if name.startswith("zero/") else rows[np.flatnonzero(pr)[0]]
            pats[i] = (name + "+1", rows, pr)
    return pats, _expected(oracle, npa.CodeParams(n, k, wn), pats)


@shapes
def test_recover_values(gpu, oracle, nw, kw, sl, enc_family, rec_family):
    """np_recover_batch_dev asking for the payload, the restore and the verdict
    together: the restore's store path and the verify's compare on zero, 0xFF
    and sparse rows."""
    p = _params(nw, kw, sl, enc_family, rec_family)
    pats, exp = _recover_case(oracle, p.n(), p.k(), p.wanted_n, sl)
    counts = dict(zip((name for name, _, _ in pats), exp[1][1].tolist()))
    assert all(c == 0 for name, c in counts.items() if name.startswith("zero/"))  # zero rows are a codeword
    assert any(c > 0 for c in counts.values())
    run_recover(gpu, p, sl, pats, exp, label=f"{nw},{kw}",
                variants=[((True, True, True), True, True), ((False, True, True), False, True)])


# ---- ragged and host -------------------------------------------------------
class Ragged:
    """Items of different lengths in one shard buffer: item i's rows at
    offs[i], its payload at poffs[i]; absent rows, gaps and guards hold FILL."""

    def __init__(self, p, per_item):
        self.p, self.per_item = p, per_item
        n, k = p.n(), p.k()
        self.items, so, po = [], 16, 3
        for rows, pr in per_item:
            sl = rows.shape[1]
            self.items.append((po, 0, so, sl))
            so += n * sl + 16 + 2 * (len(self.items) % 2)  # even shard offsets, 2 mod 4 among them
            po += (sl // 2) * 2 * k + 5
        self.ssize, self.psize = so + 64, po + 64
        self.before = np.full(self.ssize, FILL, np.uint8)
        for (_, _, so, sl), (rows, pr) in zip(self.items, per_item):
            view = self.before[so:so + n * sl].reshape(n, sl)
            view[pr != 0] = rows[pr != 0]

    def expected(self, oracle):
        p = self.p
        n, k, wn = p.n(), p.k(), p.wanted_n
        self.restored = self.before.copy()
        self.out = np.full(self.psize, GUARD, np.uint8)
        self.flags = np.zeros((len(self.items), n), np.uint8)
        counts, self.status = [], []
        for i, ((po, _, so, sl), (rows, pr)) in enumerate(zip(self.items, self.per_item)):
            pay, absent, fl = _expected_one(oracle, n, k, wn, rows, pr)
            self.status.append((npa.NeedMoreShards.code if pay is None else 0, int((pr != 0).sum())))
            counts.append(UNDECODABLE if pay is None else int(fl.sum()))
            if pay is None:
                continue
            self.out[po:po + len(pay)] = np.frombuffer(pay, np.uint8)
            self.flags[i] = fl
            view = self.restored[so:so + n * sl].reshape(n, sl)
            for v, data in absent.items():
                view[v] = np.frombuffer(data, np.uint8)
        self.counts = np.asarray(counts, np.uint32)
        return self

    def run(self, gpu, dpres, calls=("reconstruct", "restore", "verify", "recover")):
        """{call: its buffers}, each whole with its fills, for the flags at dpres."""
        import torch

        p, batch, n = self.p, len(self.items), self.p.n()
        dbefore = _dev(self.before)
        res = {}

        def bufs():
            return (dbefore.clone(), _full(self.psize, GUARD), _full(4 * batch + 128, GUARD),
                    _full(batch * n + 128, GUARD), _full((batch, 2), -1, torch.int32))

        if "reconstruct" in calls:
            buf, out, cnt, mp, st = bufs()
            npa.reconstruct_ragged_dev(p, buf.data_ptr(), self.ssize, dpres, out.data_ptr(), self.psize, self.items,
                                       ctx=gpu, stream=_stream(), d_status=st.data_ptr())
            res["reconstruct"] = (buf, out, cnt, mp, st)
        if "restore" in calls:
            buf, out, cnt, mp, st = bufs()
            npa.restore_shards_ragged_dev(p, buf.data_ptr(), self.ssize, dpres, self.items, ctx=gpu, stream=_stream(),
                                          d_status=st.data_ptr())
            res["restore"] = (buf, out, cnt, mp, st)
        if "verify" in calls:
            buf, out, cnt, mp, st = bufs()
            npa.verify_shards_ragged_dev(p, buf.data_ptr(), self.ssize, dpres, self.items, cnt.data_ptr() + 64, ctx=gpu,
                                         stream=_stream(), d_mismatch=mp.data_ptr() + 64, d_status=st.data_ptr())
            res["verify"] = (buf, out, cnt, mp, st)
        if "recover" in calls:
            buf, out, cnt, mp, st = bufs()
            npa.recover_ragged_dev(p, buf.data_ptr(), self.ssize, dpres, self.items, d_out=out.data_ptr(),
                                   out_size=self.psize, restore=True, d_bad_rows=cnt.data_ptr() + 64,
                                   d_mismatch=mp.data_ptr() + 64, d_status=st.data_ptr(), ctx=gpu, stream=_stream())
            res["recover"] = (buf, out, cnt, mp, st)
        torch.cuda.synchronize()
        return res

    def check(self, res):
        """The 0/1 outputs of run() against the oracle, every buffer whole."""
        batch, n = len(self.items), self.p.n()
        cnt_none = np.full(4 * batch + 128, GUARD, np.uint8)
        cnt_want = cnt_none.copy()
        cnt_want[64:-64] = self.counts.view(np.uint8)
        map_none = np.full(batch * n + 128, GUARD, np.uint8)
        map_want = map_none.copy()
        map_want[64:-64] = self.flags.reshape(-1)
        none_out = np.full(self.psize, GUARD, np.uint8)
        want = {"reconstruct": (self.before, self.out, cnt_none, map_none),
                "restore": (self.restored, none_out, cnt_none, map_none),
                "verify": (self.before, none_out, cnt_want, map_want),
                "recover": (self.restored, self.out, cnt_want, map_want)}
        for call, (buf, out, cnt, mp, st) in res.items():
            for what, got, exp in zip(("shards", "payloads", "counts", "map"), (buf, out, cnt, mp), want[call]):
                got = _host(got)
                bad = np.flatnonzero(got != exp)
                assert bad.size == 0, (call, what, bad.size, "first byte", int(bad[0]))
            assert [tuple(int(x) for x in r) for r in _host(st)] == self.status, call


def _same(res, ref, tag):
    """Every buffer of every call byte-identical to the 0/1 call's."""
    import torch

    assert res.keys() == ref.keys()
    for call in ref:
        assert len(res[call]) == len(ref[call])
        for i, (a, b) in enumerate(zip(res[call], ref[call])):
            if isinstance(b, torch.Tensor):
                assert torch.equal(a, b), (tag, call, i, (a != b).reshape(-1).nonzero()[:8].reshape(-1).tolist())
            elif isinstance(b, np.ndarray):
                assert np.array_equal(a, b), (tag, call, i, np.flatnonzero(a != b)[:8].tolist())
            else:
                assert a == b, (tag, call, i)


RAGGED_LENGTHS = (2 * 300, 2 * 256, 2 * 1)


@functools.lru_cache(maxsize=None)
def _ragged_values_case(oracle, n, k, wn):
    rng = np.random.default_rng(13 * n + k + wn)
    masks = _decode_masks(rng, n, k, wn)
    per_item = []
    for i, name in enumerate(vc.CLASSES):
        pr = masks[(i + 1) % len(masks)][1]
        if (i + 1) % len(masks) == 0:  # k random rows and one more: the verdict compares a row
            pr = pr.copy()
            pr[int(np.flatnonzero(pr[k:wn] == 0)[0]) + k] = 1
        per_item.append((vc.received_rows(name, rng, n, RAGGED_LENGTHS[i % 3] // 2, pr), pr))
    return Ragged(npa.CodeParams(n, k, wn), per_item).expected(oracle)


@pytest.mark.parametrize("nw,kw,sl,enc_family,rec_family", RAGGED)
def test_recover_ragged_values(gpu, oracle, nw, kw, sl, enc_family, rec_family):
    """np_recover_ragged_dev: one call whose items carry different classes and
    rows of 600, 512 and 2 bytes."""
    p = _params(nw, kw, sl, enc_family, rec_family)
    r = _ragged_values_case(oracle, p.n(), p.k(), p.wanted_n)
    dpres = _dev(np.stack([pr for _, pr in r.per_item]))
    r.check(r.run(gpu, dpres.data_ptr(), calls=("recover",)))


class HostBatch:
    """A uniform batch in pageable host memory with guards around every buffer."""

    def __init__(self, p, sl, pats, pres):
        n, k = p.n(), p.k()
        self.p, self.sl, self.batch, self.n = p, sl, len(pats), n
        self.stride, self.pay_len = n * sl + 64, (sl // 2) * 2 * k
        self.ostride = self.pay_len + OUT_SLACK
        self.before = _stage(pats, n, sl, self.stride, offset=64)
        self.pres = np.ascontiguousarray(pres)
        self.fresh()

    def fresh(self):
        self.sh = self.before.copy()
        self.out = np.full(64 + self.batch * self.ostride + 64, GUARD, np.uint8)
        self.cnt = np.full(4 * self.batch + 128, GUARD, np.uint8)
        self.mp = np.full(self.batch * self.n + 128, GUARD, np.uint8)
        self.st = np.full((self.batch, 2), -1, np.int32)

    def recover(self, gpu, with_status=True, b0=0, count=None):
        count = self.batch - b0 if count is None else count
        npa.recover_batch_host(self.p, self.sh.ctypes.data + 64 + b0 * self.stride, self.sl, self.stride,
                               self.pres.ctypes.data + b0 * self.n, count, ctx=gpu,
                               out=self.out.ctypes.data + 64 + b0 * self.ostride, out_stride=self.ostride, restore=True,
                               bad_rows=self.cnt.ctypes.data + 64 + 4 * b0, mismatch=self.mp.ctypes.data + 64 + b0 * self.n,
                               status=self.st.ctypes.data + 8 * b0 if with_status else 0)

    def reconstruct(self, gpu, b0=0, count=None):
        count = self.batch - b0 if count is None else count
        npa.reconstruct_batch_host(self.p, self.sh.ctypes.data + 64 + b0 * self.stride, self.sl, self.stride,
                                   self.pres.ctypes.data + b0 * self.n, count,
                                   self.out.ctypes.data + 64 + b0 * self.ostride, self.ostride, ctx=gpu)

    def buffers(self):
        return tuple(a.copy() for a in (self.sh, self.out, self.cnt, self.mp, self.st))

    def check(self, exp, restore, verify, with_status=True, tag=""):
        """The buffers against the oracle's answers `exp` (_expected)."""
        exp_rows, (flags, counts, status), pays = exp
        want = self.before.copy()
        if restore:
            for b in range(self.batch):
                view = want[64 + b * self.stride: 64 + b * self.stride + self.n * self.sl].reshape(self.n, self.sl)
                for v, data in (exp_rows[b] or {}).items():
                    view[v] = np.frombuffer(data, np.uint8)
        assert np.array_equal(self.sh, want), (tag, "shards")
        _assert_out(self.out, _want_out(pays, self.pay_len, self.ostride), [""] * self.batch, self.ostride, tag)
        if verify:
            assert self.cnt[64:-64].copy().view(np.uint32).tolist() == counts.tolist(), tag
            assert np.array_equal(self.mp[64:-64].reshape(self.batch, self.n), flags), tag
            assert (self.cnt[:64] == GUARD).all() and (self.cnt[-64:] == GUARD).all(), tag
            assert (self.mp[:64] == GUARD).all() and (self.mp[-64:] == GUARD).all(), tag
        else:
            assert (self.cnt == GUARD).all() and (self.mp == GUARD).all(), tag
        if with_status:
            assert [tuple(int(x) for x in r) for r in self.st] == status, tag
        else:
            assert (self.st == -1).all(), tag


def test_recover_host_values(gpu, oracle):
    """np_recover_batch_host on (1024, 342), pageable buffers, every class."""
    p = _params(1024, 342, SL, FAST, FAST)
    pats, exp = _recover_case(oracle, p.n(), p.k(), p.wanted_n, SL)
    h = HostBatch(p, SL, pats, np.stack([pr for _, _, pr in pats]))
    h.recover(gpu)
    h.check(exp, True, True, tag="recover_batch_host")


# ---- the low-level hooks -----------------------------------------------------
def test_mul_dev_values(gpu, oracle):
    """np_mul_dev on zero, 0xFFFF, 1 and one-hot operands against every
    multiplier class (log form: 0, 1, 65534, 65535 and random)."""
    import torch

    rng = np.random.default_rng(3)
    a = np.concatenate([vc.vector(name, rng, 64) for name in vc.VECTORS] + [np.arange(64, dtype=np.uint16)])
    m = np.tile(np.concatenate([[0, 1, 65534, 65535], rng.integers(0, 65536, 60)]).astype(np.uint16), len(a) // 64)
    da, dm = _dev(a.view(np.int16)), _dev(m.view(np.int16))
    out = _full(a.size, 0x7777, torch.int16)
    npa.mul_dev(da.data_ptr(), dm.data_ptr(), out.data_ptr(), a.size, ctx=gpu, stream=_stream())
    want = np.array([oracle.mul(int(x), int(y)) for x, y in zip(a, m)], np.uint16)
    assert np.array_equal(_as_u16(out), want)
    assert not _as_u16(out)[a == 0].any()  # the a == 0 return


def _columns(rng, size, cols):
    """cols x size: one column of each vector class among random ones."""
    x = rng.integers(0, 65536, (cols, size), dtype=np.uint16)
    names = ["random"] * cols
    few = cols <= len(vc.VECTORS)  # then a zero and a one-hot column, the last one random
    for j, name in enumerate(("zero", "last")[:cols - 1] if few else vc.VECTORS):
        c = j if few else (5 * j + 1) % cols
        assert names[c] == "random"
        x[c] = vc.vector(name, rng, size)
        names[c] = name
    return x, names


@pytest.mark.parametrize("size,column_counts", [(2, (1, 37)), (64, (1, 37)), (1024, (1, 37)), (4096, (1, 37)),
                                                (65536, (3,))])
def test_afft_dev_values(gpu, oracle, size, column_counts):
    rng = np.random.default_rng(size)
    for cols in column_counts:
        firsts = vc.VECTORS if cols == 1 else ("mixed",)
        for first in firsts:
            x, names = _columns(rng, size, cols)
            if cols == 1:
                x[0], names[0] = vc.vector(first, rng, size), first
            for index in sorted({0, size % 65536, 65536 - size}):
                for inverse in (False, True):
                    t = _dev(x.view(np.int16))
                    npa.afft_dev(t.data_ptr(), size, index, cols, inverse=inverse, ctx=gpu, stream=_stream())
                    got = _as_u16(t)
                    f = oracle.inverse_afft if inverse else oracle.afft
                    for c in range(cols):
                        assert np.array_equal(got[c], f(x[c], size, index)), (names[c], c, cols, index, inverse)
                        if names[c] == "zero":
                            assert not got[c].any()


@pytest.mark.parametrize("size", [4, 1024, 65536])
def test_walsh_dev_values(gpu, oracle, size):
    rng = np.random.default_rng(size)
    for name in vc.VECTORS:
        x = vc.vector(name, rng, size)
        t = _dev(x.view(np.int16))
        npa.walsh_dev(t.data_ptr(), size, ctx=gpu, stream=_stream())
        assert np.array_equal(_as_u16(t), oracle.walsh(x)), name


@pytest.mark.parametrize("n,k", [(16, 8), (256, 64), (4096, 256)])
def test_codec_hooks_values(gpu, oracle, n, k):
    """np_encode_low_dev and np_decode_main_dev with 1 and 9 columns, the
    vectors and erasure patterns of tests/test_values_cpu.py."""
    import torch

    rng = np.random.default_rng(n + k)
    for cols in (1, 9):
        for first in (vc.VECTORS if cols == 1 else ("mixed",)):
            d, names = _columns(rng, k, cols)
            if cols == 1:
                d[0], names[0] = vc.vector(first, rng, k), first
            dd = _dev(d.view(np.int16))
            cw = _full((cols, n), 0x5A5A, torch.int16)
            npa.encode_low_dev(dd.data_ptr(), k, cw.data_ptr(), n, cols, ctx=gpu, stream=_stream())
            code = _as_u16(cw).copy()
            for c in range(cols):
                assert np.array_equal(code[c], oracle.encode_low(d[c], k, n)), (names[c], cols)
                if names[c] == "zero":
                    assert not code[c].any()
            for pattern in vc.ERASURES:
                er = vc.erasure(pattern, rng, n, k)
                if er is None:
                    continue
                full = oracle.eval_error_polynomial(er)
                pres, loc = _dev(1 - er), _dev(full[:n].copy().view(np.int16))
                # the received words: the codewords, and degenerate words that are none
                noise, _ = _columns(rng, n, cols)
                for words in (code, noise):
                    recv = words.copy()
                    recv[:, er == 1] = 0
                    t = _dev(recv.view(np.int16))
                    npa.decode_main_dev(t.data_ptr(), k, pres.data_ptr(), loc.data_ptr(), n, cols, ctx=gpu,
                                        stream=_stream())
                    got = _as_u16(t)
                    for c in range(cols):
                        want = oracle.decode_main(recv[c], k, er, full)
                        assert np.array_equal(got[c], want), (names[c], pattern, cols, c)


# ------------------------------------------------------ (b) presence bytes ----
class PresenceCase:
    pass


@functools.lru_cache(maxsize=None)
def _presence_case(oracle, n, k, wn, sl):
    """Five masks over random received bytes and over codewords, and the
    oracle's answers for the 0/1 spelling (read only)."""
    c = PresenceCase()
    rng = np.random.default_rng(17 * n + k + wn + sl)
    cols = sl // 2
    c.p = npa.CodeParams(n, k, wn)
    masks = vc.masks(rng, n, k, wn)
    c.names = [name for name, _ in masks]
    c.pres = np.stack([pr for _, pr in masks])
    assert (c.pres.sum(axis=1) >= k).tolist() == [True, True, False, True, True] and not c.pres[:, wn:].any()
    c.pats = [(name, rng.integers(0, 256, (n, sl), dtype=np.uint8), pr) for name, pr in masks]
    c.exp = _expected(oracle, c.p, c.pats)
    assert c.exp[1][1][0] > 0 and c.exp[1][1][2] == UNDECODABLE  # random rows mismatch; k - 1 does not decode
    # codewords of full-length payloads: the opt-in prefix decode returns the payload
    c.code_pay = rng.integers(0, 256, (len(masks), cols * 2 * k), dtype=np.uint8)
    c.code = []
    for b, (name, pr) in enumerate(masks):
        st, enc = oracle.encode(c.code_pay[b].tobytes(), n, k, wn)
        assert st == 0
        rows = np.full((n, sl), FILL, np.uint8)
        rows[:wn] = np.frombuffer(b"".join(enc), np.uint8).reshape(wn, sl)
        c.code.append((name, rows, pr))
    c.locators = np.stack([oracle.eval_error_polynomial(1 - pr)[:n] for pr in c.pres])
    # decode_main on 9 columns of payload 0's rows under mask 0
    er = (1 - c.pres[0]).astype(np.uint8)
    words = np.ascontiguousarray(c.pats[0][1][:, :18].reshape(n, 9, 2)).astype(np.uint16)
    c.words = np.ascontiguousarray((words[:, :, 0] << 8 | words[:, :, 1]).T)
    c.words[:, er == 1] = 0
    full = oracle.eval_error_polynomial(er)
    c.decoded = np.stack([oracle.decode_main(c.words[j], k, er, full) for j in range(9)])
    return c


def _device_outputs(gpu, c, sl, dp, pres):
    """Every device entry point of (b) on the flags at device address `dp`
    (host copy `pres`): {call: its buffers, whole}."""
    import torch

    p = c.p
    n, k = p.n(), p.k()
    batch, stride, pay_len = len(c.pats), n * sl + 64, (sl // 2) * 2 * k
    ostride = pay_len + OUT_SLACK
    s = _stream()
    dbefore, dcode = _dev(_stage(c.pats, n, sl, stride)), _dev(_stage(c.code, n, sl, stride))
    res = {}

    def outbuf():
        return _full(64 + batch * ostride + 64, GUARD)

    def status():
        return _full((batch, 2), -1, torch.int32)

    loc = _full((batch, n), 0x5A5A, torch.int16)
    npa.error_locator_dev(n, dp, batch, loc.data_ptr(), ctx=gpu, stream=s)
    res["locator"] = (loc,)
    for name, locators in (("dev3", 0), ("dev3+locators", loc.data_ptr())):
        out, st = outbuf(), status()
        npa.reconstruct_batch_dev2(p, dbefore.data_ptr(), sl, stride, dp, locators, batch, out.data_ptr() + 64, ostride,
                                   ctx=gpu, stream=s, d_status=st.data_ptr())
        res[name] = (out, st)
    for name, locators in (("dev2", None), ("dev2+locators", loc.data_ptr())):
        out = outbuf()
        npa._raise(npa.lib().np_reconstruct_batch_dev2(gpu.handle, C.byref(p._c()), dbefore.data_ptr(), sl, stride, dp,
                                                       locators, batch, out.data_ptr() + 64, ostride, s or None))
        res[name] = (out,)
    out, st = outbuf(), status()
    npa.reconstruct_codewords_batch_dev(p, dcode.data_ptr(), sl, stride, dp, batch, out.data_ptr() + 64, ostride,
                                        ctx=gpu, stream=s, d_status=st.data_ptr())
    res["codewords"] = (out, st)
    # the host-mask call fails as a whole on the k - 1 payload: the decodable runs, then the whole batch
    out = outbuf()
    runs = [(0, 2), (3, 2)]
    for b0, count in runs:
        npa.reconstruct_batch_dev(p, dbefore.data_ptr() + b0 * stride, sl, stride, pres[b0:b0 + count].tobytes(), count,
                                  out.data_ptr() + 64 + b0 * ostride, ostride, ctx=gpu, stream=s)
    with pytest.raises(npa.NeedMoreShards) as ei:
        npa.reconstruct_batch_dev(p, dbefore.data_ptr(), sl, stride, pres.tobytes(), batch, out.data_ptr() + 64,
                                  ostride, ctx=gpu, stream=s)
    assert ei.value == npa.NeedMoreShards(k - 1, k, n)
    res["host-mask"] = (out,)
    buf, st = dbefore.clone(), status()
    npa.restore_shards_batch_dev(p, buf.data_ptr(), sl, stride, dp, batch, ctx=gpu, stream=s, d_status=st.data_ptr())
    res["restore"] = (buf, st)
    cnt, mp, st = _full(4 * batch + 128, GUARD), _full(batch * n + 128, GUARD), status()
    npa.verify_shards_batch_dev(p, dbefore.data_ptr(), sl, stride, dp, batch, cnt.data_ptr() + 64, ctx=gpu, stream=s,
                                d_mismatch=mp.data_ptr() + 64, d_status=st.data_ptr())
    res["verify"] = (cnt, mp, st)
    buf, out, cnt, mp, st = dbefore.clone(), outbuf(), _full(4 * batch + 128, GUARD), _full(batch * n + 128, GUARD), \
        status()
    npa.recover_batch_dev(p, buf.data_ptr(), sl, stride, dp, batch, ctx=gpu, stream=s, d_out=out.data_ptr() + 64,
                          out_stride=ostride, restore=True, d_bad_rows=cnt.data_ptr() + 64,
                          d_mismatch=mp.data_ptr() + 64, d_status=st.data_ptr())
    res["recover"] = (buf, out, cnt, mp, st)
    # decode_main: one mask row (payload 0's), its locator, 9 columns
    t = _dev(c.words.view(np.int16))
    dl = _dev(c.locators[0].view(np.int16))
    npa.decode_main_dev(t.data_ptr(), k, dp, dl.data_ptr(), n, 9, ctx=gpu, stream=s)
    res["decode_main"] = (t,)
    torch.cuda.synchronize()
    assert torch.equal(dbefore, _dev(_stage(c.pats, n, sl, stride)))  # the calls above only read it
    return res


def _check_device_outputs(c, sl, res):
    """The 0/1 outputs of _device_outputs against the oracle."""
    p = c.p
    n, k = p.n(), p.k()
    batch, stride, pay_len = len(c.pats), n * sl + 64, (sl // 2) * 2 * k
    ostride = pay_len + OUT_SLACK
    exp_rows, (flags, counts, status), pays = c.exp
    want_out = _want_out(pays, pay_len, ostride)
    assert np.array_equal(_as_u16(res["locator"][0]), c.locators)
    for call in ("dev3", "dev3+locators", "dev2", "dev2+locators", "recover"):
        out = res[call][1] if call == "recover" else res[call][0]
        _assert_out(_host(out), want_out, c.names, ostride, call)
    # the host-mask call never decoded the k - 1 payload: the same bytes
    _assert_out(_host(res["host-mask"][0]), want_out, c.names, ostride, "host-mask")
    code_out = _want_out([None if pays[b] is None else c.code_pay[b].tobytes() for b in range(batch)], pay_len, ostride)
    _assert_out(_host(res["codewords"][0]), code_out, c.names, ostride, "codewords")
    before = _stage(c.pats, n, sl, stride)
    restored = before.copy()
    for b in range(batch):
        view = restored[b * stride: b * stride + n * sl].reshape(n, sl)
        for v, data in (exp_rows[b] or {}).items():
            view[v] = np.frombuffer(data, np.uint8)
    assert not np.array_equal(before, restored)
    for call in ("restore", "recover"):
        got = _host(res[call][0])
        for b in range(batch):
            bad = np.flatnonzero(got[b * stride:(b + 1) * stride] != restored[b * stride:(b + 1) * stride])
            assert bad.size == 0, (call, b, c.names[b], bad.size, "rows", sorted(set((bad // sl).tolist()))[:8])
        assert np.array_equal(got, restored), call
    for call, cnt, mp in (("verify", res["verify"][0], res["verify"][1]), ("recover", res["recover"][2], res["recover"][3])):
        cnt, mp = _host(cnt), _host(mp)
        assert (cnt[:64] == GUARD).all() and (cnt[-64:] == GUARD).all() and (mp[:64] == GUARD).all() \
            and (mp[-64:] == GUARD).all(), call
        assert cnt[64:-64].copy().view(np.uint32).tolist() == counts.tolist(), call
        assert np.array_equal(mp[64:-64].reshape(batch, n), flags), call  # exactly 0 or 1
    for call in ("dev3", "dev3+locators", "codewords", "restore", "verify", "recover"):
        assert [tuple(int(x) for x in r) for r in _host(res[call][-1])] == status, call
    assert np.array_equal(_as_u16(res["decode_main"][0]), c.decoded)


def _presence_device(gpu, oracle, p, sl, offsets):
    import torch

    c = _presence_case(oracle, p.n(), p.k(), p.wanted_n, sl)
    ref = None
    for offset in offsets:
        for spelling in vc.SPELLINGS:
            pres = vc.spell(c.pres, spelling)
            assert np.array_equal(pres != 0, c.pres != 0)
            base = _full(16 + pres.size + 16, 0xEE)  # torch allocations are at least 256-byte aligned
            assert base.data_ptr() % 16 == 0
            base[offset:offset + pres.size] = _dev(pres.reshape(-1))
            res = _device_outputs(gpu, c, sl, base.data_ptr() + offset, pres)
            if ref is None:
                _check_device_outputs(c, sl, res)
                ref = res
            else:
                _same(res, ref, f"flags written as {spelling}, d_present {offset} past a 16-byte boundary")
            assert torch.equal(base[offset:offset + pres.size], _dev(pres.reshape(-1)))
    return c


@shapes
def test_presence_bytes_device(gpu, oracle, nw, kw, sl, enc_family, rec_family):
    """The device calls: np_reconstruct_batch_dev (host mask), _dev2 and _dev3
    with and without caller locators, np_reconstruct_codewords_batch_dev,
    np_error_locator_dev, np_decode_main_dev, and the restore, verify and
    recover calls."""
    p = _params(nw, kw, sl, enc_family, rec_family)
    _presence_device(gpu, oracle, p, sl, (0,))


@pytest.mark.parametrize("nw,kw,sl,enc_family,rec_family", RESIDENT)
def test_presence_bytes_unaligned_flags(gpu, oracle, nw, kw, sl, enc_family, rec_family):
    """d_present one byte past a 16-byte aligned base: every flag row starts at
    1 mod 4, the byte path of lane_rows_present.  The aligned 0/1 call is the
    reference."""
    p = _params(nw, kw, sl, enc_family, rec_family)
    _presence_device(gpu, oracle, p, sl, (0, 1))


@shapes
def test_presence_bytes_host(gpu, oracle, nw, kw, sl, enc_family, rec_family):
    """np_reconstruct_batch_host and np_recover_batch_host, with and without
    `status`; without it the k - 1 payload fails the call up front with the
    detail (k - 1, k, n) whatever the flag bytes are, and nothing is written."""
    import torch

    p = _params(nw, kw, sl, enc_family, rec_family)
    n, k = p.n(), p.k()
    c = _presence_case(oracle, n, k, p.wanted_n, sl)
    exp_rows, (flags, counts, status), pays = c.exp
    torch.cuda.synchronize()
    ref = None
    for spelling in vc.SPELLINGS:
        res = {}
        h = HostBatch(p, sl, c.pats, vc.spell(c.pres, spelling))
        h.recover(gpu)
        if ref is None:
            h.check(c.exp, True, True, tag="recover_batch_host")
        res["recover"] = h.buffers()
        h.fresh()
        for b0, count in ((0, 2), (3, 2)):  # the decodable runs, no status: nothing fails
            h.recover(gpu, with_status=False, b0=b0, count=count)
        res["recover-no-status"] = h.buffers()
        if ref is None:
            assert (h.st == -1).all() and (h.cnt[64 + 8:64 + 12] == GUARD).all() \
                and (h.mp[64 + 2 * n:64 + 3 * n] == GUARD).all()
            # the k - 1 payload was not part of a call: give it its entries, then compare as above
            h.st[:] = np.asarray(status, np.int32)
            h.cnt[64 + 8:64 + 12] = 0xFF
            h.mp[64 + 2 * n:64 + 3 * n] = 0
            h.check(c.exp, True, True, tag="recover_batch_host without status")
        h.fresh()
        for what, call in (("recover", lambda: h.recover(gpu, with_status=False)), ("reconstruct", lambda: h.reconstruct(gpu))):
            with pytest.raises(npa.NeedMoreShards) as ei:
                call()
            assert ei.value == npa.NeedMoreShards(k - 1, k, n), (what, spelling)
            assert np.array_equal(h.sh, h.before) and (h.out == GUARD).all() and (h.cnt == GUARD).all() \
                and (h.mp == GUARD).all() and (h.st == -1).all(), (what, spelling)
        for b0, count in ((0, 2), (3, 2)):
            h.reconstruct(gpu, b0=b0, count=count)
        if ref is None:
            h.check((exp_rows, (flags, counts, status), pays), False, False, with_status=False,
                    tag="reconstruct_batch_host")
        res["reconstruct"] = h.buffers()
        if ref is None:
            ref = res
        else:
            _same(res, ref, f"flags written as {spelling}")


@functools.lru_cache(maxsize=None)
def _contexts():
    return npa.Context(0), npa.Context(0)


@shapes
def test_presence_bytes_multi(gpu, oracle, nw, kw, sl, enc_family, rec_family):
    """np_reconstruct_batch_multi and np_recover_batch_multi over two contexts
    on device 0 (ranges of 3 and 2 payloads)."""
    import torch

    p = _params(nw, kw, sl, enc_family, rec_family)
    n, k = p.n(), p.k()
    c = _presence_case(oracle, n, k, p.wanted_n, sl)
    exp_rows, (flags, counts, status), pays = c.exp
    ctxs = _contexts()
    batch, stride, pay_len = len(c.pats), n * sl + 64, (sl // 2) * 2 * k
    ostride = pay_len + OUT_SLACK
    ranges = [npa.batch_split(batch, 2, i) for i in range(2)]
    assert ranges == [(0, 3), (3, 2)]
    before = _stage(c.pats, n, sl, stride)[:batch * stride].reshape(batch, stride)
    ref = None
    for spelling in vc.SPELLINGS:
        pres = vc.spell(c.pres, spelling)
        d_pr = [_dev(pres[b0:b0 + cnt]) for b0, cnt in ranges]
        res = {}
        for call in ("reconstruct", "recover"):
            d_sh = [_dev(before[b0:b0 + cnt]) for b0, cnt in ranges]
            d_out = [_full((cnt, ostride), GUARD) for _, cnt in ranges]
            d_cnt = [_full(4 * cnt, GUARD) for _, cnt in ranges]
            d_map = [_full((cnt, n), GUARD) for _, cnt in ranges]
            d_st = [_full((cnt, 2), -1, torch.int32) for _, cnt in ranges]
            ptrs = [[t.data_ptr() for t in ts] for ts in (d_sh, d_pr, d_out, d_cnt, d_map, d_st)]
            torch.cuda.synchronize()
            if call == "reconstruct":
                npa.reconstruct_batch_multi(ctxs, p, ptrs[0], sl, stride, ptrs[1], batch, ptrs[2], ostride, ptrs[5])
            else:
                npa.recover_batch_multi(ctxs, p, ptrs[0], sl, stride, ptrs[1], batch, d_out=ptrs[2], out_stride=ostride,
                                        restore=True, d_bad_rows=ptrs[3], d_mismatch=ptrs[4], d_status=ptrs[5])
            res[call] = tuple(np.concatenate([_host(t) for t in ts]) for ts in (d_sh, d_out, d_cnt, d_map, d_st))
        if ref is None:
            for call, (sh, out, cnt, mp, st) in res.items():
                want = before.copy()
                if call == "recover":
                    for b in range(batch):
                        view = want[b, :n * sl].reshape(n, sl)
                        for v, data in (exp_rows[b] or {}).items():
                            view[v] = np.frombuffer(data, np.uint8)
                assert np.array_equal(sh, want), call
                want_out = _want_out(pays, pay_len, ostride)[64:-64].reshape(batch, ostride)
                assert np.array_equal(out, want_out), call
                assert [tuple(int(x) for x in r) for r in st] == status, call
                if call == "recover":
                    assert cnt.view(np.uint32).tolist() == counts.tolist() and np.array_equal(mp, flags)
                else:
                    assert (cnt == GUARD).all() and (mp == GUARD).all()
            ref = res
        else:
            _same(res, ref, f"flags written as {spelling}")


@functools.lru_cache(maxsize=None)
def _ragged_presence_case(oracle, n, k, wn):
    rng = np.random.default_rng(19 * n + k + wn)
    masks = vc.masks(rng, n, k, wn)
    per_item = [(rng.integers(0, 256, (n, RAGGED_LENGTHS[i % 3]), dtype=np.uint8), pr)
                for i, (_, pr) in enumerate(masks)]
    return Ragged(npa.CodeParams(n, k, wn), per_item).expected(oracle)


@pytest.mark.parametrize("nw,kw,sl,enc_family,rec_family", RAGGED)
def test_presence_bytes_ragged(gpu, oracle, nw, kw, sl, enc_family, rec_family):
    """The four ragged calls; items of 600, 512 and 2 bytes per row."""
    p = _params(nw, kw, sl, enc_family, rec_family)
    r = _ragged_presence_case(oracle, p.n(), p.k(), p.wanted_n)
    assert r.counts[2] == UNDECODABLE and r.counts[0] > 0
    pres01 = np.stack([pr for _, pr in r.per_item])
    ref = None
    for spelling in vc.SPELLINGS:
        dpres = _dev(vc.spell(pres01, spelling))
        res = r.run(gpu, dpres.data_ptr())
        if ref is None:
            r.check(res)
            ref = res
        else:
            _same(res, ref, f"flags written as {spelling}")


# ------------------------------------- (c) every bit position of the verify ----
@functools.lru_cache(maxsize=None)
def _codeword_rows(oracle, n, k, wn, sl):
    rng = np.random.default_rng(23 * n + k + wn + sl)
    st, enc = oracle.encode(rng.integers(0, 256, (sl // 2) * 2 * k, dtype=np.uint8).tobytes(), n, k, wn)
    assert st == 0 and len(enc[0]) == sl
    rows = np.full((n, sl), FILL, np.uint8)
    rows[:wn] = np.frombuffer(b"".join(enc), np.uint8).reshape(wn, sl)
    rows.setflags(write=False)
    return rows


class Flipped:
    """One payload per byte position p of a row: bit p % 8 of byte p flipped in
    parity row k + (7 p + 3) % (wanted_n - k); absent rows hold FILL.  The
    batch is the largest buffer of the module (368 MB at (1024, 342)), so the
    calls run on it in place and `unchanged_but` undoes the flips and compares
    it with the staged payload in pieces."""

    def __init__(self, code, pres, k, wn, sl):
        import torch

        n = code.shape[0]
        self.n, self.sl, self.batch = n, sl, sl
        self.stride = n * sl + 64  # rows of 74 bytes lie at odd-dword addresses by themselves
        staged = np.full((n, sl), FILL, np.uint8)
        staged[pres != 0] = code[pres != 0]
        one = np.full(self.stride, FILL, np.uint8)
        one[:n * sl] = staged.reshape(-1)
        self.one = _dev(one)
        self.buf = self.one.repeat(sl, 1)
        self.pos = torch.arange(sl, device="cuda")
        self.hit_d = k + (7 * self.pos + 3) % (wn - k)
        self.hit = self.hit_d.cpu().numpy()
        self.dpres = _dev(np.tile(pres, (sl, 1)))
        self._flip()

    def _flip(self):
        import torch

        self.buf[self.pos, self.hit_d * self.sl + self.pos] ^= (1 << (self.pos % 8)).to(torch.uint8)

    def verdicts(self, gpu, p):
        """(call, counts, map) through np_verify_shards_batch_dev and through
        np_recover_batch_dev with restore and verdict requested."""
        import torch

        for call in ("verify", "recover"):
            cnt, mp = _full(self.batch, 7, torch.int32), _full((self.batch, self.n), GUARD)
            if call == "verify":
                npa.verify_shards_batch_dev(p, self.buf.data_ptr(), self.sl, self.stride, self.dpres.data_ptr(),
                                            self.batch, cnt.data_ptr(), ctx=gpu, stream=_stream(),
                                            d_mismatch=mp.data_ptr())
            else:
                npa.recover_batch_dev(p, self.buf.data_ptr(), self.sl, self.stride, self.dpres.data_ptr(), self.batch,
                                      ctx=gpu, stream=_stream(), restore=True, d_bad_rows=cnt.data_ptr(),
                                      d_mismatch=mp.data_ptr())
            yield call, _host(cnt).view(np.uint32), _host(mp)

    def unchanged_but(self, rows):
        """After the calls: no byte of the batch changed outside `rows`; returns
        those rows of every payload, (batch, len(rows), shard_len), on the host."""
        import torch

        self._flip()  # back to `batch` copies of the staged payload
        n, sl = self.n, self.sl
        keep = torch.ones(self.stride, dtype=torch.bool, device="cuda")
        for v in rows:
            keep[v * sl:(v + 1) * sl] = False
        for b0 in range(0, self.batch, 64):
            piece = self.buf[b0:b0 + 64]
            assert bool((piece[:, keep] == self.one[keep]).all()), f"payloads {b0} .. {b0 + 63} changed outside rows {rows}"
        idx = torch.tensor([v * sl + j for v in rows for j in range(sl)], dtype=torch.long, device="cuda")
        return _host(self.buf[:, idx]).reshape(self.batch, len(rows), sl)


@pytest.mark.parametrize("nw,kw,sl,family", [(256, 86, SL, FAST), (1024, 342, SL, FAST), (60, 20, SL, SMALL),
                                             (60, 20, 2 * 37, SMALL)])
def test_verify_every_bit_position(gpu, oracle, nw, kw, sl, family):
    """Copy mode -- every row below wanted_n present -- so exactly the altered
    parity row mismatches: k_encode_verify and k_encode_recover on the fast
    shapes, k_compare_present_rows on (60, 20)."""
    p = _params(nw, kw, sl, family, family)
    n, k, wn = p.n(), p.k(), p.wanted_n
    code = _codeword_rows(oracle, n, k, wn, sl)
    pres = np.zeros(n, np.uint8)
    pres[:wn] = 1
    f = Flipped(code, pres, k, wn, sl)
    # the flipped rows walk all 16 positions of a row group and every parity segment
    assert len(set((f.hit % 16).tolist())) == 16 and set((f.hit // k).tolist()) == set(range(1, (wn - 1) // k + 1))
    want = np.zeros((sl, n), np.uint8)
    want[np.arange(sl), f.hit] = 1
    for call, cnt, mp in f.verdicts(gpu, p):
        missed = np.flatnonzero(cnt != 1)
        assert missed.size == 0, (call, "byte positions whose flipped bit gave no single mismatch", missed[:16].tolist(),
                                  cnt[missed[:16]].tolist())
        wrong = np.flatnonzero((mp != want).any(axis=1))
        assert wrong.size == 0, (call, "byte positions with a wrong map", wrong[:16].tolist())
    f.unchanged_but([])  # nothing absent below wanted_n: nothing restored


def test_verify_every_bit_position_rows_absent(gpu, oracle):
    """(1024, 342) with rows 3, 77 and 200 absent: a flipped bit spreads, so
    the flagged set of the payloads at p = 25 j comes from the oracle's
    encode(reconstruct(received)); every other payload must flag a row."""
    nw, kw, sl = 1024, 342, SL
    p = _params(nw, kw, sl, FAST, FAST)
    n, k, wn = p.n(), p.k(), p.wanted_n
    code = _codeword_rows(oracle, n, k, wn, sl)
    gone = [3, 77, 200]
    pres = np.zeros(n, np.uint8)
    pres[:wn] = 1
    pres[gone] = 0
    f = Flipped(code, pres, k, wn, sl)
    exact = list(range(0, sl, 25))
    assert len(exact) == 24
    flags, rows_want = {}, {}
    for pos in exact:
        rows = code.copy()
        rows[f.hit[pos], pos] ^= np.uint8(1 << (pos % 8))
        pay, absent, fl = _expected_one(oracle, n, k, wn, rows, pres)
        assert pay is not None and sorted(absent) == gone and fl.any()
        flags[pos] = fl
        rows_want[pos] = np.stack([np.frombuffer(absent[v], np.uint8) for v in gone])
    for call, cnt, mp in f.verdicts(gpu, p):
        for pos in exact:
            assert int(cnt[pos]) == int(flags[pos].sum()), (call, pos)
            assert np.array_equal(mp[pos], flags[pos]), (call, pos, np.flatnonzero(mp[pos])[:8].tolist())
        missed = np.flatnonzero(cnt < 1)
        assert missed.size == 0, (call, "byte positions whose flipped bit went unseen", missed[:16].tolist())
        assert (cnt == mp.sum(axis=1)).all() and (cnt <= wn - k).all(), call
    # the recover call wrote the three absent rows and nothing else
    written = f.unchanged_but(gone)
    for pos in exact:
        assert np.array_equal(written[pos], rows_want[pos]), pos
    assert (written != FILL).any(axis=2).all()

"""np_recover_batch_dev / np_rs_recover: the payload, the absent rows and the
verdict from one decode.  Each requested output equals, byte for byte, what
np_reconstruct_batch_dev3, np_restore_shards_batch_dev and
np_verify_shards_batch_dev give on the same received rows -- checked against
the oracle's ReedSolomon::reconstruct and ReedSolomon::encode(reconstruct(..))
(mod.rs:162-239, mod.rs:117-157) for any received bytes, and once against the
three calls themselves.  An output that was not requested keeps its fill, the
shard buffer changes in the restored rows only, and nothing around the results
is written.

Each shape is one batch whose payloads carry the patterns of `_patterns`; the
oracle's answers are computed once per shape and shared by the seven request
combinations, each with and without d_status and (where it verifies) with and
without d_mismatch.  Direct shapes (k in {64, 128, 256}) run the masked, the
verify or -- restore and verify together -- the recover encode; the others the
ordinary encode into scratch, then the copy and / or the compare."""
import functools
import itertools

import numpy as np
import pytest

import novelpoly_amd as npa
from test_gpu_restore import expected_rows
from test_gpu_verify import SlicesCase, _codeword, _flip, expected_case

pytestmark = pytest.mark.gpu

FILL = 0x5A
GUARD = 0xA5
SL = 2 * 300  # one full 256-column tile plus a partial one
UNDECODABLE = 0xFFFFFFFF
OUT_SLACK = 32  # out_stride - (shard_len / 2) * 2k

# (n_wanted, k_wanted, shard_len)
DIRECT = [(256, 86, SL), (512, 128, SL), (1024, 342, SL),  # n = 4k
          (600, 256, SL),    # n1024 k256, wanted_n inside segment 2
          (512, 256, SL),    # n = 2k
          (2048, 256, SL)]   # n = 8k: the runtime shift loop
# k = 16 (small), k = 512, k = 1024 (resident)
FALLBACK = [(60, 20, SL), (1024, 512, SL), (4096, 1366, 2 * 260)]

# (d_out, restore, verify): the seven non-empty requests
COMBOS = [c for c in itertools.product((False, True), repeat=3) if any(c)]


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _patterns(oracle, rng, n, k, wn, sl):
    """[(name, rows n x sl, present n)] -- rows >= wanted_n are never present."""
    syms = sl // 2

    def rand_rows():
        return rng.integers(0, 256, (n, sl), dtype=np.uint8)

    def pres_without(absent):
        p = np.zeros(n, np.uint8)
        p[:wn] = 1
        p[np.asarray(absent, dtype=np.int64)] = 0
        return p

    def flip(rows, v):
        _flip(rows, int(v), int(rng.integers(0, syms)), rng)

    out = []
    code = _codeword(oracle, rng, n, k, wn, sl)
    # 1: one 16-row window of parity segment 1 (the 16 rows of one wave and pass)
    # with an absent row, an altered present row and intact present rows
    w0 = k + 16 * int(rng.integers(0, max(1, (min(2 * k, wn) - k) // 16)))
    a, f = rng.choice(np.arange(w0, min(w0 + 16, wn)), 2, replace=False)
    rows = code.copy()
    flip(rows, f)
    out.append(("window", rows, pres_without([a])))
    # 2: a segment that only stores (all its rows absent) next to one that only
    # compares (all present, one row altered); n / k in {4, 8}
    if n // k >= 4 and wn > 2 * k:
        rows = code.copy()
        flip(rows, rng.integers(2 * k, min(3 * k, wn)))
        out.append(("store-segment+compare-segment", rows, pres_without(np.arange(k, 2 * k))))
    # 3: absent systematic rows together with an altered present parity row
    rows = code.copy()
    flip(rows, rng.integers(k, wn))
    out.append(("systematic-absent+parity-flip", rows, pres_without(rng.choice(k, min(3, k - 1), replace=False))))
    # 4: copy mode -- every systematic row present, the present parity rows random, half of the parity rows absent
    rows = code.copy()
    rows[k:] = rng.integers(0, 256, (n - k, sl), dtype=np.uint8)
    out.append(("copy-mode", rows, pres_without(k + rng.choice(wn - k, max(1, (wn - k) // 2), replace=False))))
    # 5: random bytes with more than k rows present
    out.append(("random", rand_rows(), pres_without(rng.choice(wn, min((n - k) // 2, wn - k - 1), replace=False))))
    # 6: exactly k rows present
    out.append(("exactly-k", rand_rows(), pres_without(rng.choice(wn, wn - k, replace=False))))
    # 7: k - 1 rows present: NeedMoreShards, nothing touched
    out.append(("k-1", rand_rows(), pres_without(rng.choice(wn, wn - k + 1, replace=False))))
    # 8: every row present: no store, compares only (two parity rows altered)
    rows = code.copy()
    for v in rng.choice(np.arange(k, wn), 2, replace=False):
        flip(rows, v)
    out.append(("all-present", rows, pres_without([])))
    # 9: every parity row absent: stores only
    out.append(("parity-absent", code, pres_without(np.arange(k, wn))))
    return out


def expected_recover(oracle, p, sl, pats):
    """The oracle's answers for the batch `pats` [(name, rows, present)]:
    (restored rows per payload, (flags, counts, status), payloads), read only."""
    n, k = p.n(), p.k()
    rows = expected_rows(oracle, p, sl, pats)
    case = expected_case(oracle, p, sl, [(name, r, pr, None) for name, r, pr in pats])
    pays = []
    for name, r, pr in pats:
        st, pay = oracle.reconstruct([r[v].tobytes() if pr[v] else None for v in range(n)], n, k)
        assert st in (0, npa.NeedMoreShards.code)
        pays.append(None if st else pay)
    for b in range(len(pats)):  # the three agree on which payloads decode
        assert (rows[b] is None) == (pays[b] is None) == (case[1][b] == UNDECODABLE) == (case[2][b][0] != 0)
    return rows, case, pays


def run_recover(gpu, p, sl, pats, expected, offset=0, slack=64, combos=COMBOS, label="", out_offset=0,
                out_slack=OUT_SLACK, variants=None):
    """One batch of `pats` under `p` against `expected` (expected_recover), once
    per request combination, with and without d_status and d_mismatch: every
    byte of the shard buffer, of d_out, of the counts and the map and their
    guards, and the statuses.  d_out sits `out_offset` bytes behind its 64 guard
    bytes with out_stride = payload length + `out_slack`; `variants`: the calls
    as [((d_out, restore, verify), d_status given, d_mismatch given)] in place
    of every one of `combos`."""
    import torch

    exp_rows, (want_flags, want_counts, status), pays = expected
    n, k = p.n(), p.k()
    batch, stride = len(pats), n * sl + slack
    pay_len = (sl // 2) * 2 * k
    ostride = pay_len + out_slack
    before = np.full(offset + batch * stride + 64, FILL, np.uint8)
    for b, (name, rows, pr) in enumerate(pats):
        view = before[offset + b * stride: offset + b * stride + n * sl].reshape(n, sl)
        view[pr != 0] = rows[pr != 0]
    restored = before.copy()  # every byte but the restored rows stays as it was
    for b in range(batch):
        view = restored[offset + b * stride: offset + b * stride + n * sl].reshape(n, sl)
        for v, data in (exp_rows[b] or {}).items():
            view[v] = np.frombuffer(data, np.uint8)
    want_out = np.full((batch, ostride), GUARD, np.uint8)
    for b, pay in enumerate(pays):
        if pay is not None:
            assert len(pay) == pay_len
            want_out[b, :pay_len] = np.frombuffer(pay, np.uint8)
    dpres = _dev(np.stack([pr for _, _, pr in pats]))
    dbefore = _dev(before)
    s = torch.cuda.current_stream().cuda_stream
    if variants is None:
        variants = [v for v in itertools.product(combos, (True, False), (True, False)) if v[0][2] or not v[2]]
    for (with_out, restore, verify), with_status, with_map in variants:
        assert verify or not with_map
        tag = f"{label} out {with_out}, restore {restore}, verify {verify}, status {with_status}, map {with_map}"
        buf = dbefore.clone()
        st_d = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
        cnt_d = torch.full((64 + 4 * batch + 64,), GUARD, dtype=torch.uint8, device="cuda")
        map_d = torch.full((64 + batch * n + 64,), GUARD, dtype=torch.uint8, device="cuda")
        out_d = torch.full((64 + out_offset + batch * ostride + 64,), GUARD, dtype=torch.uint8, device="cuda")
        npa.recover_batch_dev(p, buf.data_ptr() + offset, sl, stride, dpres.data_ptr(), batch, ctx=gpu, stream=s,
                              d_out=out_d.data_ptr() + 64 + out_offset if with_out else 0,
                              out_stride=ostride if with_out else 0,
                              restore=restore, d_bad_rows=cnt_d.data_ptr() + 64 if verify else 0,
                              d_mismatch=map_d.data_ptr() + 64 if with_map else 0,
                              d_status=st_d.data_ptr() if with_status else 0)
        got, cnt, mp, out = _host(buf), _host(cnt_d), _host(map_d), _host(out_d)
        # the shard buffer, whole: the restored rows and nothing else
        want = restored if restore else before
        for b, (name, _, pr) in enumerate(pats):
            lo, hi = offset + b * stride, offset + (b + 1) * stride
            if not np.array_equal(got[lo:hi], want[lo:hi]):
                bad = np.flatnonzero(got[lo:hi] != want[lo:hi])
                rows_bad = sorted(set((bad // sl).tolist()))[:8]
                raise AssertionError(f"{tag}: payload {b} ({name}): {bad.size} shard bytes differ, rows {rows_bad} "
                                     f"(absent: {[v for v in rows_bad if v < n and not pr[v]]})")
        assert np.array_equal(got[:offset], want[:offset]) and np.array_equal(got[-64:], want[-64:]), tag
        # the payloads
        assert (out[:64 + out_offset] == GUARD).all() and (out[-64:] == GUARD).all(), tag
        if with_out:
            o = out[64 + out_offset:-64].reshape(batch, ostride)
            for b, (name, _, _) in enumerate(pats):
                assert np.array_equal(o[b], want_out[b]), (tag, b, name, int(np.flatnonzero(o[b] != want_out[b])[0]))
        else:
            assert (out == GUARD).all(), tag
        # the verdict
        assert (cnt[:64] == GUARD).all() and (cnt[-64:] == GUARD).all(), tag
        if verify:
            got_counts = cnt[64:-64].copy().view(np.uint32)
            wrong = [(int(b), pats[b][0]) for b in np.flatnonzero(got_counts != want_counts)]
            assert got_counts.tolist() == want_counts.tolist(), (tag, "payloads whose count differs", wrong)
        else:
            assert (cnt == GUARD).all(), tag
        if with_map:
            assert (mp[:64] == GUARD).all() and (mp[-64:] == GUARD).all(), tag
            m = mp[64:-64].reshape(batch, n)
            for b, (name, _, _) in enumerate(pats):
                assert np.array_equal(m[b], want_flags[b]), \
                    (tag, b, name, np.flatnonzero(m[b]).tolist()[:8], np.flatnonzero(want_flags[b]).tolist()[:8])
        else:
            assert (mp == GUARD).all(), tag
        if with_status:
            stat = _host(st_d)
            assert [tuple(int(x) for x in r) for r in stat] == status, tag
            errs = npa.payload_errors(p, stat)
            for b, (code, have) in enumerate(status):
                assert errs[b] == (npa.NeedMoreShards(have, k, n) if code else None), (tag, b)
        else:
            assert bool((st_d == -1).all()), tag


@functools.lru_cache(maxsize=None)
def _shape_case(oracle, n, k, wn, sl):
    """The shape's batch and the oracle's answers, computed once (read only)."""
    p = npa.CodeParams(n, k, wn)
    rng = np.random.default_rng(1000 * n + 10 * k + wn + sl)
    pats = _patterns(oracle, rng, n, k, wn, sl)
    exp = expected_recover(oracle, p, sl, pats)
    counts = dict(zip((name for name, _, _ in pats), exp[1][1].tolist()))
    # the patterns do what their names say
    assert counts["window"] == 1 and counts["all-present"] == 2 and counts["parity-absent"] == 0
    assert counts["exactly-k"] == 0 and counts["k-1"] == UNDECODABLE and counts["copy-mode"] > 0
    assert counts.get("store-segment+compare-segment", 1) == 1
    return p, pats, exp


def _run_shape(gpu, oracle, nw, kw, sl, offset=0, slack=64):
    d = npa.CodeParams.derive_parameters(nw, kw)
    p, pats, exp = _shape_case(oracle, d.n(), d.k(), d.wanted_n, sl)
    run_recover(gpu, p, sl, pats, exp, offset, slack, label=f"{nw},{kw}")


@pytest.mark.parametrize("nw,kw,sl", DIRECT)
def test_recover_direct(gpu, oracle, nw, kw, sl):
    _run_shape(gpu, oracle, nw, kw, sl)


def test_recover_direct_unaligned_rows(gpu, oracle):
    """Rows at odd-dword addresses and a second tile of one column: odd chunk
    count, d_shards 2 bytes into its allocation, batch_stride = n * shard_len + 2."""
    _run_shape(gpu, oracle, 1024, 342, 2 * 257, offset=2, slack=2)


@pytest.mark.parametrize("nw,kw,sl", FALLBACK)
def test_recover_fallback(gpu, oracle, nw, kw, sl):
    _run_shape(gpu, oracle, nw, kw, sl)


@pytest.mark.parametrize("n,k,wn", [(1024, 256, 768), (512, 64, 320)])
def test_recover_segment_purposes(gpu, oracle, n, k, wn):
    """n / k in {4, 8} with wanted_n on a segment boundary: segment 1 only
    stores (all its rows absent), segment 2 only compares (all present, one row
    altered), the segments at and above wanted_n do neither; at n / k = 8
    segment 3 stores and compares, segment 4 only compares intact rows."""
    p = npa.CodeParams(n, k, wn)
    rng = np.random.default_rng(n + k + wn)
    rows = _codeword(oracle, rng, n, k, wn, SL)
    hit = int(rng.integers(2 * k, 3 * k))
    _flip(rows, hit, int(rng.integers(0, SL // 2)), rng)
    pres = np.zeros(n, np.uint8)
    pres[:wn] = 1
    pres[k:2 * k] = 0
    if wn > 3 * k:
        pres[3 * k + rng.choice(k, k // 2, replace=False)] = 0
    pats = [("segments", rows, pres)]
    exp = expected_recover(oracle, p, SL, pats)
    assert np.flatnonzero(exp[1][0][0]).tolist() == [hit]
    run_recover(gpu, p, SL, pats, exp, label=f"n{n} k{k} wanted {wn}")


def test_recover_equals_the_three_calls(gpu):
    """Random bytes at (1024, 342): the three existing device calls on copies of
    the buffer give exactly the new call's outputs."""
    import torch

    p = npa.CodeParams.derive_parameters(1024, 342)
    n, k, wn = p.n(), p.k(), p.wanted_n
    batch, sl, stride = 8, SL, n * SL + 64
    pay_len = (sl // 2) * 2 * k
    rng = np.random.default_rng(342)
    before = rng.integers(0, 256, batch * stride, dtype=np.uint8)
    pres = np.ones((batch, n), np.uint8)
    for b in range(batch):  # 342 .. 349 absent rows, and the last payload one row short of k
        pres[b, rng.choice(wn, 342 + b if b < batch - 1 else wn - k + 1, replace=False)] = 0
    dpres, dbefore = _dev(pres), _dev(before)
    s = torch.cuda.current_stream().cuda_stream

    def outputs():
        return (torch.full((batch, pay_len), GUARD, dtype=torch.uint8, device="cuda"),
                torch.full((batch,), 7, dtype=torch.int32, device="cuda"),
                torch.full((batch, n), GUARD, dtype=torch.uint8, device="cuda"),
                torch.full((batch, 2), -1, dtype=torch.int32, device="cuda"))

    out_a, cnt_a, map_a, st_a = outputs()
    st_r, st_v = st_a.clone(), st_a.clone()
    buf_r = dbefore.clone()
    npa.reconstruct_batch_dev2(p, dbefore.data_ptr(), sl, stride, dpres.data_ptr(), 0, batch, out_a.data_ptr(), pay_len,
                               ctx=gpu, stream=s, d_status=st_a.data_ptr())
    npa.verify_shards_batch_dev(p, dbefore.data_ptr(), sl, stride, dpres.data_ptr(), batch, cnt_a.data_ptr(), ctx=gpu,
                                stream=s, d_mismatch=map_a.data_ptr(), d_status=st_v.data_ptr())
    npa.restore_shards_batch_dev(p, buf_r.data_ptr(), sl, stride, dpres.data_ptr(), batch, ctx=gpu, stream=s,
                                 d_status=st_r.data_ptr())
    out_b, cnt_b, map_b, st_b = outputs()
    buf_b = dbefore.clone()
    npa.recover_batch_dev(p, buf_b.data_ptr(), sl, stride, dpres.data_ptr(), batch, ctx=gpu, stream=s,
                          d_out=out_b.data_ptr(), out_stride=pay_len, restore=True, d_bad_rows=cnt_b.data_ptr(),
                          d_mismatch=map_b.data_ptr(), d_status=st_b.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b) and torch.equal(buf_r, buf_b)
    assert torch.equal(cnt_a, cnt_b) and torch.equal(map_a, map_b)
    assert torch.equal(st_a, st_b) and torch.equal(st_r, st_b) and torch.equal(st_v, st_b)
    # the batch is not trivial: rows were written, rows mismatch, one payload is undecodable
    assert not torch.equal(buf_b, dbefore) and int(cnt_b[0]) > 0 and int(cnt_b[-1]) == -1
    assert bool((out_b[-1] == GUARD).all()) and not bool((out_b[0] == GUARD).all())


@pytest.mark.parametrize("nw,kw", [(1024, 342), (60, 20)])
def test_recover_host_single(gpu, oracle, nw, kw):
    """ReedSolomon.recover on random bytes with odd-length shards (zero padded
    like WrappedShard): the payload, all wanted_n shards and the mismatching
    rows against the oracle, and NeedMoreShards with the reference's fields."""
    p = npa.CodeParams.derive_parameters(nw, kw)
    n, k, wn = p.n(), p.k(), p.wanted_n
    rng = np.random.default_rng(nw + kw)
    odd = SL - 1
    pres = np.ones(wn, bool)
    pres[rng.choice(wn, min((n - k) // 2, wn - k - 1), replace=False)] = False
    recv = [rng.integers(0, 256, odd, dtype=np.uint8).tobytes() if pres[v] else None for v in range(wn)]
    padded = [None if s is None else s + b"\x00" for s in recv] + [None] * (n - wn)
    st, pay = oracle.reconstruct(padded, n, k)
    assert st == 0
    st, enc = oracle.encode(pay, n, k, wn)
    assert st == 0
    want_shards = [padded[v] if pres[v] else enc[v] for v in range(wn)]
    want_rows = [v for v in range(wn) if pres[v] and padded[v] != enc[v]]
    assert want_rows and all(v >= k for v in want_rows)
    rs = p.make_encoder(gpu)
    got = rs.recover(recv)
    assert got[0] == pay and got[1] == want_shards and got[2] == want_rows
    # what the three separate calls return
    assert got == (rs.reconstruct(recv), rs.restore_shards(recv), rs.mismatched_shards(recv))
    if kw == npa.recoverablity_subset_size(nw):
        assert npa.recover(recv, nw, ctx=gpu) == got
    short = list(recv)
    for v in np.flatnonzero(pres)[k - 1:]:
        short[v] = None
    with pytest.raises(npa.NeedMoreShards) as ei:
        rs.recover(short)
    assert ei.value == npa.NeedMoreShards(k - 1, k, n)


@pytest.mark.parametrize("nw,kw,batch,scratch", [(256, 86, 1100, 1 << 20), (1024, 512, 520, 2 << 20)])
def test_recover_slices(gpu, nw, kw, batch, scratch):
    """Payloads of 1 MiB.  (256, 86), direct: 1100 of them are two uneven slices
    of the 1 GiB payload scratch of an MI355X, as test_restore_slices.
    (1024, 512): scratch rows of 2 MiB per payload, so 520 of them are slices of
    512 and 8.  Restore and verify without d_out run per slice at
    d_shards + b0 * batch_stride, with the map and the status of the caller at
    their slice offsets or the call's own; with d_out the direct shape is one
    slice and the other is sliced as before.  SlicesCase works the slice length
    out from the device's memory as the context does, and asserts that the batch
    is more than one slice and that every slice holds every payload class.
    Compared on the device."""
    import torch

    c = SlicesCase(gpu, nw, kw, batch, scratch)
    s = torch.cuda.current_stream().cuda_stream
    for with_out, given in ((False, True), (False, False), (True, True)):
        tag = f"out {with_out}, map and status {given}"
        cnt = torch.full((batch,), 7, dtype=torch.int32, device="cuda")
        mp = torch.full((batch, c.n), GUARD, dtype=torch.uint8, device="cuda")
        st = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
        out = torch.full((batch, c.plen), GUARD, dtype=torch.uint8, device="cuda") if with_out else None
        npa.recover_batch_dev(c.p, c.work.data_ptr(), c.sl, c.n * c.sl, c.pres.data_ptr(), batch, ctx=gpu, stream=s,
                              d_out=out.data_ptr() if with_out else 0, out_stride=c.plen if with_out else 0,
                              restore=True, d_bad_rows=cnt.data_ptr(), d_mismatch=mp.data_ptr() if given else 0,
                              d_status=st.data_ptr() if given else 0)
        torch.cuda.synchronize()
        assert torch.equal(cnt, c.counts), (tag, (cnt != c.counts).nonzero()[:8].tolist())
        assert torch.equal(c.work, c.want), (tag, (c.work != c.want).any(dim=2).nonzero()[:8].tolist())
        if given:
            assert torch.equal(mp, c.flags) and torch.equal(st, c.status), tag
        else:
            assert bool((mp == GUARD).all()) and bool((st == -1).all()), tag
        if with_out:
            assert torch.equal(out[~c.c], c.pay[~c.c]) and bool((out[c.c] == GUARD).all()), tag
        del out
        c.blank()

"""np_restore_shards_batch_dev / np_rs_restore_shards: the absent rows below
wanted_n of every decodable payload become the rows of the reference's
ReedSolomon::encode(ReedSolomon::reconstruct(received)) (mod.rs:117-157 after
mod.rs:162-239), byte for byte against the oracle for any received bytes, and
no other byte of the caller's shard buffer changes.

Each shape is one batch whose payloads carry the erasure patterns of
`_patterns`; the shard buffer has 64 spare bytes per payload, and absent rows
and spare bytes are pre-filled with 0x5A.  Direct shapes (k in {64, 128, 256})
run the row-masked encode, the others the encode into scratch and the copy of
the absent rows."""
import numpy as np
import pytest

import novelpoly_amd as npa

pytestmark = pytest.mark.gpu

FILL = 0x5A
SL = 2 * 300  # one full 256-column tile plus a partial one

# (n_wanted, k_wanted, shard_len)
DIRECT = [(256, 86, SL), (512, 128, SL), (1024, 342, SL),  # n = 4k
          (600, 256, SL),     # n1024 k256, wanted_n inside segment 2
          (512, 256, SL),     # n = 2k
          (512, 64, SL), (2048, 256, SL),  # n = 8k: the runtime shift loop
          (700, 234, SL)]     # n1024 k128, partial segment 5
# k <= 32 (small, generic), k = 1024 (resident), k = 512, k = 2048 (big), k = 4096 (huge)
FALLBACK = [(60, 20, SL), (16, 8, SL), (1024, 20, SL), (4096, 1366, 2 * 260), (1024, 512, SL),
            (7000, 2334, 2 * 260), (16384, 5462, 2 * 70)]
LARGE = {(4096, 1366), (7000, 2334), (16384, 5462)}  # patterns 1, 2, 6, 7 only


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _codeword(oracle, rng, n, k, wn, sl):
    plen = (sl // 2) * 2 * k - 3
    st, shards = oracle.encode(rng.integers(0, 256, plen, dtype=np.uint8).tobytes(), n, k, wn)
    assert st == 0 and len(shards[0]) == sl
    rows = np.full((n, sl), FILL, np.uint8)
    rows[:wn] = np.stack([np.frombuffer(s, np.uint8) for s in shards])
    return rows


def _patterns(oracle, rng, n, k, wn, sl, large):
    """[(name, rows n x sl, present n)] -- rows >= wanted_n are never present."""
    def rand_rows():
        return rng.integers(0, 256, (n, sl), dtype=np.uint8)

    def pres_without(absent):
        p = np.zeros(n, np.uint8)
        p[:wn] = 1
        p[np.asarray(absent, dtype=np.int64)] = 0
        return p

    def segment(q):  # rows of segment q below wanted_n, half of them (at least one) absent
        rows = np.arange(q * k, min((q + 1) * k, wn))
        return rng.choice(rows, max(1, len(rows) // 2), replace=False) if len(rows) else rows

    out = []
    # 1: random bytes, min((n - k) / 2, wanted_n - k) random rows below wanted_n absent
    out.append(("random", rand_rows(), pres_without(rng.choice(wn, min((n - k) // 2, wn - k), replace=False))))
    # 2: a codeword with only row wanted_n - 1 absent
    out.append(("last-row", _codeword(oracle, rng, n, k, wn, sl), pres_without([wn - 1])))
    if not large:
        # 3: codewords with absences confined to segments
        segs = {4: [[3], [2], [1, 3]], 8: [[5], [4, 7]]}.get(n // k, [])
        for qs in segs:
            absent = np.concatenate([segment(q) for q in qs]).astype(np.int64)
            out.append(("segments-" + "+".join(map(str, qs)), _codeword(oracle, rng, n, k, wn, sl), pres_without(absent)))
        out.append(("systematic-few", _codeword(oracle, rng, n, k, wn, sl),
                    pres_without(rng.choice(k, min(3, k), replace=False))))
        # 4: all systematic rows present, the other present rows random, half of the parity rows absent
        rows = _codeword(oracle, rng, n, k, wn, sl)
        rows[k:] = rng.integers(0, 256, (n - k, sl), dtype=np.uint8)
        out.append(("copy-mode", rows, pres_without(k + rng.choice(wn - k, max(1, (wn - k) // 2), replace=False))))
        # 5: exactly k rows present
        out.append(("exactly-k", rand_rows(), pres_without(rng.choice(wn, wn - k, replace=False))))
    # 6: k - 1 rows present: NeedMoreShards, untouched
    out.append(("k-1", rand_rows(), pres_without(rng.choice(wn, wn - k + 1, replace=False))))
    # 7: no absent row below wanted_n: nothing is written
    out.append(("none-absent", rand_rows(), pres_without([])))
    return out


def _expected_rows(oracle, rows, pres, n, k, wn, sl):
    """{v: bytes} for the absent rows below wanted_n, or None for NeedMoreShards."""
    recv = [rows[v].tobytes() if pres[v] else None for v in range(n)]
    st, pay = oracle.reconstruct(recv, n, k)
    if st:
        assert st == npa.NeedMoreShards.code
        return None
    absent = [v for v in range(wn) if not pres[v]]
    if not absent:
        return {}
    assert len(pay) == (sl // 2) * 2 * k
    st, enc = oracle.encode(pay, n, k, wn)
    assert st == 0 and len(enc[0]) == sl
    return {v: enc[v] for v in absent}


def expected_rows(oracle, p, sl, pats):
    """_expected_rows of every payload of `pats` [(name, rows n x sl, present n)]."""
    return [_expected_rows(oracle, rows, pr, p.n(), p.k(), p.wanted_n, sl) for _, rows, pr in pats]


def run_restore(gpu, oracle, p, sl, pats, offset=0, slack=64, expected=None):
    """One batch of `pats` [(name, rows n x sl, present n)] under `p` (d_shards
    `offset` bytes into its allocation, batch_stride = n * sl + slack), with and
    without d_status: every byte of the buffer against the oracle's
    (`expected`: expected_rows(pats) when the caller shares it between runs)."""
    import torch

    n, k, wn = p.n(), p.k(), p.wanted_n
    batch, stride = len(pats), n * sl + slack
    before = np.full(offset + batch * stride + 64, FILL, np.uint8)
    pres = np.stack([pr for _, _, pr in pats])
    for b, (name, rows, pr) in enumerate(pats):
        view = before[offset + b * stride: offset + b * stride + n * sl].reshape(n, sl)
        view[pr != 0] = rows[pr != 0]
    want = before.copy()  # every byte but the restored rows stays as it was
    status = []
    if expected is None:
        expected = expected_rows(oracle, p, sl, pats)
    for b, (name, rows, pr) in enumerate(pats):
        exp = expected[b]
        status.append((npa.NeedMoreShards.code if exp is None else 0, int(pr.sum())))
        view = want[offset + b * stride: offset + b * stride + n * sl].reshape(n, sl)
        for v, data in (exp or {}).items():
            view[v] = np.frombuffer(data, np.uint8)
    dpres = _dev(pres)
    s = torch.cuda.current_stream().cuda_stream
    for with_status in (True, False):
        buf = _dev(before)
        st_d = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
        npa.restore_shards_batch_dev(p, buf.data_ptr() + offset, sl, stride, dpres.data_ptr(), batch, ctx=gpu, stream=s,
                                     d_status=st_d.data_ptr() if with_status else 0)
        got = _host(buf)
        wrong = []  # every payload that differs, the first in detail
        for b, (name, _, pr) in enumerate(pats):
            lo, hi = offset + b * stride, offset + (b + 1) * stride
            if not np.array_equal(got[lo:hi], want[lo:hi]):
                bad = np.flatnonzero(got[lo:hi] != want[lo:hi])
                rows_bad = sorted(set((bad // sl).tolist()))[:8]
                wrong.append(f"payload {b} ({name}), status buffer {with_status}: {bad.size} bytes differ, "
                             f"rows {rows_bad} (absent: {[v for v in rows_bad if v < n and not pr[v]]})")
        if wrong:
            raise AssertionError(wrong[0] + f"; {len(wrong)} payloads differ: " + ", ".join(w.split(",")[0] for w in wrong))
        assert np.array_equal(got[:offset], want[:offset]) and np.array_equal(got[-64:], want[-64:])
        if with_status:
            stat = _host(st_d)
            assert [tuple(int(x) for x in r) for r in stat] == status
            errs = npa.payload_errors(p, stat)
            for b, (code, have) in enumerate(status):
                assert errs[b] == (npa.NeedMoreShards(have, k, n) if code else None), b


def _run_shape(gpu, oracle, nw, kw, sl, offset=0, slack=64):
    p = npa.CodeParams.derive_parameters(nw, kw)
    rng = np.random.default_rng(1000 * nw + kw + sl + offset)
    pats = _patterns(oracle, rng, p.n(), p.k(), p.wanted_n, sl, (nw, kw) in LARGE)
    run_restore(gpu, oracle, p, sl, pats, offset, slack)


@pytest.mark.parametrize("nw,kw,sl", DIRECT)
def test_restore_direct(gpu, oracle, nw, kw, sl):
    _run_shape(gpu, oracle, nw, kw, sl)


def test_restore_direct_unaligned_rows(gpu, oracle):
    """Rows at even but not 4-byte-aligned addresses: odd chunk count, d_shards
    2 bytes into the allocation, batch_stride = n * shard_len + 2."""
    _run_shape(gpu, oracle, 1024, 342, 2 * 257, offset=2, slack=2)


@pytest.mark.parametrize("nw,kw,sl", FALLBACK)
def test_restore_fallback(gpu, oracle, nw, kw, sl):
    _run_shape(gpu, oracle, nw, kw, sl)


@pytest.mark.parametrize("nw,kw", [(1024, 342), (60, 20)])
def test_restore_host_single(gpu, oracle, nw, kw):
    """ReedSolomon.restore_shards on random bytes with odd-length shards (zero
    padded like WrappedShard), and its NeedMoreShards with the reference's fields."""
    p = npa.CodeParams.derive_parameters(nw, kw)
    n, k, wn = p.n(), p.k(), p.wanted_n
    rng = np.random.default_rng(nw + kw)
    odd = SL - 1
    pres = np.ones(wn, bool)
    pres[rng.choice(wn, min((n - k) // 2, wn - k), replace=False)] = False
    recv = [rng.integers(0, 256, odd, dtype=np.uint8).tobytes() if pres[v] else None for v in range(wn)]
    padded = [None if s is None else s + b"\x00" for s in recv] + [None] * (n - wn)
    st, pay = oracle.reconstruct(padded, n, k)
    assert st == 0
    st, enc = oracle.encode(pay, n, k, wn)
    assert st == 0
    want = [padded[v] if pres[v] else enc[v] for v in range(wn)]
    rs = p.make_encoder(gpu)
    got = rs.restore_shards(recv)
    assert len(got) == wn and got == want
    if kw == npa.recoverablity_subset_size(nw):
        assert npa.restore_shards(recv, nw, ctx=gpu) == want
    short = list(recv)
    for v in np.flatnonzero(pres)[k - 1:]:
        short[v] = None
    with pytest.raises(npa.NeedMoreShards) as ei:
        rs.restore_shards(short)
    assert ei.value == npa.NeedMoreShards(k - 1, k, n)


def test_restore_slices(gpu):
    """1100 payloads of 1 MiB at n256 k64: 1.07 GiB of decoded payloads, more
    than the context's payload scratch, so the call runs in two uneven slices.
    Generated, blanked and compared on the device."""
    import torch

    p = npa.CodeParams.derive_parameters(256, 86)
    n, k, batch, plen = p.n(), p.k(), 1100, 1 << 20
    sl = p.make_encoder(gpu).shard_len(plen)
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    pay = torch.randint(0, 256, (batch, plen), dtype=torch.uint8, device="cuda", generator=gen)
    ref = torch.empty((batch, n, sl), dtype=torch.uint8, device="cuda")
    npa.encode_batch_dev(p, pay.data_ptr(), plen, plen, batch, ref.data_ptr(), n * sl, ctx=gpu, stream=s)
    del pay
    order = torch.rand((batch, n), device="cuda", generator=gen).argsort(dim=1)
    pres = torch.ones((batch, n), dtype=torch.uint8, device="cuda")
    pres.scatter_(1, order[:, : (n - k) // 2], 0)
    work = ref.clone()
    work[pres == 0] = FILL
    st_d = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
    npa.restore_shards_batch_dev(p, work.data_ptr(), sl, n * sl, pres.data_ptr(), batch, ctx=gpu, stream=s,
                                 d_status=st_d.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(work, ref)
    assert bool((st_d[:, 0] == 0).all()) and bool((st_d[:, 1] == n - (n - k) // 2).all())

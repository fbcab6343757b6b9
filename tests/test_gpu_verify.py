"""np_verify_shards_batch_dev / np_rs_verify_shards: a present row below
wanted_n mismatches when it differs from its row of the reference's
ReedSolomon::encode(ReedSolomon::reconstruct(received)) (mod.rs:117-157 after
mod.rs:162-239).  The per-payload counts and the optional flag map equal the
oracle's for any received bytes, the shard buffer is only read, and nothing
around the results is written.

Each shape is one batch whose payloads carry the patterns of `_patterns`; the
oracle's answer is computed once per shape and shared by the variants (with and
without d_status, with and without d_mismatch, d_shards at offsets 0 and 2 of
its allocation).  Direct shapes (k in {64, 128, 256}) run the verify encode,
the others the encode into scratch and the compare of the present rows."""
import functools

import numpy as np
import pytest

import novelpoly_amd as npa

pytestmark = pytest.mark.gpu

FILL = 0x5A
GUARD = 0xA5
SL = 2 * 300  # one full 256-column tile plus a partial one
UNDECODABLE = 0xFFFFFFFF

# (n_wanted, k_wanted, shard_len)
DIRECT = [(256, 86, SL), (512, 128, SL), (1024, 342, SL),  # n = 4k
          (600, 256, SL),     # n1024 k256, wanted_n inside segment 2
          (512, 256, SL),     # n = 2k
          (512, 64, SL), (2048, 256, SL),  # n = 8k: the runtime shift loop
          (700, 234, SL)]     # n1024 k128, partial segment 5
# k <= 32 (small, generic), k = 512, k = 1024 (resident), k = 2048 (big), k = 4096 (huge)
FALLBACK = [(60, 20, SL), (16, 8, SL), (1024, 20, SL), (1024, 512, SL), (4096, 1366, 2 * 260),
            (7000, 2334, 2 * 260), (16384, 5462, 2 * 70)]
LARGE = {(4096, 1366), (7000, 2334), (16384, 5462)}  # patterns 1, 2, 3, 10, 11 only


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


def _flip(rows, v, sym, rng):
    """One bit of symbol `sym` of row v."""
    rows[v, 2 * sym + int(rng.integers(0, 2))] ^= np.uint8(1 << int(rng.integers(0, 8)))


def _patterns(oracle, rng, n, k, wn, sl, large):
    """[(name, rows n x sl, present n, exact)] -- rows >= wanted_n are never
    present; exact: the mismatching rows when the pattern fixes them, else None."""
    syms = sl // 2

    def rand_rows():
        return rng.integers(0, 256, (n, sl), dtype=np.uint8)

    def pres_without(absent):
        p = np.zeros(n, np.uint8)
        p[:wn] = 1
        p[np.asarray(absent, dtype=np.int64)] = 0
        return p

    def parity(p):  # present parity rows
        return np.flatnonzero(p[k:wn]) + k

    out = []
    code = _codeword(oracle, rng, n, k, wn, sl)
    pres1 = pres_without(rng.choice(wn, min((n - k) // 2, wn - k - 1), replace=False))
    # 1: a codeword, min((n - k) / 2, wanted_n - k - 1) random rows absent
    out.append(("codeword", code, pres1, []))
    # 2: one bit of the last symbol (a partial-tile column) of a present parity row
    rows = code.copy()
    _flip(rows, int(rng.choice(parity(pres1))), syms - 1, rng)
    out.append(("last-symbol", rows, pres1, None))
    # 3: one bit of symbol 0 of the first present parity row
    rows = code.copy()
    _flip(rows, int(parity(pres1)[0]), 0, rng)
    out.append(("first-symbol", rows, pres1, None))
    if not large:
        # 4: symbols 255 and 256 (the tile boundary) of two different present parity rows
        rows = code.copy()
        two = rng.choice(parity(pres1), 2, replace=False)
        _flip(rows, int(two[0]), 255, rng)
        _flip(rows, int(two[1]), 256, rng)
        out.append(("tile-boundary", rows, pres1, None))
        # 5: copy mode -- every systematic row, half of the parity rows, two of them altered
        rows = code.copy()
        pres = pres_without(k + rng.choice(wn - k, (wn - k) // 2, replace=False))
        two = rng.choice(parity(pres), 2, replace=False)
        _flip(rows, int(two[0]), int(rng.integers(0, syms)), rng)
        _flip(rows, int(two[1]), int(rng.integers(0, syms)), rng)
        out.append(("copy-mode", rows, pres, sorted(int(v) for v in two)))
        # 6: a present systematic row altered while other systematic rows are absent
        rows = code.copy()
        gone = rng.choice(k, min(3, k - 1), replace=False)
        pres = pres_without(gone)
        _flip(rows, int(rng.choice(np.setdiff1d(np.arange(k), gone))), int(rng.integers(0, syms)), rng)
        out.append(("systematic-flip", rows, pres, None))
        # 7: present parity rows confined to single segments, one row of each altered
        for qs in {4: [[3], [1, 3]], 8: [[5], [4, 7]]}.get(n // k, []):
            rows = code.copy()
            pres = np.zeros(n, np.uint8)
            pres[:k] = 1
            hit = []
            for q in qs:
                seg = np.arange(q * k, min((q + 1) * k, wn))
                pres[seg] = 1
                if len(seg):
                    hit.append(int(rng.choice(seg)))
                    _flip(rows, hit[-1], int(rng.integers(0, syms)), rng)
            out.append(("segments-" + "+".join(map(str, qs)), rows, pres, sorted(hit)))
        # 8: random bytes, exactly k rows present: always consistent
        out.append(("random-exactly-k", rand_rows(), pres_without(rng.choice(wn, wn - k, replace=False)), []))
        # 9: random bytes, more than k rows present
        out.append(("random", rand_rows(), pres1, None))
    # 10: k - 1 rows present: NeedMoreShards
    out.append(("k-1", rand_rows(), pres_without(rng.choice(wn, wn - k + 1, replace=False)), None))
    # 11: every row of a codeword
    out.append(("all-present", code, pres_without([]), []))
    return out


def _expected_flags(oracle, rows, pres, n, k, wn, sl):
    """n flags (1: row v < wanted_n is present and differs from the
    re-encoding), or None for NeedMoreShards."""
    recv = [rows[v].tobytes() if pres[v] else None for v in range(n)]
    st, pay = oracle.reconstruct(recv, n, k)
    if st:
        assert st == npa.NeedMoreShards.code
        return None
    assert len(pay) == (sl // 2) * 2 * k
    st, enc = oracle.encode(pay, n, k, wn)
    assert st == 0 and len(enc) == wn and all(len(e) == sl for e in enc[:1])
    flags = np.zeros(n, np.uint8)
    for v in range(wn):
        if pres[v] and enc[v] != recv[v]:
            flags[v] = 1
    return flags


def expected_case(oracle, p, sl, pats):
    """The oracle's answer for the batch `pats` [(name, rows n x sl, present n,
    exact)] under `p`: (flags batch x n, counts, [(status, have)]), read only.
    `exact` is the list of mismatching rows where the pattern fixes it, else None."""
    n, k, wn = p.n(), p.k(), p.wanted_n
    flags = np.zeros((len(pats), n), np.uint8)
    counts, status = [], []
    for b, (name, rows, pr, exact) in enumerate(pats):
        exp = _expected_flags(oracle, rows, pr, n, k, wn, sl)
        if exp is None:
            assert exact is None, name
            counts.append(UNDECODABLE)
            status.append((npa.NeedMoreShards.code, int(pr.sum())))
            continue
        if exact is not None:  # the patterns whose answer the semantics fix
            assert np.flatnonzero(exp).tolist() == exact, (name, np.flatnonzero(exp).tolist(), exact)
        assert not exp[:k].any(), name  # systematic rows never mismatch
        flags[b] = exp
        counts.append(int(exp.sum()))
        status.append((0, int(pr.sum())))
    flags.setflags(write=False)
    return flags, np.asarray(counts, np.uint32), status


@functools.lru_cache(maxsize=None)
def _shape_case(oracle, nw, kw, sl):
    """The shape's batch and the oracle's answer, computed once (read only)."""
    p = npa.CodeParams.derive_parameters(nw, kw)
    n, k, wn = p.n(), p.k(), p.wanted_n
    rng = np.random.default_rng(1000 * nw + kw + sl)
    pats = _patterns(oracle, rng, n, k, wn, sl, (nw, kw) in LARGE)
    flags, counts, status = expected_case(oracle, p, sl, pats)
    for b, (name, _, _, exact) in enumerate(pats):
        assert (counts[b] == UNDECODABLE) == (name == "k-1"), name
        if name != "k-1" and exact is None and name != "random":
            assert flags[b].any(), name  # an altered symbol with > k rows present shows
    return p, pats, flags, counts, status


# (offset of d_shards in its allocation, batch_stride - n * shard_len, d_status given, d_mismatch given);
# offset 2, stride n * sl + 2: rows at any even address
ALL_VARIANTS = tuple((offset, slack, st, mp) for offset, slack in ((0, 64), (2, 2)) for st in (True, False)
                     for mp in (True, False))
SWEEP_VARIANTS = ((0, 64, True, True), (2, 2, False, False))


def run_verify(gpu, p, sl, pats, expected, variants=ALL_VARIANTS, label=""):
    """One batch of `pats` under `p` against `expected` (expected_case), once
    per variant: counts, map, statuses, the guards around them, and d_shards
    unchanged."""
    import torch

    want_flags, want_counts, status = expected
    n, k = p.n(), p.k()
    batch = len(pats)
    pres = np.stack([pr for _, _, pr, _ in pats])
    dpres = _dev(pres)
    s = torch.cuda.current_stream().cuda_stream
    staged = (None, None, None)  # one staging of the batch per (offset, slack)
    for offset, slack, with_status, with_map in variants:
        stride = n * sl + slack
        if staged[0] != (offset, slack):
            before = np.full(offset + batch * stride + 64, FILL, np.uint8)
            for b, (name, rows, pr, _) in enumerate(pats):
                view = before[offset + b * stride: offset + b * stride + n * sl].reshape(n, sl)
                view[pr != 0] = rows[pr != 0]
            staged = ((offset, slack), before, _dev(before))
        _, before, buf = staged
        tag = f"offset {offset}, status {with_status}, map {with_map}"
        st_d = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
        cnt_d = torch.full((64 + 4 * batch + 64,), GUARD, dtype=torch.uint8, device="cuda")
        map_d = torch.full((64 + batch * n + 64,), GUARD, dtype=torch.uint8, device="cuda")
        npa.verify_shards_batch_dev(p, buf.data_ptr() + offset, sl, stride, dpres.data_ptr(), batch,
                                    cnt_d.data_ptr() + 64, ctx=gpu, stream=s,
                                    d_mismatch=map_d.data_ptr() + 64 if with_map else 0,
                                    d_status=st_d.data_ptr() if with_status else 0)
        cnt, mp = _host(cnt_d), _host(map_d)
        assert (cnt[:64] == GUARD).all() and (cnt[-64:] == GUARD).all(), tag
        got_counts = cnt[64:-64].copy().view(np.uint32)
        print(f"{label} {tag}: counts {got_counts.tolist()} want {want_counts.tolist()}")
        wrong = [(int(b), pats[b][0]) for b in np.flatnonzero(got_counts != want_counts)]
        assert got_counts.tolist() == want_counts.tolist(), (tag, "payloads whose count differs", wrong)
        if with_map:
            assert (mp[:64] == GUARD).all() and (mp[-64:] == GUARD).all(), tag
            got = mp[64:-64].reshape(batch, n)
            for b, (name, _, _, _) in enumerate(pats):
                assert np.array_equal(got[b], want_flags[b]), \
                    (tag, b, name, np.flatnonzero(got[b]).tolist()[:8], np.flatnonzero(want_flags[b]).tolist()[:8])
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
        assert np.array_equal(_host(buf), before), tag  # d_shards is only read


def _run_shape(gpu, oracle, nw, kw, sl):
    p, pats, flags, counts, status = _shape_case(oracle, nw, kw, sl)
    run_verify(gpu, p, sl, pats, (flags, counts, status), label=f"{nw},{kw}")


@pytest.mark.parametrize("nw,kw,sl", DIRECT)
def test_verify_direct(gpu, oracle, nw, kw, sl):
    _run_shape(gpu, oracle, nw, kw, sl)


@pytest.mark.parametrize("nw,kw,sl", [(1024, 342, 2 * 257), (512, 64, 2 * 259)])
def test_verify_direct_column_tail(gpu, oracle, nw, kw, sl):
    """A second tile of 1 and of 3 columns: the per-column path of the compare,
    where a lane holds fewer than its four columns (300 columns leave whole
    lanes only).  With offset 2 the rows are at 2-mod-4 addresses."""
    _run_shape(gpu, oracle, nw, kw, sl)


@pytest.mark.parametrize("nw,kw,sl", FALLBACK)
def test_verify_fallback(gpu, oracle, nw, kw, sl):
    _run_shape(gpu, oracle, nw, kw, sl)


@pytest.mark.parametrize("nw,kw", [(1024, 342), (60, 20)])
def test_verify_host_single(gpu, oracle, nw, kw):
    """ReedSolomon.verify / mismatched_shards on odd-length shards (zero padded
    like WrappedShard and compared over the padded row), and NeedMoreShards
    raised with the reference's fields."""
    p = npa.CodeParams.derive_parameters(nw, kw)
    n, k, wn = p.n(), p.k(), p.wanted_n
    rng = np.random.default_rng(nw + kw)
    odd = SL - 1

    def mismatching(received):  # the oracle's answer over the zero-padded rows
        padded = [None if s is None else s + b"\x00" * (len(s) & 1) for s in received] + [None] * (n - wn)
        st, pay = oracle.reconstruct(padded, n, k)
        assert st == 0
        st, enc = oracle.encode(pay, n, k, wn)
        assert st == 0
        return [i for i in range(wn) if padded[i] is not None and padded[i] != enc[i]]

    st, shards = oracle.encode(rng.integers(0, 256, (SL // 2) * 2 * k - 3, dtype=np.uint8).tobytes(), n, k, wn)
    assert st == 0 and len(shards[0]) == SL
    pres = np.ones(wn, bool)
    pres[rng.choice(wn, min((n - k) // 2, wn - k - 1), replace=False)] = False
    recv = [shards[v] if pres[v] else None for v in range(wn)]
    rs = p.make_encoder(gpu)
    # a codeword, then one bit of its last byte (in the partial tile) altered
    assert rs.verify(recv) is True and rs.mismatched_shards(recv) == []
    bad = list(recv)
    v = int(np.flatnonzero(pres[k:])[0]) + k
    row = bytearray(bad[v])
    row[SL - 1] ^= 0x10
    bad[v] = bytes(row)
    want = mismatching(bad)
    assert want
    assert rs.verify(bad) is False and rs.mismatched_shards(bad) == want
    if kw == npa.recoverablity_subset_size(nw):
        assert npa.verify(recv, nw, ctx=gpu) is True and npa.verify(bad, nw, ctx=gpu) is False
    # odd lengths: random bytes with more than k shards, and with exactly k (always consistent)
    rnd = [rng.integers(0, 256, odd, dtype=np.uint8).tobytes() if pres[i] else None for i in range(wn)]
    want = mismatching(rnd)
    assert want and all(i >= k for i in want)
    assert rs.verify(rnd) is False and rs.mismatched_shards(rnd) == want
    only_k = list(rnd)
    for i in np.flatnonzero(pres)[k:]:
        only_k[i] = None
    assert mismatching(only_k) == []
    assert rs.verify(only_k) is True and rs.mismatched_shards(only_k) == []
    short = list(recv)
    for i in np.flatnonzero(pres)[k - 1:]:
        short[i] = None
    for call in (rs.verify, rs.mismatched_shards):
        with pytest.raises(npa.NeedMoreShards) as ei:
            call(short)
        assert ei.value == npa.NeedMoreShards(k - 1, k, n)


def slice_len(scratch):
    """Payloads per slice of a uniform restore / verify / recover call that keeps
    `scratch` bytes per payload in context scratch (masked_shape in engine.cpp):
    an eighth of the context's scratch cap, which is a 32nd of the device's
    memory within 2 .. 8 GiB, in multiples of 8 payloads.  1 GiB of an MI355X."""
    import torch

    cap = min(8 << 30, max(2 << 30, torch.cuda.get_device_properties(0).total_memory // 32)) // 8
    per = cap // scratch
    return per & ~7 if per >= 8 else max(1, per)


class SlicesCase:
    """A batch too large for one scratch slice, generated, blanked and compared
    on the device (no oracle: the truth is the encode of the payloads).  `work`
    is encode(pay) with the absent rows set to FILL, `want` what a restore
    leaves.  Three payload classes, each in every slice:
      A (even b): every systematic row present, (n - k) / 2 parity rows absent,
        one byte altered in one present parity row: exactly that row mismatches;
      B (odd b): (n - k) / 2 absences anywhere, nothing altered: no mismatch;
      C (b = 96 mod 97, and the last b): k - 1 present rows: NeedMoreShards,
        nothing touched.
    `scratch` is what the call keeps in context scratch per payload, in bytes:
    the decoded payload (verify, and restore or recover without d_out), or the
    n shard rows where the row-masked encodes do not serve (n, k).  The case
    asserts that the batch is then more than one slice on this device, and that
    every slice holds all three classes."""

    def __init__(self, gpu, nw, kw, batch, scratch, plen=1 << 20):
        import torch

        p = npa.CodeParams.derive_parameters(nw, kw)
        n, k = p.n(), p.k()
        sl = p.make_encoder(gpu).shard_len(plen)
        assert (sl // 2) * 2 * k == plen and p.wanted_n == n
        s = torch.cuda.current_stream().cuda_stream
        gen = torch.Generator(device="cuda").manual_seed(7 + n + k)
        self.p, self.n, self.k, self.sl, self.batch, self.plen = p, n, k, sl, batch, plen
        self.pay = torch.randint(0, 256, (batch, plen), dtype=torch.uint8, device="cuda", generator=gen)
        want = torch.empty((batch, n, sl), dtype=torch.uint8, device="cuda")
        npa.encode_batch_dev(p, self.pay.data_ptr(), plen, plen, batch, want.data_ptr(), n * sl, ctx=gpu, stream=s)
        b = torch.arange(batch, device="cuda")
        self.c = (b % 97 == 96) | (b == batch - 1)
        self.a = (b % 2 == 0) & ~self.c
        gone = (n - k) // 2
        rnd = torch.rand((batch, n), device="cuda", generator=gen)
        rnd[:, :k] += 2.0 * self.a[:, None]  # A: the parity rows come first in the order
        order = rnd.argsort(dim=1)
        ones = torch.ones((batch, n), dtype=torch.uint8, device="cuda")
        self.pres = torch.where(self.c[:, None], ones.scatter(1, order[:, : n - k + 1], 0),
                                ones.scatter(1, order[:, :gone], 0))
        ia = self.a.nonzero().squeeze(1)
        hit = order[ia, gone]  # A: the first parity row that stays present
        col = torch.randint(0, sl, (ia.numel(),), device="cuda", generator=gen)
        want[ia, hit, col] ^= 0x40
        self.flags = torch.zeros((batch, n), dtype=torch.uint8, device="cuda")
        self.flags[ia, hit] = 1
        self.counts = torch.where(self.c, -1, self.a.to(torch.int32)).to(torch.int32)  # -1: UINT32_MAX
        self.status = torch.stack([torch.where(self.c, npa.NeedMoreShards.code, 0),
                                   torch.where(self.c, k - 1, n - gone)], dim=1).to(torch.int32)
        self.work = want.clone()
        self.blank()
        want[self.c] = self.work[self.c]
        self.want = want
        torch.cuda.synchronize()
        assert bool((hit >= k).all()) and bool((self.pres[ia, hit] == 1).all())
        assert bool((self.pres.sum(dim=1) == self.status[:, 1]).all())
        self.per = slice_len(scratch)
        assert self.per < batch, f"one slice of {self.per} payloads takes the whole batch of {batch}"
        for b0 in range(0, batch, self.per):
            for name, cls in (("A", self.a), ("B", ~self.a & ~self.c), ("C", self.c)):
                assert bool(cls[b0 : b0 + self.per].any()), f"no payload of class {name} in the slice at {b0}"

    def blank(self):
        """Absent rows back to FILL: `work` as it was before a restore."""
        self.work[self.pres == 0] = FILL


def test_verify_slices(gpu):
    """1100 payloads of 1 MiB at n256 k64 (two uneven slices of the payload
    scratch on an MI355X, as test_restore_slices): counts, the map at
    d_mismatch + b0 * n or the call's own per slice, and the statuses.
    SlicesCase asserts that the batch is sliced and every class in every slice."""
    import torch

    c = SlicesCase(gpu, 256, 86, 1100, scratch=1 << 20)
    s = torch.cuda.current_stream().cuda_stream
    before = c.work.clone()
    for with_map in (True, False):
        cnt = torch.full((c.batch,), 7, dtype=torch.int32, device="cuda")
        mp = torch.full((c.batch, c.n), GUARD, dtype=torch.uint8, device="cuda")
        st = torch.full((c.batch, 2), -1, dtype=torch.int32, device="cuda")
        npa.verify_shards_batch_dev(c.p, c.work.data_ptr(), c.sl, c.n * c.sl, c.pres.data_ptr(), c.batch,
                                    cnt.data_ptr(), ctx=gpu, stream=s, d_mismatch=mp.data_ptr() if with_map else 0,
                                    d_status=st.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(cnt, c.counts), (with_map, (cnt != c.counts).nonzero()[:8].tolist())
        assert torch.equal(mp, c.flags) if with_map else bool((mp == GUARD).all()), with_map
        assert torch.equal(st, c.status) and torch.equal(c.work, before), with_map

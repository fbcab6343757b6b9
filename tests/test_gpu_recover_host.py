"""np_recover_batch_host and the multi-device recover calls: the payload, the
absent rows and the verdict of a HOST-memory batch from one decode per payload,
pipelined over the context's slots.  Each requested output equals, byte for
byte, the oracle's ReedSolomon::reconstruct and ReedSolomon::encode(
reconstruct(..)) (mod.rs:162-239, mod.rs:117-157) for any received bytes --
what np_recover_batch_dev gives (tests/test_gpu_recover.py, whose patterns and
expectations these tests share).

Every host buffer sits inside odd-sized canary guards and is compared WHOLE,
guards included: `shards` against the received bytes with the oracle's rows in
the absent places below wanted_n of the payloads that decode (0x5C garbage in
every other absent place, unchanged); `out`, `bad_rows`, `mismatch` and
`status` against their fills wherever they must not be written.  The batch is
the nine patterns of test_gpu_recover._patterns with the k - 1 payload in the
middle."""
import functools

import numpy as np
import pytest

import novelpoly_amd as npa
from test_gpu_host_guard import CANARY, GUARD
from test_gpu_recover import COMBOS, _patterns, expected_recover

pytestmark = pytest.mark.gpu

GARBAGE = 0x5C  # absent rows, rows >= wanted_n, the gap up to batch_stride
FILLS = dict(out=0x11, bad=0x22, map=0x33, status=0x44)
SL = 2 * 300
ALL = (True, True, True)
RESTORE = (False, True, False)


def _guarded(nbytes, fill, pinned=False):
    """(base, view): nbytes inside GUARD canary bytes on each side; GUARD is odd,
    so the view starts at an odd byte offset into its allocation (numpy's, or a
    pinned one of torch's)."""
    total = nbytes + 2 * GUARD
    if pinned:
        import torch

        base = torch.empty(total, dtype=torch.uint8, pin_memory=True).numpy()
        base[...] = CANARY
    else:
        base = np.full(total, CANARY, np.uint8)
    view = base[GUARD:GUARD + nbytes]
    view[...] = fill
    return base, view


@functools.lru_cache(maxsize=None)
def _case(oracle, nw, kw, sl):
    """The shape's batch -- the k - 1 payload mid-batch -- and the oracle's
    answers, computed once (read only)."""
    d = npa.CodeParams.derive_parameters(nw, kw)
    p = npa.CodeParams(d.n(), d.k(), d.wanted_n)
    rng = np.random.default_rng(7000 * nw + 10 * kw + sl)
    pats = _patterns(oracle, rng, p.n(), p.k(), p.wanted_n, sl)
    assert len(pats) == 9
    short = [i for i, (name, _, _) in enumerate(pats) if name == "k-1"]
    assert len(short) == 1
    pats.insert(4, pats.pop(short[0]))
    exp = expected_recover(oracle, p, sl, pats)
    assert [b for b, pay in enumerate(exp[2]) if pay is None] == [4]
    assert any(exp[0][b] for b in range(9) if b != 4) and exp[1][1][0] > 0  # rows to restore, rows that mismatch
    return p, pats, exp


def _subset(case, keep):
    """The payloads `keep` of a case, with their expectations."""
    p, pats, (rows, (flags, counts, status), pays) = case
    return p, [pats[b] for b in keep], ([rows[b] for b in keep], (flags[keep], counts[keep], [status[b] for b in keep]),
                                        [pays[b] for b in keep])


class HostBatch:
    """The guarded host buffers of one call on `pats`, and what each must hold
    afterwards for a request (with_out, restore, verify)."""

    def __init__(self, p, sl, pats, slack=0, out_slack=0, pinned=False):
        self.p, self.sl, self.pats = p, sl, pats
        n, k = p.n(), p.k()
        self.batch, self.stride = len(pats), n * sl + slack
        self.pay_len = (sl // 2) * 2 * k
        self.ostride = self.pay_len + out_slack
        self.sh_b, self.sh = _guarded(self.batch * self.stride, GARBAGE, pinned)
        for b, (_, rows, pr) in enumerate(pats):
            view = self.sh[b * self.stride: b * self.stride + n * sl].reshape(n, sl)
            view[pr != 0] = rows[pr != 0]
        self.received = self.sh_b.copy()
        self.pres_b, self.pres = _guarded(self.batch * n, 0, pinned)
        self.pres[...] = np.stack([pr for _, _, pr in pats]).reshape(-1)
        self.pres_before = self.pres_b.copy()
        self.out_b, self.out = _guarded(self.batch * self.ostride, FILLS["out"], pinned)
        self.bad_b, self.bad = _guarded(4 * self.batch, FILLS["bad"], pinned)
        self.map_b, self.map = _guarded(self.batch * n, FILLS["map"], pinned)
        self.st_b, self.st = _guarded(8 * self.batch, FILLS["status"], pinned)
        self.untouched = {name: getattr(self, name + "_b").copy() for name in ("sh", "out", "bad", "map", "st")}

    def kwargs(self, combo, with_status=True, with_map=None):
        with_out, restore, verify = combo
        with_map = verify if with_map is None else with_map
        return dict(out=self.out.ctypes.data if with_out else 0, out_stride=self.ostride if with_out else 0,
                    restore=restore, bad_rows=self.bad.ctypes.data if verify else 0,
                    mismatch=self.map.ctypes.data if with_map else 0, status=self.st.ctypes.data if with_status else 0)

    def args(self):
        return self.p, self.sh.ctypes.data, self.sl, self.stride, self.pres.ctypes.data, self.batch

    def check(self, expected, combo, with_status=True, with_map=None, tag=""):
        with_out, restore, verify = combo
        with_map = verify if with_map is None else with_map
        exp_rows, (want_flags, want_counts, status), pays = expected
        n, sl = self.p.n(), self.sl
        assert np.array_equal(self.pres_b, self.pres_before), (tag, "present mask written")
        # the shard buffer, whole: the restored rows and nothing else
        want = self.received.copy()
        if restore:
            body = want[GUARD:GUARD + self.batch * self.stride]
            for b in range(self.batch):
                view = body[b * self.stride: b * self.stride + n * sl].reshape(n, sl)
                for v, data in (exp_rows[b] or {}).items():
                    view[v] = np.frombuffer(data, np.uint8)
        if not np.array_equal(self.sh_b, want):
            bad = np.flatnonzero(self.sh_b != want) - GUARD
            where = sorted({(int(x) // self.stride, (int(x) % self.stride) // sl) for x in bad[:4096]})[:8]
            raise AssertionError(f"{tag}: {bad.size} shard bytes differ, (payload, row) {where}")
        # the payloads, whole: fills where a payload does not decode and between the payloads
        want = self.untouched["out"].copy()
        if with_out:
            body = want[GUARD:GUARD + self.batch * self.ostride].reshape(self.batch, self.ostride)
            for b, pay in enumerate(pays):
                if pay is not None:
                    body[b, :self.pay_len] = np.frombuffer(pay, np.uint8)
        assert np.array_equal(self.out_b, want), (tag, "out", int(np.flatnonzero(self.out_b != want)[0]) - GUARD)
        want = self.untouched["bad"].copy()
        if verify:
            want[GUARD:GUARD + 4 * self.batch] = np.asarray(want_counts, np.uint32).view(np.uint8)
        assert np.array_equal(self.bad_b, want), (tag, "bad_rows", self.bad.copy().view(np.uint32).tolist())
        want = self.untouched["map"].copy()
        if with_map:
            want[GUARD:GUARD + self.batch * n] = np.asarray(want_flags).reshape(-1)
        assert np.array_equal(self.map_b, want), (tag, "mismatch")
        want = self.untouched["st"].copy()
        if with_status:
            want[GUARD:GUARD + 8 * self.batch] = np.asarray(status, np.uint32).reshape(-1).view(np.uint8)
        assert np.array_equal(self.st_b, want), (tag, "status", self.st.copy().view(np.uint32).tolist())

    def check_untouched(self, tag=""):
        assert np.array_equal(self.pres_b, self.pres_before), tag
        for name, before in self.untouched.items():
            assert np.array_equal(getattr(self, name + "_b"), before), (tag, name)


def _run(gpu, case, sl, combo, with_status=True, with_map=None, pinned=False, slack=0, out_slack=0, tag=""):
    p, pats, exp = case
    h = HostBatch(p, sl, pats, slack, out_slack, pinned)
    npa.recover_batch_host(*h.args(), ctx=gpu, **h.kwargs(combo, with_status, with_map))
    h.check(exp, combo, with_status, with_map, tag=f"{tag} {combo} pinned {pinned}")
    return h


@pytest.mark.parametrize("combo", COMBOS)
def test_every_request_combination(gpu, oracle, combo):
    case = _case(oracle, 1024, 342, SL)
    _run(gpu, case, SL, combo)
    if combo[2]:  # the counts without the map
        _run(gpu, case, SL, combo, with_map=False)


# direct n = 4k twice, wanted_n < n at n = 8k, small k, resident with rows 2 mod 4
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("nw,kw,sl", [(1024, 342, SL), (256, 86, SL), (300, 100, SL), (60, 20, SL), (4096, 1366, 42)])
def test_shapes(gpu, oracle, nw, kw, sl, pinned):
    case = _case(oracle, nw, kw, sl)
    for combo in (ALL, RESTORE):
        _run(gpu, case, sl, combo, pinned=pinned, tag=f"{nw},{kw},{sl}")


# 2 and 18: the 2-byte path; 4098: two pieces, the second 2 bytes long at 2-byte
# alignment; 8208: three pieces, all 16-byte
@pytest.mark.parametrize("sl", [2, 18, 4098, 8208])
def test_row_sizes_of_the_pack_kernel(gpu, oracle, sl):
    _run(gpu, _case(oracle, 256, 86, sl), sl, (True, True, False), tag=f"shard_len {sl}")


@pytest.mark.parametrize("env", [dict(NP_PIPE_SB="1"), dict(NP_PIPE_SB="2"), dict(NP_PIPE_SLOTS="1"),
                                 dict(NP_PIPE_SLOTS="1", NP_PIPE_SB="2")],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_pipeline_edges(gpu, oracle, monkeypatch, env):
    """Sub-batches of 1 and 2 payloads: 9 and 5 of them over 4 slots (slots
    reused, a partial last one, a sub-batch that is only the k - 1 payload), and
    one slot."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    case = _case(oracle, 256, 86, SL)
    for combo in (ALL, RESTORE):
        _run(gpu, case, SL, combo, tag=str(env))


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_strides_with_gaps(gpu, oracle, pinned):
    """batch_stride = n * shard_len + 100 and out_stride = payload length + 37:
    the gaps keep their bytes."""
    _run(gpu, _case(oracle, 256, 86, SL), SL, ALL, pinned=pinned, slack=100, out_slack=37)


def test_only_systematic_rows_cross_when_no_verdict_is_asked(gpu, oracle):
    """Every payload has its k systematic rows and no verdict is requested: the
    k systematic rows are all that is shipped, and the restored rows and the
    payloads are the same."""
    p, pats, exp = _case(oracle, 256, 86, SL)
    keep = [b for b, (_, _, pr) in enumerate(pats) if pr[:p.k()].all()]
    assert len(keep) >= 4
    sub = _subset((p, pats, exp), keep)
    for combo in ((True, True, False), RESTORE, ALL):
        _run(gpu, sub, SL, combo, tag="systematic rows present")


def test_without_status(gpu, oracle):
    """status == NULL: a batch that all decodes gives what the call with status
    gives; with the k - 1 payload the call raises NeedMoreShards(k - 1, k, n) and
    every buffer keeps its bytes."""
    case = _case(oracle, 256, 86, SL)
    p, pats, exp = case
    decodable = _subset(case, [b for b in range(9) if b != 4])
    a = _run(gpu, decodable, SL, ALL, with_status=True)
    b = _run(gpu, decodable, SL, ALL, with_status=False)
    for name in ("sh", "out", "bad", "map"):
        assert np.array_equal(getattr(a, name + "_b"), getattr(b, name + "_b")), name
    for combo in (ALL, RESTORE):
        h = HostBatch(p, SL, pats)
        with pytest.raises(npa.NeedMoreShards) as ei:
            npa.recover_batch_host(*h.args(), ctx=gpu, **h.kwargs(combo, with_status=False))
        assert ei.value == npa.NeedMoreShards(p.k() - 1, p.k(), p.n())
        h.check_untouched(str(combo))


def test_two_calls_back_to_back(gpu, oracle):
    """Different requests on one context, one after the other, in both orders:
    the second call's results are its own (the slots' staging and device buffers
    are reused)."""
    case = _case(oracle, 256, 86, SL)
    other = _case(oracle, 60, 20, SL)
    _run(gpu, case, SL, ALL)
    _run(gpu, case, SL, (False, False, True), with_map=False)
    _run(gpu, other, SL, (True, True, False))
    _run(gpu, case, SL, RESTORE, with_status=True)
    _run(gpu, case, SL, ALL)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("nw,kw,nctx", [(1024, 342, 2), (256, 86, 3)])
def test_recover_batch_multi(gpu, oracle, nw, kw, nctx):
    """Device buffers per context (several contexts on device 0, as
    tests/test_gpu_multi.py): all three requests, every payload against the
    same expectations."""
    import torch

    p, pats, (exp_rows, (want_flags, want_counts, status), pays) = _case(oracle, nw, kw, SL)
    n, k, batch = p.n(), p.k(), len(pats)
    pay_len = (SL // 2) * 2 * k
    ctxs = [npa.Context(0) for _ in range(nctx)]
    ranges = [npa.batch_split(batch, nctx, i) for i in range(nctx)]
    before = np.full((batch, n, SL), GARBAGE, np.uint8)
    for b, (_, rows, pr) in enumerate(pats):
        before[b][pr != 0] = rows[pr != 0]
    pres = np.stack([pr for _, _, pr in pats])
    d_sh = [_dev(before[b0:b0 + c]) for b0, c in ranges]
    d_pr = [_dev(pres[b0:b0 + c]) for b0, c in ranges]
    d_out = [torch.full((c, pay_len), FILLS["out"], dtype=torch.uint8, device="cuda") for _, c in ranges]
    d_bad = [torch.full((c,), 7, dtype=torch.int32, device="cuda") for _, c in ranges]
    d_map = [torch.full((c, n), FILLS["map"], dtype=torch.uint8, device="cuda") for _, c in ranges]
    d_st = [torch.full((c, 2), -1, dtype=torch.int32, device="cuda") for _, c in ranges]
    torch.cuda.synchronize()
    ptrs = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    npa.recover_batch_multi(ctxs, p, ptrs(d_sh), SL, n * SL, ptrs(d_pr), batch, d_out=ptrs(d_out), out_stride=pay_len,
                            restore=True, d_bad_rows=ptrs(d_bad), d_mismatch=ptrs(d_map), d_status=ptrs(d_st))
    torch.cuda.synchronize()
    got = np.concatenate([t.cpu().numpy() for t in d_sh])
    out = np.concatenate([t.cpu().numpy() for t in d_out])
    bad = np.concatenate([t.cpu().numpy() for t in d_bad]).view(np.uint32)
    mp = np.concatenate([t.cpu().numpy() for t in d_map])
    st = np.concatenate([t.cpu().numpy() for t in d_st])
    for b, (name, _, _) in enumerate(pats):
        want = before[b].copy()
        for v, data in (exp_rows[b] or {}).items():
            want[v] = np.frombuffer(data, np.uint8)
        assert np.array_equal(got[b], want), (b, name)
        if pays[b] is None:
            assert (out[b] == FILLS["out"]).all(), (b, name)
        else:
            assert out[b].tobytes() == pays[b], (b, name)
        assert int(bad[b]) == int(want_counts[b]) and np.array_equal(mp[b], want_flags[b]), (b, name)
        assert tuple(int(x) for x in st[b]) == status[b], (b, name)


@pytest.mark.parametrize("nctx", [2, 3])
def test_recover_batch_host_multi(gpu, oracle, nctx):
    """One guarded buffer set, nine payloads over 2 contexts (ranges of 5 and
    4) and 3 contexts, all three requests; and without status the mask check fails the
    whole call before any range runs."""
    case = _case(oracle, 1024, 342, SL)
    p, pats, exp = case
    ctxs = [npa.Context(0) for _ in range(nctx)]
    h = HostBatch(p, SL, pats, slack=100, out_slack=37)
    npa.recover_batch_host_multi(ctxs, *h.args(), **h.kwargs(ALL))
    h.check(exp, ALL, tag=f"nctx {nctx}")
    h = HostBatch(p, SL, pats)
    with pytest.raises(npa.NeedMoreShards) as ei:
        npa.recover_batch_host_multi(ctxs, *h.args(), **h.kwargs(ALL, with_status=False))
    assert ei.value == npa.NeedMoreShards(p.k() - 1, p.k(), p.n())
    h.check_untouched()

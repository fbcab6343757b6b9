"""The `_dev` calls across streams, host threads and scratch in flight.

Every `_dev` entry point is asynchronous on the caller's stream, but the prefix
/ big / huge / generic records, the tile slots and the statuses of a decode
(d_big), the payloads, plans, scratch rows, flags and statuses of a restore /
verify / recover (d_restore) and the plan of a ragged call (d_ragged, uploaded
through a ring of np_ctx::kRaggedStage pinned buffers) belong to the CONTEXT.
engine.cpp orders their users through three events (big_done, restore_done,
ragged_done: a launch waits for every earlier launch of the context on any
stream, and a buffer that must grow is freed only after the event is
synchronised) and one event per staging buffer (reused only after its last
upload has left it); the calls take the context lock and keep their error
detail per thread.  The rest of the suite hands the
library one stream and synchronises before it looks; these tests put two
streams, two host threads and the host pipeline on one context.

The gate (tests/_stream_gate.py).  A call only competes with one that has not
started, so every case queues a bounded sleep on the victim's stream, records
`gate_end` behind it, enqueues the victim and then the competitors, and reads
`gate_end.query()` from the host: the gate must still be running (repeated
with the gate doubled, three gates at the most, then the test fails).  Were one
of the library's waits missing, a competitor on another stream would simply run
whole BEFORE the victim -- and two calls that run one after the other are both
right in either order.  So the two-stream cases also wait, from the host, for
the competitor's stream alone and assert that the gate is over by then: the
competitor was ordered behind the pending call, as engine.cpp promises ("after
every earlier launch of this context on any stream").  Where a call must block
the host itself (growth of a scratch buffer under a pending call, reuse of a
staging buffer whose upload is pending) that is asserted right after the call.

A failure is a wrong answer, never a fault: victim and competitor have the same
(n, k, wanted_n), shard_len, batch and strides (ragged: the same items), and
differ in their buffers, bytes and presence patterns -- other absent rows, the
copy-mode and the k - 1 payload at other indices -- so a record, plan or status
that reaches the wrong call still names rows and addresses inside a live buffer
of the right size.  Everything is compared bit for bit with the oracle
(test_gpu_recover._patterns / expected_recover, the ragged cases of
test_gpu_ragged_recover), buffers whole, fills and guards included.

No checked-build (`*_bounds.py`) child runs this file: that child is written
for one launch at a time (NP_PIPE_SLOTS=1), and its counters are not made for
kernels of several streams running at once."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import novelpoly_amd as npa
from _stream_gate import Gate, run_gated
from test_gpu_ragged import Case as RaggedCase
from test_gpu_ragged_recover import _check as ragged_check
from test_gpu_ragged_recover import _out_items, _recover_case
from test_gpu_ragged_masked import _mcase
from test_gpu_recover import FILL, GUARD, OUT_SLACK, _patterns, expected_recover
from test_gpu_recover_host import ALL, HostBatch
from test_gpu_recover_host import _case as host_case
from test_gpu_recover_host import _subset

pytestmark = pytest.mark.gpu

RING = 4  # np_ctx::kRaggedStage

# key: ((n, k, wanted_n), shard_len) -- the smallest shape of each scratch user
SHAPES = {
    "F": ((256, 64, 256), 2 * 300),      # derive(256, 86): fast decode, direct masked encodes
    "S": ((64, 16, 60), 2 * 300),        # derive(60, 20): small, scratch-row masked path
    "R": ((1024, 512, 1024), 42),        # resident
    "B": ((4096, 2048, 4096), 42),       # big records + tile scratch; big encode scratch
    "H": ((8192, 4096, 8192), 42),       # huge
    "G": ((1024, 64, 1000), 2 * 300),    # generic reconstruct, n / k = 16
}
# Five payloads per set: the copy-mode payload at 1 / 4, the k - 1 payload at 3 / 0
NAMES = {"A": ["window", "copy-mode", "random", "k-1", "parity-absent"],
         "B": ["k-1", "exactly-k", "systematic-absent+parity-flip", "all-present", "copy-mode"]}


def test_shapes_are_the_derived_ones():
    for key, nw, kw in (("F", 256, 86), ("S", 60, 20)):
        d = npa.CodeParams.derive_parameters(nw, kw)
        assert (d.n(), d.k(), d.wanted_n) == SHAPES[key][0]


def _payloads_only(oracle, p, sl, pats):
    """expected_recover without the re-encoding: (None, (None, None, status), payloads)."""
    n, k = p.n(), p.k()
    pays, status = [], []
    for name, rows, pr in pats:
        st, pay = oracle.reconstruct([rows[v].tobytes() if pr[v] else None for v in range(n)], n, k)
        assert st == (npa.NeedMoreShards.code if name == "k-1" else 0), name
        pays.append(None if st else pay)
        status.append((st, int(pr.sum())))
    return None, (None, None, status), pays


@functools.lru_cache(maxsize=None)
def _set(oracle, key, which, full):
    """(p, shard_len, patterns, expectations) of pattern set `which` of a shape,
    computed once (read only).  full: with the restored rows and the verdict."""
    (n, k, wn), sl = SHAPES[key]
    p = npa.CodeParams(n, k, wn)
    rng = np.random.default_rng(31 * n + 7 * k + wn + sl + (0 if which == "A" else 1000003))
    by_name = {name: (name, rows, pr) for name, rows, pr in _patterns(oracle, rng, n, k, wn, sl)}
    pats = [by_name[name] for name in NAMES[which]]
    exp = expected_recover(oracle, p, sl, pats) if full else _payloads_only(oracle, p, sl, pats)
    assert [b for b, pay in enumerate(exp[2]) if pay is None] == [NAMES[which].index("k-1")]
    return p, sl, pats, exp


def _repeat(case, batch):
    """The set's payloads over and over, `batch` of them."""
    p, sl, pats, exp = case
    keep = [b % len(pats) for b in range(batch)]
    _, pats, exp = _subset((p, pats, exp), keep)
    return p, sl, pats, exp


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, copy=True)).cuda()


def _runs_beside(victim, other):
    """True if work on `other` finishes while a sleep on `victim` is running:
    the two do not share a hardware queue."""
    import torch

    g = Gate(victim, 2.0)
    with torch.cuda.stream(other):
        torch.empty(64, device="cuda").zero_()
    beside = not _behind(g, other)
    victim.synchronize()
    return beside


def _streams(count=2):
    """Streams for a case, the first for the victim.  The process has fewer
    hardware queues than torch has streams (4 by default), and work on a stream
    that shares the victim's queue waits behind the gate whatever the library
    does; so the others are picked, among a few of torch's pool, from those that
    were seen to run beside a sleep on the first.  (If none is found the case
    still runs, and its ordering assertions hold trivially.)"""
    import torch

    torch.cuda.synchronize()
    got = [torch.cuda.Stream()]
    for _ in range(8):
        if len(got) == count:
            break
        cand = torch.cuda.Stream()
        if all(cand.cuda_stream != s.cuda_stream for s in got) and _runs_beside(got[0], cand):
            got.append(cand)
    while len(got) < count:
        got.append(torch.cuda.Stream())
    return got


def _gate(gate_ms, victim_stream, *others):
    """The gate on the victim's stream, behind everything the test's stream has
    queued so far (the inputs, which the other streams wait for as well)."""
    import torch

    for s in (victim_stream,) + others:
        s.wait_stream(torch.cuda.current_stream())
    return Gate(victim_stream, gate_ms)


def _behind(g, stream):
    """Waits for `stream` alone; true if the gate is over by then (what was
    queued on `stream` ran behind the call that waits behind the gate)."""
    import torch

    done = torch.cuda.Event()
    done.record(stream)
    done.synchronize()
    return not g.open()


UNORDERED = "the competing call finished while the call queued before it had not started: it did not wait for it"


class Dev:
    """The device buffers of one uniform call on `pats`, each pre-filled, and the
    check of every byte of them after the call made through one of the methods."""

    def __init__(self, case):
        import torch

        self.p, self.sl, self.pats, self.exp = case
        n, k = self.p.n(), self.p.k()
        self.batch, self.stride = len(self.pats), n * self.sl + 64
        self.pay_len = (self.sl // 2) * 2 * k
        self.ostride = self.pay_len + OUT_SLACK
        self.before = np.full(self.batch * self.stride + 64, FILL, np.uint8)
        for b, (_, rows, pr) in enumerate(self.pats):
            view = self.before[b * self.stride: b * self.stride + n * self.sl].reshape(n, self.sl)
            view[pr != 0] = rows[pr != 0]
        self.buf = _dev(self.before)
        self.pres = _dev(np.stack([pr for _, _, pr in self.pats]))
        self.out = torch.full((self.batch, self.ostride), GUARD, dtype=torch.uint8, device="cuda")
        self.cnt = torch.full((self.batch,), 7, dtype=torch.int32, device="cuda")
        self.map = torch.full((self.batch, n), GUARD, dtype=torch.uint8, device="cuda")
        self.st = torch.full((self.batch, 2), -1, dtype=torch.int32, device="cuda")
        self.req = None

    def _args(self):
        return self.p, self.buf.data_ptr(), self.sl, self.stride, self.pres.data_ptr()

    def reconstruct(self, ctx, stream, with_status=True):
        self.req = dict(out=True, restore=False, verify=False, map=False, status=with_status)
        npa.reconstruct_batch_dev2(*self._args(), 0, self.batch, self.out.data_ptr(), self.ostride, ctx=ctx,
                                   stream=stream.cuda_stream, d_status=self.st.data_ptr() if with_status else 0)

    def restore(self, ctx, stream, with_status=True):
        self.req = dict(out=False, restore=True, verify=False, map=False, status=with_status)
        npa.restore_shards_batch_dev(*self._args(), self.batch, ctx=ctx, stream=stream.cuda_stream,
                                     d_status=self.st.data_ptr() if with_status else 0)

    def verify(self, ctx, stream, with_map=False, with_status=True):
        self.req = dict(out=False, restore=False, verify=True, map=with_map, status=with_status)
        npa.verify_shards_batch_dev(*self._args(), self.batch, self.cnt.data_ptr(), ctx=ctx, stream=stream.cuda_stream,
                                    d_mismatch=self.map.data_ptr() if with_map else 0,
                                    d_status=self.st.data_ptr() if with_status else 0)

    def recover(self, ctx, stream, with_out=True, restore=True, verify=True, with_map=True, with_status=True):
        self.req = dict(out=with_out, restore=restore, verify=verify, map=with_map and verify, status=with_status)
        npa.recover_batch_dev(*self._args(), self.batch, ctx=ctx, stream=stream.cuda_stream,
                              d_out=self.out.data_ptr() if with_out else 0, out_stride=self.ostride if with_out else 0,
                              restore=restore, d_bad_rows=self.cnt.data_ptr() if verify else 0,
                              d_mismatch=self.map.data_ptr() if with_map and verify else 0,
                              d_status=self.st.data_ptr() if with_status else 0)

    def check(self, tag):
        """After the caller synchronised: every buffer, whole, against the oracle
        or its fill."""
        rows, (want_flags, want_counts, status), pays = self.exp
        n, sl, req = self.p.n(), self.sl, self.req
        tag = f"{tag} {req}"
        want = self.before.copy()
        if req["restore"]:
            for b in range(self.batch):
                view = want[b * self.stride: b * self.stride + n * sl].reshape(n, sl)
                for v, data in (rows[b] or {}).items():
                    view[v] = np.frombuffer(data, np.uint8)
        got = self.buf.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            where = sorted({(int(x) // self.stride, (int(x) % self.stride) // sl) for x in bad[:4096]})[:8]
            raise AssertionError(f"{tag}: {bad.size} shard bytes differ, (payload, row) {where}")
        want = np.full((self.batch, self.ostride), GUARD, np.uint8)
        if req["out"]:
            for b, pay in enumerate(pays):
                if pay is not None:
                    want[b, :self.pay_len] = np.frombuffer(pay, np.uint8)
        got = self.out.cpu().numpy()
        wrong = [(b, self.pats[b][0]) for b in range(self.batch) if not np.array_equal(got[b], want[b])]
        assert not wrong, (tag, "payloads that differ", wrong)
        got = self.cnt.cpu().numpy()
        if req["verify"]:
            assert got.view(np.uint32).tolist() == np.asarray(want_counts).tolist(), (tag, "counts")
        else:
            assert (got == 7).all(), (tag, "counts written")
        got = self.map.cpu().numpy()
        if req["map"]:
            wrong = [(b, self.pats[b][0]) for b in range(self.batch) if not np.array_equal(got[b], want_flags[b])]
            assert not wrong, (tag, "maps that differ", wrong)
        else:
            assert (got == GUARD).all(), (tag, "map written")
        got = self.st.cpu().numpy()
        if req["status"]:
            assert [tuple(int(x) for x in r) for r in got] == [tuple(x) for x in status], (tag, "status")
        else:
            assert (got == -1).all(), (tag, "status written")


class DevEncode:
    """np_encode_batch_dev of the payloads a set decodes to (payload length
    shard_len / 2 * 2k, so the shape and the batch are the decode's; random
    bytes in place of the payload that does not decode), into a filled buffer."""

    def __init__(self, oracle, case):
        import torch

        self.p, self.sl, pats, exp = case
        n, k, wn = self.p.n(), self.p.k(), self.p.wanted_n
        self.pay_len = (self.sl // 2) * 2 * k
        rng = np.random.default_rng(n + k)
        pays = tuple(rng.integers(0, 256, self.pay_len, dtype=np.uint8).tobytes() if pay is None else pay
                     for pay in exp[2])
        self.batch, self.stride = len(pays), n * self.sl + 64
        self.want = _encoded(oracle, (n, k, wn), self.sl, pays, self.stride)
        self.payloads = _dev(np.frombuffer(b"".join(pays), np.uint8))
        self.shards = torch.full((self.batch * self.stride + 64,), FILL, dtype=torch.uint8, device="cuda")

    def encode(self, ctx, stream):
        npa.encode_batch_dev(self.p, self.payloads.data_ptr(), self.pay_len, self.pay_len, self.batch,
                             self.shards.data_ptr(), self.stride, ctx=ctx, stream=stream.cuda_stream)

    def check(self, tag):
        got = self.shards.cpu().numpy()
        if not np.array_equal(got, self.want):
            bad = np.flatnonzero(got != self.want)
            where = sorted({(int(x) // self.stride, (int(x) % self.stride) // self.sl) for x in bad[:4096]})[:8]
            raise AssertionError(f"{tag}: {bad.size} encoded bytes differ, (payload, row) {where}")


@functools.lru_cache(maxsize=None)
def _encoded(oracle, nkw, sl, pays, stride):
    n, k, wn = nkw
    want = np.full(len(pays) * stride + 64, FILL, np.uint8)
    for b, pay in enumerate(pays):
        st, rows = oracle.encode(pay, n, k, wn)
        assert st == 0 and len(rows) == wn and len(rows[0]) == sl
        want[b * stride: b * stride + wn * sl] = np.frombuffer(b"".join(rows), np.uint8)
    want.setflags(write=False)
    return want


class DevRagged:
    """The device buffers of one ragged call on case `c` with the staged rows
    and expectations `e` (test_gpu_ragged_recover.expected_items)."""

    def __init__(self, c, e):
        import torch

        self.c, self.e = c, e
        batch = len(c.items)
        self.buf, self.pres = _dev(e.before), _dev(e.pres)
        self.out = torch.full((c.psize,), GUARD, dtype=torch.uint8, device="cuda")
        self.cnt = torch.full((4 * batch,), GUARD, dtype=torch.uint8, device="cuda")
        self.map = torch.full((batch, c.n), GUARD, dtype=torch.uint8, device="cuda")
        self.st = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
        self.req = None

    def reconstruct(self, ctx, stream, with_status=True):
        c = self.c
        self.req = (True, False, False, with_status, False)
        npa.reconstruct_ragged_dev(c.p, self.buf.data_ptr(), c.ssize, self.pres.data_ptr(), self.out.data_ptr(), c.psize,
                                   c.items, ctx=ctx, stream=stream.cuda_stream,
                                   d_status=self.st.data_ptr() if with_status else 0)

    def recover(self, ctx, stream, with_map=True, with_status=True):
        """All three requests."""
        c = self.c
        self.req = (True, True, True, with_status, with_map)
        npa.recover_ragged_dev(c.p, self.buf.data_ptr(), c.ssize, self.pres.data_ptr(), _out_items(c),
                               d_out=self.out.data_ptr(), out_size=c.psize, restore=True, d_bad_rows=self.cnt.data_ptr(),
                               d_mismatch=self.map.data_ptr() if with_map else 0,
                               d_status=self.st.data_ptr() if with_status else 0, ctx=ctx, stream=stream.cuda_stream)

    def check(self, tag):
        res = tuple(t.cpu().numpy() for t in (self.buf, self.out, self.cnt, self.map, self.st))
        ragged_check(self.c, self.e, res, *self.req, f"{tag} {self.req}")


class DevRaggedEncode:
    """np_encode_ragged_dev of a case of test_gpu_ragged.py into a filled buffer."""

    def __init__(self, c):
        self.c = c
        self.payloads = _dev(c.payloads)
        self.shards = _dev(np.full(c.ssize, FILL, np.uint8))

    def encode(self, ctx, stream):
        c = self.c
        npa.encode_ragged_dev(c.p, self.payloads.data_ptr(), c.psize, self.shards.data_ptr(), c.ssize, c.items, ctx=ctx,
                              stream=stream.cuda_stream)

    def check(self, tag):
        got = self.shards.cpu().numpy()
        if not np.array_equal(got, self.c.shards):  # the items' rows, and the fill everywhere else
            bad = np.flatnonzero(got != self.c.shards)
            raise AssertionError(f"{tag}: {bad.size} bytes differ, first at {bad[:8].tolist()}")


@functools.lru_cache(maxsize=None)
def _ragged_payloads(oracle, batch, seed):
    """F's ragged batch (the items of test_gpu_ragged.py) with the payloads of `seed`: one geometry for every seed."""
    c = RaggedCase(oracle, 256, 86, batch, seed=seed)
    assert c.items == _mcase(oracle, 256, 86, batch).items
    return c


def _sync():
    import torch

    torch.cuda.synchronize()


# ---- 1: d_big across two streams -------------------------------------------
@pytest.mark.parametrize("with_status", [True, False], ids=["status", "own-status"])
@pytest.mark.parametrize("key", list(SHAPES))
def test_big_scratch_two_streams(gpu, oracle, key, with_status):
    """np_reconstruct_batch_dev3 without locators behind the gate on stream 1,
    the same call with the other pattern set on stream 2: the records (and,
    without d_status, the statuses) of both live in d_big."""
    a, b = _set(oracle, key, "A", False), _set(oracle, key, "B", False)
    s1, s2 = _streams()

    def case(gate_ms):
        v, c = Dev(a), Dev(b)
        g = _gate(gate_ms, s1, s2)
        v.reconstruct(gpu, s1, with_status)
        c.reconstruct(gpu, s2, with_status)
        ms, held = g.host_ms(), g.open()
        behind = _behind(g, s2)
        _sync()
        v.check("victim")
        c.check("competitor")
        assert behind or not gate_ms, UNORDERED
        return held, ms

    run_gated(case, label=f"d_big {key} status {with_status}")


@pytest.mark.parametrize("key", ["B", "H"])
def test_big_scratch_decode_and_encode(gpu, oracle, key):
    """The decode behind the gate, np_encode_batch_dev of the same shape on
    stream 2: the encode's tile scratch and the decode's records share d_big."""
    a, b = _set(oracle, key, "A", False), _set(oracle, key, "B", False)
    s1, s2 = _streams()

    def case(gate_ms):
        v, c = Dev(a), DevEncode(oracle, b)
        g = _gate(gate_ms, s1, s2)
        v.reconstruct(gpu, s1, False)
        c.encode(gpu, s2)
        ms, held = g.host_ms(), g.open()
        behind = _behind(g, s2)
        _sync()
        v.check("victim")
        c.check("competing encode")
        assert behind or not gate_ms, UNORDERED
        return held, ms

    run_gated(case, label=f"d_big {key} decode + encode")


# ---- 2: d_restore across two streams ---------------------------------------
@pytest.mark.parametrize("with_out", [True, False], ids=["out", "no-out"])
@pytest.mark.parametrize("key", ["F", "S"])
def test_restore_scratch_two_streams(gpu, oracle, key, with_out):
    """np_recover_batch_dev with all requests behind the gate (without d_out its
    payloads live in d_restore, as the plan or the scratch rows do either way);
    on stream 2 a restore, a verify with its flag map in scratch and a
    restore-only recover of the other pattern set."""
    a, b = _set(oracle, key, "A", True), _set(oracle, key, "B", True)
    s1, s2 = _streams()

    def case(gate_ms):
        v, c1, c2, c3 = Dev(a), Dev(b), Dev(b), Dev(b)
        g = _gate(gate_ms, s1, s2)
        v.recover(gpu, s1, with_out=with_out, with_map=True, with_status=with_out)
        c1.restore(gpu, s2, with_status=False)
        c2.verify(gpu, s2, with_map=False, with_status=False)
        c3.recover(gpu, s2, with_out=False, restore=True, verify=False)
        ms, held = g.host_ms(), g.open()
        behind = _behind(g, s2)
        _sync()
        v.check("victim")
        for name, c in (("restore", c1), ("verify", c2), ("restore-only recover", c3)):
            c.check(f"competing {name}")
        assert behind or not gate_ms, UNORDERED
        return held, ms

    run_gated(case, label=f"d_restore {key} out {with_out}")


# ---- 3: growth under a pending call ----------------------------------------
@pytest.mark.parametrize("kind", ["reconstruct", "recover"])
def test_growth_waits_for_the_pending_call(oracle, kind):
    """A fresh context: the victim (F, batch 2) allocates the scratch and waits
    behind the gate; the same call at batch 64 on stream 2 needs a larger d_big
    (recover: d_restore too) and may free the old buffer only once the victim is
    through with it -- the call returns after the gate, and both are right."""
    small = _repeat(_set(oracle, "F", "A", True), 2)
    large = _repeat(_set(oracle, "F", "B", True), 64)
    s1, s2 = _streams()

    def call(d, ctx, s):
        if kind == "reconstruct":
            d.reconstruct(ctx, s, with_status=False)
        else:
            d.recover(ctx, s, with_out=False, with_map=False, with_status=False)

    def case(gate_ms):
        ctx = npa.Context(0)
        v, c = Dev(small), Dev(large)
        g = _gate(gate_ms, s1, s2)
        call(v, ctx, s1)
        ms, held = g.host_ms(), g.open()  # the victim is queued and has not started
        call(c, ctx, s2)
        over = not g.open()
        _sync()
        ctx.close()
        v.check("victim (batch 2)")
        c.check("competitor (batch 64)")
        assert over, "the growing call returned while the call using the old scratch had not started"
        return held, ms

    run_gated(case, label=f"growth {kind}", warm=False)


def test_ragged_growth_waits_for_the_pending_call(oracle):
    """The ragged twin: the second encode's plan (11 items) is larger than the
    d_ragged the first (1 item) allocated."""
    one, many = _ragged_payloads(oracle, 1, 0), _ragged_payloads(oracle, 11, 0)
    s1, s2 = _streams()

    def case(gate_ms):
        ctx = npa.Context(0)
        v, c = DevRaggedEncode(one), DevRaggedEncode(many)
        g = _gate(gate_ms, s1, s2)
        v.encode(ctx, s1)
        ms, held = g.host_ms(), g.open()
        c.encode(ctx, s2)
        over = not g.open()
        _sync()
        ctx.close()
        v.check("victim (1 item)")
        c.check("competitor (11 items)")
        assert over, "the growing call returned while the call using the old plan buffer had not started"
        return held, ms

    run_gated(case, label="growth ragged", warm=False)


# ---- 4: the ragged plan and its staging ring -------------------------------
def test_ragged_plan_two_streams(gpu, oracle):
    """np_encode_ragged_dev keeps nothing in context memory but its plan in
    d_ragged: the encode behind the gate on stream 1 and one of other payloads
    on stream 2 are ordered through ragged_done alone."""
    s1, s2 = _streams()

    def case(gate_ms):
        v, c = DevRaggedEncode(_ragged_payloads(oracle, 8, 0)), DevRaggedEncode(_ragged_payloads(oracle, 8, 1))
        g = _gate(gate_ms, s1, s2)
        v.encode(gpu, s1)
        c.encode(gpu, s2)
        ms, held = g.host_ms(), g.open()
        behind = _behind(g, s2)
        _sync()
        v.check("victim")
        c.check("competitor")
        assert behind or not gate_ms, UNORDERED
        return held, ms

    run_gated(case, label="d_ragged encode")


def _ring(gpu, make, run, label):
    """RING + 2 calls of identical geometry behind one gate, alternating between
    two streams.  Each makes one ragged_upload (np_encode_ragged_dev: one per
    call; np_reconstruct_ragged_dev: one per slice, and F's batch is one slice;
    np_recover_ragged_dev: one per slice in ragged_masked_reconstruct), so call
    RING takes the last free staging buffer and call RING + 1 the first one
    again, whose upload is still behind the gate: it returns after the gate."""
    streams = _streams()

    def case(gate_ms):
        devs = [make(j) for j in range(RING + 2)]
        g = _gate(gate_ms, *streams)
        for j in range(RING):
            run(devs[j], j, gpu, streams[j % 2])
        ms, held = g.host_ms(), g.open()  # the ring is full and nothing has started
        run(devs[RING], RING, gpu, streams[RING % 2])
        over = not g.open()
        run(devs[RING + 1], RING + 1, gpu, streams[(RING + 1) % 2])
        _sync()
        for j, d in enumerate(devs):
            d.check(f"call {j}")
        assert over or not gate_ms, "a staging buffer was refilled while its last upload had not started"
        return held, ms

    run_gated(case, label=label)


def test_staging_ring_encode(gpu, oracle):
    _ring(gpu, lambda j: DevRaggedEncode(_ragged_payloads(oracle, 8, j)), lambda d, j, ctx, s: d.encode(ctx, s),
          "ring encode")


def test_staging_ring_reconstruct(gpu, oracle):
    """n = 4k: the two-launch decode.  Call j carries the patterns rotated by j."""
    c = _mcase(oracle, 256, 86, 8)
    _ring(gpu, lambda j: DevRagged(c, _recover_case(oracle, 256, 86, 8, j)),
          lambda d, j, ctx, s: d.reconstruct(ctx, s, with_status=False), "ring reconstruct")


def test_staging_ring_recover(gpu, oracle):
    """All three requests; every other call keeps its flag map in scratch."""
    c = _mcase(oracle, 256, 86, 8)
    _ring(gpu, lambda j: DevRagged(c, _recover_case(oracle, 256, 86, 8, j)),
          lambda d, j, ctx, s: d.recover(ctx, s, with_map=bool(j % 2), with_status=False), "ring recover")


# ---- 5: one stream, gated --------------------------------------------------
def test_one_stream_gated(gpu, oracle):
    """Seven calls on one stream behind the gate, nothing synchronised in
    between: each call's records, plan, rows and statuses in the shared scratch
    outlive the enqueueing of the calls behind it.  The largest user of each
    buffer comes first, and the ungated first run has grown them all."""
    s1, = _streams(1)
    rag = _mcase(oracle, 256, 86, 8)

    def case(gate_ms):
        calls = [("B reconstruct", Dev(_set(oracle, "B", "A", False)), lambda d: d.reconstruct(gpu, s1, False)),
                 ("F reconstruct", Dev(_set(oracle, "F", "A", True)), lambda d: d.reconstruct(gpu, s1, False)),
                 ("G reconstruct", Dev(_set(oracle, "G", "A", False)), lambda d: d.reconstruct(gpu, s1, False)),
                 ("S verify", Dev(_set(oracle, "S", "A", True)), lambda d: d.verify(gpu, s1, False, False)),
                 ("F restore", Dev(_set(oracle, "F", "A", True)), lambda d: d.restore(gpu, s1, False)),
                 ("F ragged recover", DevRagged(rag, _recover_case(oracle, 256, 86, 8, 0)),
                  lambda d: d.recover(gpu, s1, with_map=False, with_status=False)),
                 ("F reconstruct again", Dev(_set(oracle, "F", "B", True)), lambda d: d.reconstruct(gpu, s1, False))]
        g = _gate(gate_ms, s1)
        for _, d, run in calls:
            run(d)
        ms, held = g.host_ms(), g.open()
        _sync()
        for name, d, _ in calls:
            d.check(name)
        return held, ms

    run_gated(case, label="one stream, seven calls")


# ---- 6: two host threads, one context --------------------------------------
THREAD_CALLS = 20
THREAD_GATE_MS = 1.0  # each call is still queued while the other thread enqueues its next one


def test_two_host_threads_one_context(gpu, oracle):
    """Two threads, a stream each, 20 calls each on one context: F and S in
    turn, recover with every request and reconstruct in turn, own buffers and
    pattern sets, every result checked once the thread's stream is through.
    Halfway each thread makes one call that fails its validation -- an odd
    shard_len, a pair with no power of two -- and, after both have failed, reads
    its own status and np_last_error_detail."""
    import torch

    streams = _streams()
    work = [[], []]
    for t, which in enumerate("AB"):
        for i in range(THREAD_CALLS):
            work[t].append(Dev(_set(oracle, "FS"[i % 2], which, True)))
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    Gate(streams[0], 0.1)  # (the calibration, in this thread)
    L = npa.lib()
    both_failed = threading.Barrier(2)
    failures = [None, None]

    def provoke(t, d):
        p = d.p if t == 0 else npa.CodeParams(100, 30, 100)
        sl = d.sl + 1 if t == 0 else d.sl
        st = L.np_reconstruct_batch_dev3(gpu.handle, ctypes.byref(p._c()), d.buf.data_ptr(), sl, d.stride,
                                         d.pres.data_ptr(), None, d.batch, d.out.data_ptr(), d.ostride, None,
                                         streams[t].cuda_stream)
        both_failed.wait(timeout=60)
        det = (ctypes.c_size_t * 3)()
        L.np_last_error_detail(det)
        want = (npa.EmptyShard.code, (0, 0, 0)) if t == 0 else (npa.ParamterMustBePowerOf2.code, (100, 30, 0))
        assert (st, tuple(det)) == want, f"thread {t}: status and detail {(st, tuple(det))}, its own are {want}"

    def run(t):
        try:
            s = streams[t]
            with torch.cuda.stream(s):
                for i, d in enumerate(work[t]):
                    Gate(s, THREAD_GATE_MS)
                    if (i // 2) % 2 == 0:
                        d.recover(gpu, s, with_out=bool(i & 4), with_map=bool(i & 8), with_status=bool(i & 4))
                    else:
                        d.reconstruct(gpu, s, with_status=bool(i & 4))
                    if i == THREAD_CALLS // 2:
                        provoke(t, d)
                    s.synchronize()
                    d.check(f"thread {t} call {i}")
        except BaseException as e:  # noqa: B902 -- reported by the test's thread
            failures[t] = e
            both_failed.abort()

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    _sync()
    real = [e for e in failures if e is not None and not isinstance(e, threading.BrokenBarrierError)]
    for e in real or [e for e in failures if e is not None]:
        raise e


# ---- 7: the host pipeline next to a device call ----------------------------
def test_host_pipeline_next_to_a_device_call(gpu, oracle, monkeypatch):
    """A device recover waits behind the gate; a thread runs
    np_recover_batch_host (F, nine patterns, five sub-batches of 2 over the
    pipeline's streams) on the same context while this thread issues a second
    device recover.  The context lock serialises the host call and the second
    device call, in either order; the pipeline's streams must still wait for the
    pending call's use of d_restore / d_big, so the host call returns after the
    gate."""
    monkeypatch.setenv("NP_PIPE_SB", "2")
    a, b = _set(oracle, "F", "A", True), _set(oracle, "F", "B", True)
    hp, hpats, hexp = host_case(oracle, 256, 86, 2 * 300)
    s1, s2 = _streams()

    def case(gate_ms):
        h = HostBatch(hp, 2 * 300, hpats)
        v, c = Dev(a), Dev(b)
        seen = {}

        def host():
            try:
                npa.recover_batch_host(*h.args(), ctx=gpu, **h.kwargs(ALL))
                seen["over"] = not g.open()
            except BaseException as e:  # noqa: B902 -- reported by the test's thread
                seen["error"] = e

        g = _gate(gate_ms, s1, s2)
        v.recover(gpu, s1, with_out=False, with_map=False, with_status=False)
        ms, held = g.host_ms(), g.open()
        th = threading.Thread(target=host)
        th.start()
        c.recover(gpu, s2, with_out=False, with_map=False, with_status=False)
        th.join()
        _sync()
        if "error" in seen:
            raise seen["error"]
        v.check("pending device call")
        c.check("second device call")
        h.check(hexp, ALL, tag="host pipeline")
        assert seen["over"] or not gate_ms, "the host pipeline finished while the device call before it had not started"
        return held, ms

    run_gated(case, label="host pipeline + device recover")

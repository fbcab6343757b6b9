"""The row-masked encodes of np_restore_shards_batch_dev and
np_verify_shards_batch_dev (kernels_fast_planned.hip k_encode_masked / k_encode_verify,
fed by kernels_restore.hip k_restore_plan / k_verify_plan) over what their plan
decides per payload: every set of marked size-k segments at n / k in {2, 4, 8},
three shard lengths (a partial tile, a full plus a partial tile, the streaming
store path), batches of 8 and 16 payloads with two tiles each, a wanted_n that
ends inside a segment, and the wide codes n / k in {16, 32, 64, 1024} whose
segment bits fill one plan word exactly or span several.

Every comparison is byte for byte against the oracle's
encode(reconstruct(received)), through the runners of test_gpu_restore.py and
test_gpu_verify.py.  A segment is MARKED for the restore when it holds an
absent row below wanted_n of a decodable payload, for the verify when it holds
a present row in [k, wanted_n) of one; each test prints the marked sets it
reaches and asserts that they are the ones it names."""
import itertools

import numpy as np
import pytest

import novelpoly_amd as npa
from test_gpu_restore import expected_rows, run_restore
from test_gpu_verify import SWEEP_VARIANTS, _codeword, _flip, expected_case, run_verify

pytestmark = pytest.mark.gpu

SL_TAIL = 2 * 5      # five columns: lane 0 holds four, lane 1 a tail of one
SL_TWO = 2 * 261     # a full 256-column tile plus that partial tile
SL_STREAM = 512      # one full tile; with a 128-byte-aligned base and stride the streaming stores
KS = (64, 128, 256)
RATIOS = (2, 4, 8)


# ------------------------------------------------------------ patterns ----
def _pick_rows(rng, lo, hi, count, mode):
    """`count` distinct rows of [lo, hi) (all of them when it has fewer): lo
    among them when mode & 1, hi - 1 when mode & 2, the others random and in
    different 16-row groups while the range has unused ones."""
    count = min(count, hi - lo)
    picks = []
    if mode & 1:
        picks.append(lo)
    if mode & 2 and len(picks) < count and hi - 1 not in picks:
        picks.append(hi - 1)
    for grp in rng.permutation(np.arange(lo // 16, (hi + 15) // 16)):
        if len(picks) >= count:
            break
        if any(r // 16 == grp for r in picks):
            continue
        picks.append(int(rng.integers(max(lo, 16 * grp), min(hi, 16 * grp + 16))))
    while len(picks) < count:
        r = int(rng.integers(lo, hi))
        if r not in picks:
            picks.append(r)
    return sorted(picks)


def _seg_range(q, k, wn):
    """Rows of segment q below wanted_n."""
    return q * k, min((q + 1) * k, wn)


def _live_segments(k, wn):
    return (wn + k - 1) // k


def _above(rng, pres, wn, mode):
    """Rows at and above wanted_n: absent (mode 0), present (1) or random (2)."""
    if mode == 1:
        pres[wn:] = 1
    elif mode == 2:
        pres[wn:] = rng.integers(0, 2, pres.size - wn, dtype=np.uint8)
    else:
        pres[wn:] = 0


def _restore_payload(rng, n, k, wn, sl, segs, b, above=0):
    """Random received bytes; rows to restore in exactly the segments `segs`:
    1-3 per segment, chosen by _pick_rows."""
    pres = np.ones(n, np.uint8)
    _above(rng, pres, wn, above)
    for q in segs:
        lo, hi = _seg_range(q, k, wn)
        pres[_pick_rows(rng, lo, hi, 1 + (b + q) % 3, (b + q) % 4)] = 0
    name = "restore-" + ("+".join(map(str, segs)) if len(segs) <= 8 else f"{len(segs)}-segments") + f"-above{above}"
    return name, rng.integers(0, 256, (n, sl), dtype=np.uint8), pres


def _verify_payload(rng, code, n, k, wn, sl, segs, b, above=0, whole=None, flips=None):
    """A codeword (every row of it, those above wanted_n included) with present
    parity rows in exactly the segments `segs` (1, 2 or all rows of each; all
    where whole(q)).  Even b keeps every systematic row, odd b drops one or two
    while more than k rows stay present.  One bit is altered in a present row of
    b % 3 (or `flips`) of the segments: in row positions 8..15 of a 16-row group
    for odd b // 3 where the segment has one, in 0..7 otherwise."""
    rows = code.copy()
    pres = np.zeros(n, np.uint8)
    pres[:k] = 1
    _above(rng, pres, wn, above)
    for q in segs:
        lo, hi = _seg_range(q, k, wn)
        kind = (b + q) % 3 if whole is None else (2 if whole(q) else (b + q) % 2)
        pres[lo:hi] = 1 if kind == 2 else 0
        if kind != 2:
            pres[_pick_rows(rng, lo, hi, 1 + kind, (b // 3 + q) % 4)] = 1
    parity = int(pres[k:].sum())  # present rows the decode sees besides the systematic ones
    drop = min(1 + (b // 2) % 2, parity - 1) if b % 2 and segs else 0
    if drop > 0:
        pres[rng.choice(k, drop, replace=False)] = 0
    flipped = []
    for q in list(rng.permutation(segs))[: b % 3 if flips is None else flips]:
        lo, hi = _seg_range(int(q), k, wn)
        cand = lo + np.flatnonzero(pres[lo:hi])
        half = cand[(cand % 16 >= 8) == bool((b // 3) % 2)]
        v = int(rng.choice(half if half.size else cand))
        # symbols 0, 255 (the full tile's last), 256.. (the partial tile) and any
        sym = int(rng.choice([0, min(255, sl // 2 - 1), sl // 2 - 1, int(rng.integers(0, sl // 2))]))
        _flip(rows, v, sym, rng)
        flipped.append(v)
    # every systematic row present: the decode copies them, and exactly the altered rows mismatch
    exact = sorted(flipped) if drop <= 0 else None
    name = "verify-" + ("+".join(map(str, segs)) if len(segs) <= 8 else f"{len(segs)}-segments")
    return name + f"-above{above}-drop{max(drop, 0)}-flip{len(flipped)}", rows, pres, exact


def _undecodable(rng, n, k, wn, sl, verify):
    """Random bytes with k - 1 present rows, all below wanted_n."""
    pres = np.zeros(n, np.uint8)
    pres[rng.choice(wn, k - 1, replace=False)] = 1
    rows = rng.integers(0, 256, (n, sl), dtype=np.uint8)
    return ("k-1", rows, pres, None) if verify else ("k-1", rows, pres)


def _marked(pats, k, wn, verify):
    """The marked segments of every payload, from its present flags alone."""
    out = []
    for pat in pats:
        pres = pat[2]
        if int(pres.sum()) < k:
            out.append(())
            continue
        rows = np.flatnonzero(pres[:wn] != 0) if verify else np.flatnonzero(pres[:wn] == 0)
        if verify:
            rows = rows[rows >= k]
        out.append(tuple(sorted({int(v) // k for v in rows})))
    return out


def _subsets(lo, hi):
    return [s for r in range(hi - lo + 1) for s in itertools.combinations(range(lo, hi), r)]


def _report(tag, marked, want):
    """Prints the marked sets reached and asserts they are `want` (in any order, repeats allowed)."""
    def show(s):
        return "{" + ",".join(map(str, s)) + "}" if len(s) <= 16 else \
            "{" + ",".join(map(str, s[:3])) + ",..," + str(s[-1]) + f": {len(s)} segments" + "}"

    got = sorted(set(marked))
    text = " ".join(show(s) for s in got) if len(got) <= 40 else \
        f"{len(got)} sets, sizes {sorted({len(s) for s in got})}, bitmasks {[sum(1 << q for q in s) for s in got]}"
    print(f"{tag}: marked-segment sets reached: {text}")
    assert got == sorted(set(tuple(s) for s in want)), tag


# ------------------------------------------------- 1. every segment subset ----
def _restore_sweep_case(oracle, k, ratio, wn, sl):
    """Every subset of the segments below wanted_n, then one undecodable payload."""
    n = ratio * k
    p = npa.CodeParams(n, k, wn)
    rng = np.random.default_rng(7000 + 10 * n + k + wn + sl)
    subsets = _subsets(0, _live_segments(k, wn))
    pats = [_restore_payload(rng, n, k, wn, sl, s, b, above=b % 3 if wn < n else 0) for b, s in enumerate(subsets)]
    pats.append(_undecodable(rng, n, k, wn, sl, False))
    return p, pats, subsets, expected_rows(oracle, p, sl, pats)


def _verify_sweep_case(oracle, k, ratio, wn, sl):
    """Every subset of the parity segments below wanted_n; the empty one once
    decodable and once not."""
    n = ratio * k
    p = npa.CodeParams(n, k, wn)
    rng = np.random.default_rng(8000 + 10 * n + k + wn + sl)
    subsets = _subsets(1, _live_segments(k, wn))
    code = _codeword(oracle, rng, n, k, n, sl)
    pats = [_verify_payload(rng, code, n, k, wn, sl, s, b, above=b % 3 if wn < n else 0)
            for b, s in enumerate(subsets)]
    pats.append(_undecodable(rng, n, k, wn, sl, True))
    return p, pats, subsets, expected_case(oracle, p, sl, pats)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("k", KS)
def test_sweep_restore_subsets(gpu, oracle, k, ratio):
    p, pats, subsets, exp = _restore_sweep_case(oracle, k, ratio, ratio * k, SL_TAIL)
    _report(f"restore n{ratio * k} k{k}", _marked(pats, k, p.wanted_n, False), subsets)
    assert len(subsets) == 2 ** ratio and exp[-1] is None and all(e is not None for e in exp[:-1])
    run_restore(gpu, oracle, p, SL_TAIL, pats, expected=exp)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("k", KS)
def test_sweep_verify_subsets(gpu, oracle, k, ratio):
    p, pats, subsets, exp = _verify_sweep_case(oracle, k, ratio, ratio * k, SL_TAIL)
    _report(f"verify n{ratio * k} k{k}", _marked(pats, k, p.wanted_n, True), subsets)
    assert len(subsets) == 2 ** (ratio - 1) and exp[1][-1] == 0xFFFFFFFF and exp[1][0] == 0
    run_verify(gpu, p, SL_TAIL, pats, exp, SWEEP_VARIANTS, label=f"n{ratio * k} k{k}")


def _truncated(k):
    """n = 8k, wanted_n inside the second-to-last segment and off a 16-row boundary."""
    wn = 8 * k - k - k // 2 - 3
    assert 6 * k < wn < 7 * k and wn % 16
    return wn


@pytest.mark.parametrize("k", KS)
def test_sweep_restore_truncated(gpu, oracle, k):
    """Rows at and above wanted_n are absent in a third of the payloads, present
    in a third and random in the others: the decode reads the present ones, and
    none is written."""
    wn = _truncated(k)
    p, pats, subsets, exp = _restore_sweep_case(oracle, k, 8, wn, SL_TAIL)
    _report(f"restore n{8 * k} k{k} wanted_n {wn}", _marked(pats, k, wn, False), subsets)
    assert len(subsets) == 128
    run_restore(gpu, oracle, p, SL_TAIL, pats, expected=exp)


@pytest.mark.parametrize("k", KS)
def test_sweep_verify_truncated(gpu, oracle, k):
    """As test_sweep_restore_truncated: present rows at and above wanted_n feed
    the decode and are not compared."""
    wn = _truncated(k)
    p, pats, subsets, exp = _verify_sweep_case(oracle, k, 8, wn, SL_TAIL)
    _report(f"verify n{8 * k} k{k} wanted_n {wn}", _marked(pats, k, wn, True), subsets)
    assert len(subsets) == 64
    run_verify(gpu, p, SL_TAIL, pats, exp, SWEEP_VARIANTS, label=f"n{8 * k} k{k} wanted_n {wn}")


def _selected(lo, nseg):
    """Every single segment, every adjacent pair, {1,3}, {2,3}, {0,2}, {0,3} and all of lo..nseg-1."""
    sets = [(q,) for q in range(lo, nseg)] + [(q, q + 1) for q in range(lo, nseg - 1)]
    sets += [s for s in ((1, 3), (2, 3), (0, 2), (0, 3)) if s[0] >= lo and s[1] < nseg]
    sets.append(tuple(range(lo, nseg)))
    return list(dict.fromkeys(sets))


def _padded(count):
    """(a multiple of 8 that is not one of 16, a multiple of 16), both >= count."""
    b16 = (count + 15) // 16 * 16
    b8 = (count + 7) // 8 * 8
    return (b8 if b8 % 16 else b16 + 8), b16


def _restore_tiles_case(oracle, k, ratio, sl):
    n = ratio * k
    p = npa.CodeParams(n, k, n)
    rng = np.random.default_rng(9000 + 10 * n + k + sl)
    sets = _selected(0, ratio)
    pats = [_restore_payload(rng, n, k, n, sl, sets[b % len(sets)], b) for b in range(max(_padded(len(sets))))]
    return p, pats, sets, expected_rows(oracle, p, sl, pats)


def _verify_tiles_case(oracle, k, ratio, sl):
    n = ratio * k
    p = npa.CodeParams(n, k, n)
    rng = np.random.default_rng(9500 + 10 * n + k + sl)
    sets = _selected(1, ratio)
    code = _codeword(oracle, rng, n, k, n, sl)
    count = max(_padded(len(sets)))
    # the second pass over the sets (other row counts, drops and flips) compares whole segments
    pats = [_verify_payload(rng, code, n, k, n, sl, sets[b % len(sets)], b,
                            whole=(lambda q: True) if b >= len(sets) else None) for b in range(count)]
    # altered rows with a fixed answer, in positions 8..15 of their 16-row group, altered in the full tile
    high = [v for _, rows, _, exact in pats for v in (exact or [])
            if v % 16 >= 8 and np.flatnonzero(rows[v] != code[v])[0] < 512]
    assert high, "no such row"
    return p, pats, sets, expected_case(oracle, p, sl, pats)


@pytest.mark.parametrize("sl", [SL_TWO, SL_STREAM])
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("k", KS)
def test_sweep_restore_tiles(gpu, oracle, k, ratio, sl):
    """Batches of a multiple of 8 and of 16 payloads (the tile order that keeps
    a payload on one XCD) over the selected sets, cycled to fill the batch.
    SL_TWO: two tiles per payload, rows at 4- and at 2-mod-4 addresses;
    SL_STREAM: base, stride and shard length multiples of 128."""
    p, pats, sets, exp = _restore_tiles_case(oracle, k, ratio, sl)
    _report(f"restore n{ratio * k} k{k} shard_len {sl}", _marked(pats, k, p.wanted_n, False), sets)
    b8, b16 = _padded(len(sets))
    assert b8 % 16 == 8 and b16 % 16 == 0 and min(b8, b16) >= len(sets)
    geo = ((128, 128), (0, 0)) if sl == SL_STREAM else ((0, 64), (2, 2))
    for batch, (offset, slack) in zip((b8, b16), geo):
        run_restore(gpu, oracle, p, sl, pats[:batch], offset, slack, expected=exp[:batch])


@pytest.mark.parametrize("sl", [SL_TWO, SL_STREAM])
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("k", KS)
def test_sweep_verify_tiles(gpu, oracle, k, ratio, sl):
    """As test_sweep_restore_tiles.  With every systematic row present exactly
    the altered rows mismatch, among them rows in positions 8..15 of their
    16-row group whose altered symbol lies in a full tile."""
    p, pats, sets, exp = _verify_tiles_case(oracle, k, ratio, sl)
    _report(f"verify n{ratio * k} k{k} shard_len {sl}", _marked(pats, k, p.wanted_n, True), sets)
    b8, b16 = _padded(len(sets))
    geo = ((128, 128), (0, 0)) if sl == SL_STREAM else ((0, 64), (2, 2))
    for batch, (offset, slack) in zip((b8, b16), geo):
        flags, counts, status = exp
        run_verify(gpu, p, sl, pats[:batch], (flags[:batch], counts[:batch], status[:batch]),
                   ((offset, slack, True, True), (offset, slack, False, False)),
                   label=f"n{ratio * k} k{k} shard_len {sl} batch {batch}")


# -------------------------------------------------- 2. wide codes, n / k >= 16 ----
# (n, k, wanted_n, shard_len)
WIDE = [(1024, 64, 1024, SL_TAIL), (1024, 64, 1024, SL_TWO), (2048, 64, 2000, SL_TAIL), (4096, 64, 4096, SL_TAIL),
        (4096, 128, 3996, SL_TAIL), (8192, 128, 8192, SL_TAIL), (8192, 256, 8192, SL_TAIL),
        (16384, 256, 16084, SL_TAIL)]
WIDEST = (65536, 64, 65536, 6)  # 1024 segments: 32 plan words of segment bits


def _wide_sets(n, k, wn):
    """The marked sets of the wide shapes: {1}, {31}, {32}, {31, 32}, {33}, the
    last segment below wanted_n, every fifth segment and all of them, where
    they exist; then () for the payload that has rows to restore / to compare
    at and above wanted_n only (a whole segment where n - wanted_n >= k, else
    the rest of the partial one; nothing when wanted_n = n)."""
    live = _live_segments(k, wn)
    sets = [(1,), (31,), (32,), (31, 32), (33,), (live - 1,), tuple(range(0, live, 5)), tuple(range(live))]
    return [s for s in dict.fromkeys(sets) if max(s) < live] + [()]


def _wide_restore(n, k, wn, sl, sets, extras=True):
    p = npa.CodeParams(n, k, wn)
    rng = np.random.default_rng(11000 + n + k + wn + sl)
    # rows at and above wanted_n: present (the decode reads them) but for the () payload, where
    # they are the only absent rows and nothing may be written
    pats = [_restore_payload(rng, n, k, wn, sl, s, b, above=1 if s else 0) for b, s in enumerate(sets)]
    if extras:
        pres = np.zeros(n, np.uint8)
        pres[rng.choice(wn, k, replace=False)] = 1
        pats.append(("random-exactly-k", rng.integers(0, 256, (n, sl), dtype=np.uint8), pres))
        pats.append(_undecodable(rng, n, k, wn, sl, False))
    return p, pats


def _wide_verify(oracle, n, k, wn, sl, sets, extras=True):
    p = npa.CodeParams(n, k, wn)
    rng = np.random.default_rng(12000 + n + k + wn + sl)
    code = _codeword(oracle, rng, n, k, n, sl)
    pats = []
    for b, s in enumerate(sets):
        # segment 0 is never marked.  Every fourth payload drops systematic rows (an odd number to
        # _verify_payload); the others keep them, so that their answers are fixed.  Rows at and above
        # wanted_n are present in every second payload and in the () one, where they are the only
        # present parity rows and nothing may be compared.
        pats.append(_verify_payload(rng, code, n, k, wn, sl, [q for q in s if q], 2 * b + (b % 4 == 3),
                                    above=b % 2 if s else 1, whole=(lambda q: q % 7 == 3) if len(s) > 8 else None,
                                    flips=1 + b % 2))
    if extras:
        pres = np.zeros(n, np.uint8)
        pres[rng.choice(wn, k, replace=False)] = 1
        pats.append(("random-exactly-k", rng.integers(0, 256, (n, sl), dtype=np.uint8), pres, []))
        pats.append(_undecodable(rng, n, k, wn, sl, True))
        pres = np.zeros(n, np.uint8)
        pres[:wn] = 1
        pats.append(("all-present", code, pres, []))
    return p, pats


@pytest.mark.parametrize("n,k,wn,sl", WIDE)
def test_wide_restore(gpu, oracle, n, k, wn, sl):
    sets = _wide_sets(n, k, wn)
    p, pats = _wide_restore(n, k, wn, sl, sets)
    marked = _marked(pats, k, wn, False)
    # (the payload with exactly k present rows has absences all over; the undecodable one marks nothing)
    _report(f"restore n{n} k{k} wanted_n {wn} shard_len {sl}", marked, sets + [marked[-2]])
    assert len(marked[-2]) >= 2
    run_restore(gpu, oracle, p, sl, pats, offset=2, slack=2)


@pytest.mark.parametrize("n,k,wn,sl", WIDE)
def test_wide_verify(gpu, oracle, n, k, wn, sl):
    sets = _wide_sets(n, k, wn)
    p, pats = _wide_verify(oracle, n, k, wn, sl, sets)
    marked = _marked(pats, k, wn, True)
    _report(f"verify n{n} k{k} wanted_n {wn} shard_len {sl}", marked,
            [tuple(q for q in s if q) for s in sets] + [marked[-3], tuple(range(1, _live_segments(k, wn)))])
    run_verify(gpu, p, sl, pats, expected_case(oracle, p, sl, pats), SWEEP_VARIANTS,
               label=f"n{n} k{k} wanted_n {wn} shard_len {sl}")


def _widest_sets():
    n, k, wn, _ = WIDEST
    nseg = n // k
    return [(1, nseg - 1), tuple(sorted({31, 32, 33} | set(range(0, nseg, 5)))), tuple(range(nseg))]


def test_wide_restore_1024_segments(gpu, oracle):
    """n / k = 1024, batch 3: segments {1, 1023} (31 empty words between them),
    {31, 32, 33} with every fifth segment (every word), and all segments."""
    n, k, wn, sl = WIDEST
    sets = _widest_sets()
    p, pats = _wide_restore(n, k, wn, sl, sets, extras=False)
    _report(f"restore n{n} k{k}", _marked(pats, k, wn, False), sets)
    run_restore(gpu, oracle, p, sl, pats)


def test_wide_verify_1024_segments(gpu, oracle):
    n, k, wn, sl = WIDEST
    sets = _widest_sets()
    p, pats = _wide_verify(oracle, n, k, wn, sl, sets, extras=False)
    _report(f"verify n{n} k{k}", _marked(pats, k, wn, True), [tuple(q for q in s if q) for s in sets])
    run_verify(gpu, p, sl, pats, expected_case(oracle, p, sl, pats), SWEEP_VARIANTS, label=f"n{n} k{k}")


def _host_received(n, rows, absent):
    pres = np.ones(n, bool)
    pres[absent] = False
    return [rows[v].tobytes() if pres[v] else None for v in range(n)]


def test_wide_host_restore(gpu, oracle):
    """ReedSolomon(4096, 64, 4096).restore_shards on random bytes with absent
    rows in segments 0, 1, 31, 32, 33 and 63."""
    n, k, sl = 4096, 64, SL_TAIL
    rng = np.random.default_rng(4096 + 64)
    rows = rng.integers(0, 256, (n, sl), dtype=np.uint8)
    absent = [5, 64, 127, 31 * 64 + 17, 32 * 64, 33 * 64 + 63, 63 * 64 + 40, n - 1]
    recv = _host_received(n, rows, absent)
    st, pay = oracle.reconstruct(recv, n, k)
    assert st == 0
    st, enc = oracle.encode(pay, n, k, n)
    assert st == 0
    want = [enc[v] if recv[v] is None else recv[v] for v in range(n)]
    got = npa.ReedSolomon(n, k, n, ctx=gpu).restore_shards(recv)
    assert [v for v in range(n) if got[v] != want[v]] == []


def test_wide_host_verify(gpu, oracle):
    """ReedSolomon(4096, 64, 4096).verify / mismatched_shards: a codeword, then
    one bit altered in rows of segments 1, 31, 32 and 63 (every systematic row
    present: exactly those rows), then random bytes."""
    n, k, sl = 4096, 64, SL_TAIL
    rng = np.random.default_rng(4096 + 64 + 1)
    code = _codeword(oracle, rng, n, k, n, sl)
    absent = [70, 31 * 64 + 1, 32 * 64 + 9, 40 * 64, n - 2]
    rs = npa.ReedSolomon(n, k, n, ctx=gpu)

    def mismatching(received):
        st, pay = oracle.reconstruct(received, n, k)
        assert st == 0
        st, enc = oracle.encode(pay, n, k, n)
        assert st == 0
        return [v for v in range(n) if received[v] is not None and received[v] != enc[v]]

    recv = _host_received(n, code, absent)
    assert mismatching(recv) == [] and rs.verify(recv) is True and rs.mismatched_shards(recv) == []
    bad = code.copy()
    altered = [64 + 15, 31 * 64 + 63, 32 * 64, 63 * 64 + 8]
    for v in altered:
        _flip(bad, v, int(rng.integers(0, sl // 2)), rng)
    recv = _host_received(n, bad, absent)
    assert mismatching(recv) == altered
    assert rs.verify(recv) is False and rs.mismatched_shards(recv) == altered
    recv = _host_received(n, rng.integers(0, 256, (n, sl), dtype=np.uint8), absent + list(range(3, 40)))
    want = mismatching(recv)
    assert len(want) > n // 2 and min(want) >= k
    assert rs.verify(recv) is False and rs.mismatched_shards(recv) == want

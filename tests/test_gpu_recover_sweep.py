"""The recover encode of np_recover_batch_dev (kernels_fast_planned.hip k_encode_recover
with the RecoverRows sink, fed by kernels_restore.hip k_recover_plan) over what
is new in it: the split of a wave's 16 rows into rows to store and rows to
compare, a wanted_n anywhere from 0 to n with rows present at and above it,
the wide codes n / k in {16, 32, 64, 1024} whose second row-word array sits
behind more than one segment word, and d_out at odd addresses and strides.

With the restore and the verify requested every row in [k, wanted_n) of a
decodable payload is in the plan's union -- stored when absent, compared when
present -- so every segment 1 .. ceil(wanted_n / k) - 1 is marked and the
segment-subset sweep of test_gpu_masked_sweep.py has nothing to vary here.
What varies is (a) whether segment 0 is marked (an absent systematic row below
wanted_n), (b) the number of live segments, (c) per 16-row group the split of
its mask, (d) undecodable payloads, which mark nothing, and (e) the plan array
a word index lands in.

Every comparison is byte for byte against the oracle's reconstruct and
encode(reconstruct(received)) through run_recover of test_gpu_recover.py.
Absent rows hold its fill byte: a compare of an absent row or a store into a
present one shows in the counts, the map or the shard buffer.  The presence
maps are built without the oracle (the *_layouts functions);
tests/test_recover_sweep_cpu.py checks what they reach on any machine."""
import numpy as np
import pytest

import novelpoly_amd as npa
from test_gpu_masked_sweep import (KS, RATIOS, SL_TAIL, SL_TWO, WIDE, WIDEST, _above, _host_received, _pick_rows,
                                   _wide_sets, _widest_sets)
from test_gpu_recover import COMBOS, UNDECODABLE, expected_recover, run_recover
from test_gpu_verify import _codeword, _flip

pytestmark = pytest.mark.gpu

ALL = (True, True, True)    # (d_out, restore, verify)
BOTH = (False, True, True)  # restore and verify from the payload scratch

# ------------------------------------------------------ 1. row-group classes ----
# What the 16 rows of one wave and pass do: the rows of `stores` are absent
# (stored), the others present (compared).
CLASSES = ("all-store", "all-compare", "bit0", "bit15", "0x5555", "0xaaaa")
MIXED = CLASSES[2:]


def _class_stores(cls, width=16):
    """The store bits of a group of class `cls` with `width` rows below
    wanted_n: "bit15" is the group's last such row."""
    full = (1 << width) - 1
    return {"all-store": full, "all-compare": 0, "bit0": 1, "bit15": 1 << (width - 1), "0x5555": 0x5555 & full,
            "0xaaaa": 0xAAAA & full}[cls]


def group_tail(n, k):
    """wanted_n 8 rows into a group of the last segment."""
    return (n // k - 1) * k + 40


def _group_layout(rng, n, k, wn, b):
    """Payload b of the row-group sweep: (name, present n, rows to alter).
    Group j of [k, wanted_n) has class b + j (even b) or b - j (odd b) mod 6, so
    that all-store / all-compare share a row word in both orders; the group that
    wanted_n cuts has the class restricted to its rows below wanted_n.  Rows at
    and above wanted_n are present for even b and random for odd b.  Segment 0:
    no absent row, rows 0 and k - 1, or one row in each of three groups."""
    pres = np.ones(n, np.uint8)
    _above(rng, pres, wn, 1 if b % 2 == 0 else 2)
    groups = []
    for j, row0 in enumerate(range(k, wn, 16)):
        width = min(16, wn - row0)
        cls = CLASSES[((b + j) if b % 2 == 0 else (b - j)) % 6]
        stores = _class_stores(cls, width)
        for pos in range(width):
            if (stores >> pos) & 1:
                pres[row0 + pos] = 0
        groups.append((row0, width, cls, stores))
    if b % 3 == 1:
        pres[[0, k - 1]] = 0
    elif b % 3 == 2:
        pres[_pick_rows(rng, 0, k, 3, 0)] = 0
    # one altered row beside a stored row of a mixed group ...
    mixed = [g for g in groups if g[2] in MIXED and g[1] >= 2]
    row0, width, cls, stores = mixed[int(rng.integers(0, len(mixed)))]
    pos = int(rng.choice([q for q in range(width) if (stores >> q) & 1]))
    beside = pos + 1 if pos + 1 < width and not (stores >> (pos + 1)) & 1 else pos - 1
    assert 0 <= beside < width and not (stores >> beside) & 1
    flips = [row0 + beside]
    # ... and one in an all-compare group (where the payload has none: another compared row of another group)
    plain = [g for g in groups if g[2] == "all-compare"]
    if plain:
        g = plain[int(rng.integers(0, len(plain)))]
        flips.append(g[0] + int(rng.integers(0, g[1])))
    else:
        other = [g[0] + q for g in groups if g[0] != row0 for q in range(g[1]) if not (g[3] >> q) & 1]
        flips.append(int(rng.choice(other)))
    assert all(pres[v] and k <= v < wn for v in flips) and flips[0] != flips[1]
    return f"groups-{b}-segment0-{('none', 'ends', 'three')[b % 3]}", pres, flips


def group_layouts(n, k, wn):
    """The batch of 9 of one row-group shape (its first 8 are the batch of 8):
    six class payloads, k - 1 present rows, exactly k present rows of random
    bytes, a seventh class payload.  [(name, present, rows to alter or None for
    random bytes)], built from the shape alone."""
    rng = np.random.default_rng(21000 + 10 * n + k + wn)
    lay = [_group_layout(rng, n, k, wn, b) for b in range(6)]
    for name, count in (("k-1", k - 1), ("exactly-k", k)):
        pres = np.zeros(n, np.uint8)
        pres[rng.choice(wn, count, replace=False)] = 1
        lay.append((name, pres, None))
    lay.append(_group_layout(rng, n, k, wn, 6))
    return lay


def group_reach(layouts, k, wn):
    """From the presence maps alone: the (class, half of the row word) pairs of
    the whole groups in [k, wanted_n) of the decodable payloads, the (lower,
    upper) class pairs of their row words, the classes of the group that
    wanted_n cuts, and the segment-0 states (absent systematic rows or none)."""
    pairs, words, cut, seg0 = set(), set(), set(), set()
    for name, pres, _ in layouts:
        if int(pres.sum()) < k:
            continue
        seg0.add(bool((pres[:min(k, wn)] == 0).any()))
        classes = {}
        for row0 in range(k, wn, 16):
            width = min(16, wn - row0)
            stores = sum(1 << q for q in range(width) if not pres[row0 + q])
            cls = next((c for c in CLASSES if _class_stores(c, width) == stores), None)
            if cls is None:
                continue
            if width == 16:
                classes[row0] = cls
                pairs.add((cls, (row0 >> 4) & 1))
            else:
                cut.add(cls)
        words |= {(classes[r], classes[r + 16]) for r in classes if r % 32 == 0 and r + 16 in classes}
    return pairs, words, cut, seg0


def _rows_of(oracle, rng, n, k, sl, layouts, pick_sym):
    """The received bytes of `layouts`: a codeword (all n rows of it) with one
    symbol of each row to alter changed, or random bytes."""
    code = _codeword(oracle, rng, n, k, n, sl)
    pats = []
    for b, (name, pres, flips) in enumerate(layouts):
        if flips is None:
            pats.append((name, rng.integers(0, 256, (n, sl), dtype=np.uint8), pres))
            continue
        rows = code.copy()
        for i, v in enumerate(flips):
            _flip(rows, int(v), pick_sym(b + i), rng)
        pats.append((name, rows, pres))
    return pats


def _syms(sl):
    """Symbols 0, 255 (the full tile's last), 256 (the partial tile's first) and the last, as far as they exist."""
    syms = sl // 2
    return [0, min(255, syms - 1), min(256, syms - 1), syms - 1]


GROUP_VARIANTS = [(ALL, True, True), (ALL, False, False), (BOTH, True, True), ((True, True, False), True, False),
                  ((True, False, True), True, True)]


@pytest.mark.parametrize("tail", [False, True], ids=["whole", "tail"])
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("k", KS)
def test_recover_row_groups(gpu, oracle, k, ratio, tail):
    """All six classes in both halves of a row word, at two shard lengths and
    in a batch of 8 (d_out at offset 0, out_stride the payload length) and of 9
    (d_out at an odd address, out_stride the payload length + 3)."""
    n = ratio * k
    wn = group_tail(n, k) if tail else n
    p = npa.CodeParams(n, k, wn)
    layouts = group_layouts(n, k, wn)
    pairs, words, cut, seg0 = group_reach(layouts[:8], k, wn)
    print(f"n{n} k{k} wanted_n {wn}: (class, half) reached by the batch of 8: {sorted(pairs)}; row words: "
          f"{sorted(words)}; the cut group: {sorted(cut)}; segment 0 marked: {sorted(seg0)}")
    assert pairs >= {(c, h) for c in CLASSES for h in (0, 1)}
    assert {("all-store", "all-compare"), ("all-compare", "all-store")} <= words
    assert seg0 == {False, True} and (cut >= set(CLASSES) if wn % 16 else not cut)
    for sl in (SL_TAIL, SL_TWO):
        rng = np.random.default_rng(22000 + 10 * n + k + wn + sl)
        picks = _syms(sl)
        pats = _rows_of(oracle, rng, n, k, sl, layouts, lambda i: picks[i % 4])
        exp = expected_recover(oracle, p, sl, pats)
        rows, (flags, counts, status), pays = exp
        for b, (name, _, flips) in enumerate(layouts):
            if flips is not None and name.endswith("none"):  # every systematic row present: exactly the altered rows
                assert np.flatnonzero(flags[b]).tolist() == sorted(flips), name
        assert counts[6] == UNDECODABLE and counts[7] == 0 and rows[7]
        for batch, out_offset, out_slack in ((8, 0, 0), (9, 1, 3)):
            part = (rows[:batch], (flags[:batch], counts[:batch], status[:batch]), pays[:batch])
            run_recover(gpu, p, sl, pats[:batch], part, label=f"n{n} k{k} wanted_n {wn} shard_len {sl} batch {batch}",
                        out_offset=out_offset, out_slack=out_slack, variants=GROUP_VARIANTS)


# ------------------------------------------------------- 2. wanted_n edges ----
EDGE_SHAPES = [(1024, 256), (512, 64), (256, 128)]
EDGES = [(n, k, wn) for n, k in EDGE_SHAPES
         for wn in dict.fromkeys(min(w, n) for w in (0, 1, k - 1, k, k + 1, k + 15, k + 16, k + 17, 2 * k - 1, 2 * k,
                                                    2 * k + 1, n - 1, n))]


def edge_layouts(n, k, wn):
    """Four payloads, [(name, present, rows to alter or None for random bytes)]:
    random bytes with rows at and above wanted_n present at random (three in
    four, row n - 1 absent, row wanted_n present where that is another row) and
    random absences below it, two of them systematic where they fit;
    a codeword with every row at and above wanted_n present, absences below it
    and one altered present row in [k, wanted_n); exactly k present rows of all
    n; k - 1."""
    rng = np.random.default_rng(23000 + 10 * n + k + wn)
    lay = []
    pres = np.ones(n, np.uint8)
    pres[wn:] = rng.random(n - wn) < 0.75
    if wn < n:  # an absent row at or above wanted_n (never stored) in every case, and a present one where two fit
        pres[n - 1] = 0
        if wn < n - 1:
            pres[wn] = 1
    count = max(0, min(int(pres.sum()) - k - 1, wn, int(rng.integers(2, (n - k) // 2 + 1))))
    absent = set(rng.choice(min(k, wn), min(2, count), replace=False).tolist()) if count else set()
    while len(absent) < count:
        absent.add(int(rng.integers(0, wn)))
    pres[sorted(absent)] = 0
    lay.append(("random", pres, None))
    pres = np.ones(n, np.uint8)
    flips = [int(rng.integers(k, wn))] if wn > k else []
    below = np.setdiff1d(np.arange(wn), flips)
    pres[rng.choice(below, min(below.size, (n - k) // 2), replace=False)] = 0
    lay.append(("codeword", pres, flips))
    for name, count in (("exactly-k", k), ("k-1", k - 1)):
        pres = np.zeros(n, np.uint8)
        pres[rng.choice(n, count, replace=False)] = 1
        lay.append((name, pres, None))
    return lay


@pytest.mark.parametrize("n,k,wn", EDGES)
def test_recover_wanted_n_edges(gpu, oracle, n, k, wn):
    """launch_recover's own gating (the restore runs for wanted_n > 0, the
    verify for wanted_n > k, both on the recover plan) and the plan's use of
    [k, wanted_n): a present row at or above wanted_n feeds the decode and is
    neither stored nor compared.  All seven requests, with and without d_status
    and d_mismatch."""
    sl = SL_TWO
    p = npa.CodeParams(n, k, wn)
    layouts = edge_layouts(n, k, wn)
    rng = np.random.default_rng(24000 + 10 * n + k + wn)
    picks = _syms(sl)
    pats = _rows_of(oracle, rng, n, k, sl, layouts, lambda i: picks[(i + wn) % 4])
    exp = expected_recover(oracle, p, sl, pats)
    rows, (flags, counts, status), pays = exp
    assert rows[3] is None and counts[3] == UNDECODABLE and pays[1] is not None and pays[2] is not None
    assert sum(int(pr[wn:].sum()) for _, pr, _ in layouts) > 0 or wn == n
    assert wn == n or (rows[0] is not None and not layouts[0][1][n - 1])  # decodable, with an absent row >= wanted_n
    decodable = [b for b in range(4) if rows[b] is not None]
    print(f"n{n} k{k} wanted_n {wn}: present {[int(pr.sum()) for _, pr, _ in layouts]}, of them at and above wanted_n "
          f"{[int(pr[wn:].sum()) for _, pr, _ in layouts]}, restored {[len(rows[b]) for b in decodable]}, "
          f"counts {counts.tolist()}")
    if wn == 0:  # no byte of the shard buffer changes
        assert all(rows[b] == {} for b in decodable)
    if wn <= k:  # nothing to compare, and only systematic rows are restored
        assert all(counts[b] == 0 and not flags[b].any() and all(v < k for v in rows[b]) for b in decodable)
        assert wn == 0 or any(rows[b] for b in decodable)
    else:
        assert all(max(rows[b], default=0) < wn for b in decodable) and any(rows[b] for b in decodable)
    run_recover(gpu, p, sl, pats, exp, combos=COMBOS, label=f"n{n} k{k} wanted_n {wn}", out_offset=wn % 2, out_slack=3)


# ------------------------------------------------ 3. wide codes, n / k >= 16 ----
PREFERRED = (31, 32, 33)
WIDE_VARIANTS = [(ALL, True, True), (BOTH, True, True), (ALL, False, False), (BOTH, False, False)]


def wide_layouts(n, k, wn, sets, extras=True):
    """One payload per set of `sets`: the segments that hold absent rows (1-3
    each); every other row below wanted_n is present, rows at and above it too
    but for the () payload, where they are the only absent rows and nothing may
    be written.  One altered row in a parity segment that also stores and one
    in a parity segment that does not (31, 32, 33 first), where the set leaves
    such segments.  extras: exactly k and k - 1 present rows of random bytes."""
    rng = np.random.default_rng(25000 + n + k + wn)
    live = (wn + k - 1) // k
    lay = []
    for b, s in enumerate(sets):
        pres = np.ones(n, np.uint8)
        _above(rng, pres, wn, 1 if s else 0)
        for q in s:
            pres[_pick_rows(rng, q * k, min((q + 1) * k, wn), 1 + (b + q) % 3, (b + q) % 4)] = 0
        storing = sorted((q for q in s if q >= 1), key=lambda q: (q not in PREFERRED, q))
        plain = sorted((q for q in range(1, live) if q not in s), key=lambda q: (q not in PREFERRED, q))
        segs = storing[:1] + plain[:1]
        segs += [q for q in storing[1:] + plain[1:] if q not in segs][: 2 - len(segs)]
        flips = []
        for q in segs:
            cand = q * k + np.flatnonzero(pres[q * k: min((q + 1) * k, wn)])
            flips.append(int(rng.choice(cand)))
        name = "absent-" + ("+".join(map(str, s)) if len(s) <= 8 else f"{len(s)}-segments") + \
            "-flip-" + "+".join(str(v // k) for v in flips)
        lay.append((name, pres, flips))
    if extras:
        for name, count in (("exactly-k", k), ("k-1", k - 1)):
            pres = np.zeros(n, np.uint8)
            pres[rng.choice(wn, count, replace=False)] = 1
            lay.append((name, pres, None))
    return lay


def _run_wide(gpu, oracle, n, k, wn, sl, layouts, offset, slack):
    p = npa.CodeParams(n, k, wn)
    rng = np.random.default_rng(26000 + n + k + wn + sl)
    picks = _syms(sl)
    pats = _rows_of(oracle, rng, n, k, sl, layouts, lambda i: picks[i % 4])
    exp = expected_recover(oracle, p, sl, pats)
    flags, counts = exp[1][0], exp[1][1]
    for b, (name, pres, flips) in enumerate(layouts):
        if flips is not None and pres[:k].all():  # every systematic row present: exactly the altered rows
            assert np.flatnonzero(flags[b]).tolist() == sorted(flips), name
    print(f"n{n} k{k} wanted_n {wn} shard_len {sl}: {[name for name, _, _ in layouts]}, counts {counts.tolist()}")
    run_recover(gpu, p, sl, pats, exp, offset, slack, label=f"n{n} k{k} wanted_n {wn} shard_len {sl}",
                out_offset=1, out_slack=3, variants=WIDE_VARIANTS)


@pytest.mark.parametrize("n,k,wn,sl", WIDE)
def test_recover_wide(gpu, oracle, n, k, wn, sl):
    """n / k in {16, 32, 64}: the stores' row words behind one or two segment
    words, a plan stride of recover_plan_words, and (with d_out) the decode of
    these shapes straight into the caller's buffer, which the encode then reads.
    Without d_status and d_mismatch the status and the flag map are the call's
    own."""
    layouts = wide_layouts(n, k, wn, _wide_sets(n, k, wn))
    assert [name for name, _, _ in layouts[-2:]] == ["exactly-k", "k-1"]
    _run_wide(gpu, oracle, n, k, wn, sl, layouts, 2, 2)


def test_recover_wide_1024_segments(gpu, oracle):
    """n / k = 1024, batch 3: 32 segment words in front of the two row-word arrays."""
    n, k, wn, sl = WIDEST
    _run_wide(gpu, oracle, n, k, wn, sl, wide_layouts(n, k, wn, _widest_sets(), extras=False), 2, 2)


def test_recover_wide_host(gpu, oracle):
    """ReedSolomon(4096, 64, 4096).recover on random bytes with the absent rows
    of test_wide_host_restore: payload, shards and mismatching rows."""
    n, k, sl = 4096, 64, SL_TAIL
    rng = np.random.default_rng(4096 + 64 + 2)
    rows = rng.integers(0, 256, (n, sl), dtype=np.uint8)
    absent = [5, 64, 127, 31 * 64 + 17, 32 * 64, 33 * 64 + 63, 63 * 64 + 40, n - 1]
    recv = _host_received(n, rows, absent)
    st, pay = oracle.reconstruct(recv, n, k)
    assert st == 0
    st, enc = oracle.encode(pay, n, k, n)
    assert st == 0
    want_shards = [enc[v] if recv[v] is None else recv[v] for v in range(n)]
    want_rows = [v for v in range(n) if recv[v] is not None and recv[v] != enc[v]]
    assert len(want_rows) > n // 2 and min(want_rows) >= k
    got = npa.ReedSolomon(n, k, n, ctx=gpu).recover(recv)
    assert got[0] == pay and got[2] == want_rows
    assert [v for v in range(n) if got[1][v] != want_shards[v]] == []

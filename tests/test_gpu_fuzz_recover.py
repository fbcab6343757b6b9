"""Randomised (seeded) np_recover_batch_dev and np_recover_ragged_dev, in the
style of test_gpu_fuzz_masked.py and with its shapes, column counts, offsets,
slacks, wanted_n edges, payload kinds and presence modes (random presence at
and above wanted_n).  Per uniform case in addition one of the seven requests
(restore and verify together in at least half of the cases), d_out 0, 1, 2, 4
or 8 bytes into its buffer and out_stride 0, 1, 3 or 32 bytes above the payload
length.  The ragged cases draw an explicit wanted_n too, 1-9 items with a
column count each, placed out of order with gaps, shard offsets 2 mod 16 or
128-aligned and odd payload offsets: at the direct ragged shapes (k in {64,
128, 256}, n / k in {2, 4, 8}) and at n / k = 16, which runs as uniform calls.
Byte for byte against the oracle's reconstruct and encode(reconstruct(
received)) of every payload or item.

The case plans (everything but the received bytes) are built without the
oracle: tests/test_recover_sweep_cpu.py asserts what they cover."""
import numpy as np
import pytest

import novelpoly_amd as npa
from test_gpu_fuzz_masked import BUDGET, COLUMNS, OFFSETS, SHAPES, SLACKS, _presence, _wanted_n
from test_gpu_ragged import GAPS, _up
from test_gpu_recover import COMBOS, expected_recover, run_recover
from test_gpu_verify import _codeword, _flip

pytestmark = pytest.mark.gpu

SEED = 9100  # the base at which two thirds of the payloads have >= k present rows (test_recover_sweep_cpu.py)
CASES, RAGGED_CASES = 24, 20
OUT_OFFSETS = [0, 1, 2, 4, 8]
OUT_SLACKS = [0, 1, 3, 32]
KINDS = ["codeword", "flipped", "random"]
MODES = ["random", "exactly-k", "k-1", "none-absent", "segments"]
RAGGED_DIRECT = [(r * k, k) for k in (64, 128, 256) for r in (2, 4, 8)]
# n / k = 16 at the three k of the row-masked encodes: there is no fourth such shape, so the first runs twice, with
# the plan (wanted_n, items, request, presence) of another seed
RAGGED_WIDE = [(1024, 64), (2048, 128), (4096, 256), (1024, 64)]


class Plan:
    """One case without its bytes: the code, the geometry, the request and per
    payload (kind, mode, present flags)."""


def _request(rng, case):
    """Even cases restore and verify (with or without d_out), odd ones draw any of the seven."""
    choices = [c for c in COMBOS if c[1] and c[2]] if case % 2 == 0 else COMBOS
    combo = choices[int(rng.integers(0, len(choices)))]
    return tuple(bool(x) for x in combo)


def uniform_plan(case):
    rng = np.random.default_rng(SEED + case)
    pl = Plan()
    pl.case, pl.ragged = case, False
    pl.n, pl.k = SHAPES[case % len(SHAPES)]
    n, k = pl.n, pl.k
    pl.wn = _wanted_n(rng, n, k)
    cols = int(rng.choice(COLUMNS))
    pl.sl = 2 * cols
    pl.offset, pl.slack = int(rng.choice(OFFSETS)), int(rng.choice(SLACKS))
    batch = int(rng.choice(list(range(1, 10)) + [16]))
    batch = max(1, min(batch, BUDGET // (n * cols)))
    pl.combo = _request(rng, case)
    pl.out_offset, pl.out_slack = int(rng.choice(OUT_OFFSETS)), int(rng.choice(OUT_SLACKS))
    pl.payloads = []
    for b in range(batch):
        kind, mode = str(rng.choice(KINDS)), str(rng.choice(MODES))
        pl.payloads.append((kind, mode, _presence(rng, n, k, pl.wn, mode)))
    pl.odd_out = pl.combo[0] and pl.out_offset % 2 == 1
    return pl


def ragged_plan(case):
    """Ragged case `case`: 0..15 at the direct ragged shapes, 16..19 at n / k = 16."""
    rng = np.random.default_rng(SEED + 500 + case)
    pl = Plan()
    pl.case, pl.ragged = case, True
    pl.n, pl.k = RAGGED_DIRECT[case % len(RAGGED_DIRECT)] if case < 16 else RAGGED_WIDE[case - 16]
    n, k = pl.n, pl.k
    pl.wn = _wanted_n(rng, n, k)
    cols = [int(c) for c in rng.choice(COLUMNS, int(rng.integers(1, 10)))]
    while len(cols) > 1 and n * sum(cols) > BUDGET:
        cols.pop()
    pl.cols = cols
    pl.combo = _request(rng, case)
    # placement: another order than the batch's, gaps, shard offsets 2 mod 16 or 128-aligned, odd payload offsets
    poff, soff, place = 1, 0, {}
    for j, i in enumerate(rng.permutation(len(cols)).tolist()):
        sl = 2 * cols[i]
        gap = GAPS[j % 3]
        soff = _up(soff, 128) if sl % 128 == 0 or rng.random() < 0.25 else _up(soff, 16) + 2
        poff |= int(rng.random() < 0.75)
        place[i] = (poff, soff)
        poff += cols[i] * 2 * k + gap
        soff += n * sl + gap
    pl.items = [(place[i][0], cols[i] * 2 * k, place[i][1], 2 * cols[i]) for i in range(len(cols))]
    pl.psize, pl.ssize = poff + 64, soff + 64
    pl.payloads = []
    for _ in cols:
        kind, mode = str(rng.choice(KINDS)), str(rng.choice(MODES))
        pl.payloads.append((kind, mode, _presence(rng, n, k, pl.wn, mode)))
    pl.odd_out = pl.combo[0] and any(it[0] % 2 for it in pl.items)
    return pl


def all_plans():
    return [uniform_plan(c) for c in range(CASES)] + [ragged_plan(c) for c in range(RAGGED_CASES)]


def _bytes(oracle, rng, n, k, sl, kind):
    """The n rows of one payload or item: a codeword, one with 1-3 altered symbols, or random bytes."""
    if kind == "random":
        return rng.integers(0, 256, (n, sl), dtype=np.uint8)
    rows = _codeword(oracle, rng, n, k, n, sl)
    for _ in range(int(rng.integers(1, 4)) if kind == "flipped" else 0):
        _flip(rows, int(rng.integers(0, n)), int(rng.integers(0, sl // 2)), rng)
    return rows


def _describe(pl):
    geo = f"items of {pl.cols} columns" if pl.ragged else \
        f"columns {pl.sl // 2} offset {pl.offset} slack {pl.slack} d_out offset {pl.out_offset} slack {pl.out_slack}"
    return (f"case {pl.case}: n{pl.n} k{pl.k} wanted_n {pl.wn} {geo} request (out, restore, verify) {pl.combo}: "
            + ", ".join(f"{kind}/{mode} ({int(pr.sum())} present, {int(pr[pl.wn:].sum())} at and above wanted_n)"
                        for kind, mode, pr in pl.payloads))


def _variants(combo):
    """With d_status and (where it verifies) d_mismatch, and without both."""
    return [(combo, True, combo[2]), (combo, False, False)]


@pytest.mark.parametrize("case", range(CASES))
def test_fuzz_recover(gpu, oracle, case):
    pl = uniform_plan(case)
    print(_describe(pl))
    rng = np.random.default_rng(SEED + 1000 + case)
    pats = [(f"{kind}/{mode}", _bytes(oracle, rng, pl.n, pl.k, pl.sl, kind), pres) for kind, mode, pres in pl.payloads]
    p = npa.CodeParams(pl.n, pl.k, pl.wn)
    run_recover(gpu, p, pl.sl, pats, expected_recover(oracle, p, pl.sl, pats), pl.offset, pl.slack,
                label=f"case {case}", out_offset=pl.out_offset, out_slack=pl.out_slack, variants=_variants(pl.combo))


class Staged:
    """What _call and _check of test_gpu_ragged_recover.py read of a ragged case, for explicit CodeParams."""

    def __init__(self, pl):
        self.p = npa.CodeParams(pl.n, pl.k, pl.wn)
        self.n, self.k, self.wn, self.cols, self.items = pl.n, pl.k, pl.wn, pl.cols, pl.items
        self.psize, self.ssize = pl.psize, pl.ssize

    def item_rows(self, buf, i):
        _, _, so, sl = self.items[i]
        return buf[so:so + self.n * sl].reshape(self.n, sl)


@pytest.mark.parametrize("case", range(RAGGED_CASES))
def test_fuzz_recover_ragged(gpu, oracle, case):
    from test_gpu_ragged_masked import _dev
    from test_gpu_ragged_recover import _call, _check, expected_items

    pl = ragged_plan(case)
    print(_describe(pl))
    c = Staged(pl)
    rng = np.random.default_rng(SEED + 1500 + case)
    per_item = [(_bytes(oracle, rng, pl.n, pl.k, pl.items[i][3], kind), pres)
                for i, (kind, mode, pres) in enumerate(pl.payloads)]
    e = expected_items(oracle, c, [(kind, mode) for kind, mode, _ in pl.payloads], per_item)
    dbefore, dpres = _dev(e.before), _dev(e.pres)
    for (with_out, restore, verify), with_status, with_map in _variants(pl.combo):
        tag = f"case {case}: out {with_out}, restore {restore}, verify {verify}, status {with_status}, map {with_map}"
        res = _call(gpu, c, dbefore, dpres, with_out, restore, verify, with_status, with_map)
        _check(c, e, res, with_out, restore, verify, with_status, with_map, tag)

"""Randomised (seeded) np_restore_shards_batch_dev / np_verify_shards_batch_dev
at the shapes of the row-masked encodes (k in {64, 128, 256}, n / k in {2, 4,
8, 16, 64}), in the style of test_gpu_fuzz.py: per case a wanted_n from the
edges (0, 1, k - 1, k, k + 1, around a multiple of k or of 16, n - 1, n) or
uniform, a column count around the lane, tile and two-tile boundaries, a base
offset and a stride slack (even: rows at even addresses are what the kernels
document), a batch of 1..9 or 16; per payload a codeword, a codeword with
altered bits or random bytes, and a presence pattern below wanted_n (random,
exactly k, k - 1, nothing absent, whole segments absent) with random presence
at and above it.  Byte for byte against the oracle's
encode(reconstruct(received)) through the runners of test_gpu_restore.py and
test_gpu_verify.py."""
import numpy as np
import pytest

import novelpoly_amd as npa
from test_gpu_restore import run_restore
from test_gpu_verify import _codeword, _flip, expected_case, run_verify

pytestmark = pytest.mark.gpu

SHAPES = [(r * k, k) for k in (64, 128, 256) for r in (2, 4, 8, 16, 64)]
COLUMNS = [1, 3, 4, 5, 255, 256, 257, 260, 513]
OFFSETS = [0, 2, 4, 8, 128]
SLACKS = [0, 2, 6, 64, 128]
# rows x columns x payloads of one case: the oracle takes about 1 s for this many symbols
BUDGET = 8 << 20


def _wanted_n(rng, n, k):
    m, s = int(rng.integers(1, n // k + 1)) * k, int(rng.integers(1, n // 16 + 1)) * 16
    edges = [0, 1, k - 1, k, k + 1, m - 1, min(m + 1, n), s - 1, min(s + 1, n), n - 1, n]
    return int(rng.integers(0, n + 1)) if rng.random() < 0.25 else int(rng.choice(edges))


def _presence(rng, n, k, wn, mode):
    """Present flags: `mode` below wanted_n, random at and above it."""
    pres = np.ones(n, np.uint8)
    pres[wn:] = rng.integers(0, 2, n - wn, dtype=np.uint8)
    above = int(pres[wn:].sum())
    if mode == "random":
        pres[:wn] = rng.integers(0, 2, wn, dtype=np.uint8)
    elif mode in ("exactly-k", "k-1"):  # of all n rows, as far as the rows below wanted_n allow
        keep = min(max(k - (mode == "k-1") - above, 0), wn)
        pres[:wn] = 0
        if keep:
            pres[rng.choice(wn, keep, replace=False)] = 1
    elif mode == "segments":  # whole segments absent
        for q in range((wn + k - 1) // k):
            if rng.random() < 0.4:
                pres[q * k: min((q + 1) * k, wn)] = 0
    return pres


def _case(oracle, case, verify):
    rng = np.random.default_rng((5000 if verify else 3000) + case)
    n, k = SHAPES[case % len(SHAPES)]
    wn = _wanted_n(rng, n, k)
    cols = int(rng.choice(COLUMNS))
    sl = 2 * cols
    offset, slack = int(rng.choice(OFFSETS)), int(rng.choice(SLACKS))
    batch = int(rng.choice(list(range(1, 10)) + [16]))
    batch = max(1, min(batch, BUDGET // (n * cols)))
    pats = []
    for b in range(batch):
        kind = str(rng.choice(["codeword", "flipped", "random"]))
        mode = str(rng.choice(["random", "exactly-k", "k-1", "none-absent", "segments"]))
        pres = _presence(rng, n, k, wn, mode)
        if kind == "random":
            rows = rng.integers(0, 256, (n, sl), dtype=np.uint8)
        else:
            rows = _codeword(oracle, rng, n, k, n, sl)
            for _ in range(int(rng.integers(1, 4)) if kind == "flipped" else 0):
                _flip(rows, int(rng.integers(0, n)), int(rng.integers(0, cols)), rng)
        pats.append((f"{kind}/{mode}", rows, pres))
    print(f"case {case}: n{n} k{k} wanted_n {wn} columns {cols} offset {offset} slack {slack} batch {batch}: "
          + ", ".join(f"{name} ({int(pr.sum())} present)" for name, _, pr in pats))
    return npa.CodeParams(n, k, wn), sl, pats, offset, slack


@pytest.mark.parametrize("case", range(24))
def test_fuzz_restore(gpu, oracle, case):
    p, sl, pats, offset, slack = _case(oracle, case, False)
    run_restore(gpu, oracle, p, sl, pats, offset, slack)


@pytest.mark.parametrize("case", range(24))
def test_fuzz_verify(gpu, oracle, case):
    p, sl, pats, offset, slack = _case(oracle, case, True)
    pats = [(name, rows, pres, None) for name, rows, pres in pats]
    variants = [(offset, slack, True, True), (offset, slack, False, False), (offset, slack, True, False),
                (offset, slack, False, True)][: 2 + case % 3]
    run_verify(gpu, p, sl, pats, expected_case(oracle, p, sl, pats), variants, label=f"case {case}")

"""The kernel families that run only behind a switch, against
the oracle.  The switches are read once per process, so each runs in a child:

  res0   NP_RES=0        k = 512 / 1024 on kernels_big.hip: the six
                         k_reconstruct_big<512|1024, 2|4|8> instances, their
                         k_big_records and the big encode at n / k <= 8
  huge1  NP_HUGE=1       k = 2048 on kernels_huge.hip: the M = 2 instances,
                         NQ in {2, 4, 8} (and the encode at NQ = 16)
  huge0  NP_HUGE=0       k = 4096 .. 16384 on the generic kernels, n up to 65536
  pair0  NP_HUGE_PAIR=0  payloads of <= 32 columns one per tile

A parent test starts `pytest tests/test_gpu_families.py -m gpu` with the
switch and NP_FAMILY_CHILD=<tag> set; the case tests of that tag run there and
every other test of the file skips.  The parent asserts that the child passed
and that it reports exactly the number of case tests registered for the tag
(`case` below counts them), so a skip cannot stand in for a pass.  Each case
first asserts npa.kernel_family for its shape and direction: a switch that the
library ignored fails there instead of passing on the default kernels.
NP_HUGE_PAIR has no such witness -- pairing is a launch geometry inside the
sub-transform family (kernels_huge.hip huge_pair_enabled), which
np_kernel_family does not report; the pair0 cases assert the family and
compare the bytes.

The same four children run a second time on the checked library
(lib/libnovelpoly_hip_chk.so, tests/test_gpu_bounds.py): conftest's
`_bounds_checked` asserts after every case that no global access left its
buffer.

The bodies are those of test_gpu_recover (nine patterns per shape: window,
store + compare segments, systematic rows absent, copy mode, random bytes,
exactly k, k - 1, all present, parity absent), test_gpu_parity and
test_gpu_huge, called with explicit arguments; every expected byte comes from
the oracle.

Children run one after another (the parent and one child hold the GPU).  Once
a child has died -- abort, segmentation fault, a signal, a device fault in its
output, its own or the subprocess time limit -- no further child is started:
the remaining parents fail at once.

Time limits: 120 s per test in the child, as the other children of the suite;
per child five times its first measured run on an MI355X, at least 60 s
(LIMITS).  First measured runs, seconds of the whole child process (start of
python, imports, the oracle's answers and the GPU work): product children
res0 7.6, huge1 9.0, huge0 10.5, pair0 5.4; the checked children that followed
7.8, 8.9, 11.0, 5.9 -- so every limit is the 60 s floor."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import novelpoly_amd as npa
from novelpoly_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHK_LIB = os.path.join(ROOT, "reed-solomon-novelpoly_amd", "lib", "libnovelpoly_hip_chk.so")
FAMILY = os.environ.get("NP_FAMILY_CHILD")
SWITCH = {"res0": ("NP_RES", "0"), "huge1": ("NP_HUGE", "1"), "huge0": ("NP_HUGE", "0"), "pair0": ("NP_HUGE_PAIR", "0")}
BUILDS = ("product", "checked")

# first measured run of each child on an MI355X, seconds
MEASURED = {("res0", "product"): 7.6, ("huge1", "product"): 9.0, ("huge0", "product"): 10.5,
            ("pair0", "product"): 5.4, ("res0", "checked"): 7.8, ("huge1", "checked"): 8.9,
            ("huge0", "checked"): 11.0, ("pair0", "checked"): 5.9}
LIMITS = {key: max(60, int(5 * t + 0.999)) for key, t in MEASURED.items()}

GENERIC, BIG, HUGE, RES = npa.FAMILY_GENERIC, npa.FAMILY_BIG, npa.FAMILY_HUGE, npa.FAMILY_RES
N_CASES = {tag: 0 for tag in SWITCH}


def case(tag, argnames=None, argvalues=None):
    """A case test of child `tag`, parametrised or not: counted, and skipped in every other process."""
    def wrap(f):
        N_CASES[tag] += len(argvalues) if argnames else 1
        if argnames:
            f = pytest.mark.parametrize(argnames, argvalues)(f)
        return pytest.mark.skipif(FAMILY != tag, reason=f"runs in the {tag} child")(f)

    return wrap


def _families(nw, kw, sl):
    """(encode family, reconstruct family) of the derived shape at rows of sl bytes."""
    p = npa.CodeParams.derive_parameters(nw, kw)
    return npa.kernel_family(p, sl, False), npa.kernel_family(p, sl, True)


def _shard_len(nw, kw, plen):
    p = npa.CodeParams.derive_parameters(nw, kw)
    return ((plen + 1) // 2 + p.k() - 1) // p.k() * 2


# (d_out, restore, verify): all three, restore + verify, the payload alone
COMBOS = [(True, True, True), (False, True, True), (True, False, False)]


def _recover_shape(gpu, oracle, nw, kw, sl):
    """test_gpu_recover's shape case (nine patterns, one batch) under three request combinations."""
    from test_gpu_recover import _shape_case, run_recover

    d = npa.CodeParams.derive_parameters(nw, kw)
    p, pats, exp = _shape_case(oracle, d.n(), d.k(), d.wanted_n, sl)
    run_recover(gpu, p, sl, pats, exp, combos=COMBOS, label=f"{nw},{kw}")


def _encode_vs_oracle(gpu, oracle, nw, kw, plen):
    p = npa.CodeParams.derive_parameters(nw, kw)
    pl = synth.payload(nw + kw + plen, plen)
    got = p.make_encoder(gpu).encode(pl)
    st, want = oracle.encode(pl, p.n(), p.k(), nw)
    assert st == 0
    bad = [v for v in range(nw) if got[v] != want[v]]
    assert not bad, f"{len(bad)} shards differ, first {bad[:5]}"


# ------------------------------------------------------------------ res0 ----
# the six big decode instances; wanted_n < n once per k; two column tiles (one
# partial) once per k, one partial tile elsewhere
RES0_RECOVER = [(1024, 512, 2 * 37), (2000, 667, 2 * 300), (4096, 1000, 2 * 37),
                (2048, 1024, 2 * 37), (4000, 1334, 2 * 300), (8192, 2000, 2 * 37)]


# (nothing at import time may load the library: the `gpu` fixture initialises torch's runtime first)
assert sorted((npa.next_higher_power_of_2(nw), npa.next_lower_power_of_2(kw)) for nw, kw, _ in RES0_RECOVER) == \
    sorted((q * k, k) for k in (512, 1024) for q in (2, 4, 8))


@case("res0", "nw,kw,sl", RES0_RECOVER)
def test_res0_recover(gpu, oracle, nw, kw, sl):
    assert _families(nw, kw, sl) == (BIG, BIG)
    _recover_shape(gpu, oracle, nw, kw, sl)


@case("res0", "nw,kw,plen", [(2000, 667, 1024 * 33), (1500, 512, 512 * 40 + 1)])
def test_res0_empty_segments(gpu, oracle, nw, kw, plen):
    """Empty 256-row sub-segments (k_big_records occupancy) and whole segments."""
    from test_gpu_parity import test_reconstruct_empty_segments

    assert _families(nw, kw, _shard_len(nw, kw, plen)) == (BIG, BIG)
    test_reconstruct_empty_segments(gpu, oracle, nw, kw, plen)


@case("res0")
def test_res0_encode_odd_tail(gpu, oracle):
    from test_gpu_parity import test_fast_encode_shapes

    nw, kw, plen = 1024, 512, 1024 * 100 + 3
    assert _families(nw, kw, _shard_len(nw, kw, plen))[0] == BIG
    test_fast_encode_shapes(gpu, oracle, nw, kw, plen)


@case("res0")
def test_res0_systematic_lost(gpu, oracle):
    from test_gpu_parity import test_fast_reconstruct_shapes

    nw, kw, plen = 4096, 1366, 2048 * 40 + 1
    assert _families(nw, kw, _shard_len(nw, kw, plen)) == (BIG, BIG)
    test_fast_reconstruct_shapes(gpu, oracle, nw, kw, plen, -1)


@case("res0")
def test_res0_locator_modes(gpu, oracle):
    """The caller's locators and the device's (k_big_records) at n = 4k, k = 512."""
    from test_gpu_parity import test_device_reconstruct_locator_modes

    nw, kw, plen, batch = 2048, 512, 1024 * 40, 2
    assert _families(nw, kw, _shard_len(nw, kw, plen)) == (BIG, BIG)
    test_device_reconstruct_locator_modes(gpu, oracle, nw, kw, plen, batch)


# ----------------------------------------------------------------- huge1 ----
# k = 2048 at n = 4096, 8192 (wanted_n < n), 16384; 67 columns: a full 64-column tile and 3 columns
@case("huge1", "nw,kw,sl", [(4096, 2048, 2 * 67), (8000, 2667, 2 * 67), (16384, 4000, 2 * 67)])
def test_huge1_recover(gpu, oracle, nw, kw, sl):
    assert npa.CodeParams.derive_parameters(nw, kw).k() == 2048
    assert _families(nw, kw, sl) == (HUGE, HUGE)
    _recover_shape(gpu, oracle, nw, kw, sl)


@case("huge1")
def test_huge1_paired_odd_batch(gpu, oracle):
    """Three payloads of 17 columns: paired tiles, the last one half empty, in
    the encode and in the decode with the caller's and the device's locators."""
    from test_gpu_parity import test_device_reconstruct_locator_modes

    nw, kw, plen, batch = 6000, 2048, 2 * 2048 * 17 - 3, 3
    assert _shard_len(nw, kw, plen) == 2 * 17 and _families(nw, kw, 2 * 17) == (HUGE, HUGE)
    test_device_reconstruct_locator_modes(gpu, oracle, nw, kw, plen, batch)


@case("huge1", "nw,kw,plen,k,fam", [(5000, 1667, 2048 * 40 + 3, 1024, RES), (10000, 3334, 4096 * 40 + 3, 2048, HUGE)])
def test_huge1_empty_blocks(gpu, oracle, nw, kw, plen, k, fam):
    """Whole k-row segments and so whole 1024-row blocks without a present row
    (k_huge_rec_inv skips them).  (5000, 1667) derives k = 1024, which NP_HUGE=1
    leaves on the resident kernels: asserted as the query answers; (10000, 3334)
    is the same case at k = 2048, n = 16384, on the sub-transform kernels."""
    from test_gpu_parity import test_reconstruct_empty_segments

    assert npa.CodeParams.derive_parameters(nw, kw).k() == k
    assert _families(nw, kw, _shard_len(nw, kw, plen)) == (fam, fam)
    test_reconstruct_empty_segments(gpu, oracle, nw, kw, plen)


@case("huge1")
def test_huge1_encode_wide(gpu, oracle):
    """Explicit (32768, 2048): the sub-transform encode takes any n >= 2k
    (n / k = 16), the decode is the generic one."""
    nw, kw, plen = 32768, 2048, 2 * 2048 * 66 + 1
    assert _families(nw, kw, _shard_len(nw, kw, plen)) == (HUGE, GENERIC)
    _encode_vs_oracle(gpu, oracle, nw, kw, plen)


# ----------------------------------------------------------------- huge0 ----
@case("huge0", "nw,kw,sl", [(16384, 5462, 2 * 5), (8192, 4096, 2 * 3), (65536, 21846, 2 * 3)])
def test_huge0_recover(gpu, oracle, nw, kw, sl):
    assert npa.CodeParams.derive_parameters(nw, kw).k() >= 4096
    assert _families(nw, kw, sl) == (GENERIC, GENERIC)
    _recover_shape(gpu, oracle, nw, kw, sl)


@case("huge0", "erase", [13333, -1])
def test_huge0_roundtrip(gpu, oracle, erase):
    """n = 32768, k = 4096: the encode and the reconstruct against the oracle,
    with random erasures and with every systematic row lost."""
    from test_gpu_huge import test_huge_encode, test_huge_reconstruct

    nw, kw, plen = 20000, 6667, 2 * 4096 * 3 + 1
    assert _families(nw, kw, _shard_len(nw, kw, plen)) == (GENERIC, GENERIC)
    test_huge_encode(gpu, oracle, nw, kw, plen)
    test_huge_reconstruct(gpu, oracle, nw, kw, plen, erase)


# ----------------------------------------------------------------- pair0 ----
def _pair_sets():
    from test_gpu_huge import PAIR, PAIR_REC

    # the second and the last set of each list (PAIR has three, PAIR_REC four)
    return [PAIR[1], PAIR[-1]], [PAIR_REC[1], PAIR_REC[3]]


@case("pair0", "i", [0, 1])
def test_pair0_encode_batch(gpu, oracle, i):
    from test_gpu_huge import test_huge_encode_paired_batch

    nw, kw, plen, batch = _pair_sets()[0][i]
    assert _families(nw, kw, _shard_len(nw, kw, plen)) == (HUGE, HUGE)
    test_huge_encode_paired_batch(gpu, oracle, nw, kw, plen, batch)


@case("pair0", "i", [0, 1])
def test_pair0_reconstruct_batch(gpu, oracle, i):
    from test_gpu_huge import test_huge_reconstruct_paired_batch

    nw, kw, plen, kinds = _pair_sets()[1][i]
    assert _families(nw, kw, _shard_len(nw, kw, plen)) == (HUGE, HUGE)
    test_huge_reconstruct_paired_batch(gpu, oracle, nw, kw, plen, kinds)


@case("pair0")
def test_pair0_ragged_recover(gpu, oracle):
    """One np_recover_ragged_dev call over two items of 9 and 17 columns at
    n = 16384, k = 4096 (runs of equally long items: reconstruct, ordinary
    encode, copy and compare): payload, restored rows, flags, counts and
    statuses of each item against the oracle on that item alone; every buffer
    compared whole."""
    import torch

    p = npa.CodeParams.derive_parameters(16000, 5334)
    n, k, wn = p.n(), p.k(), p.wanted_n
    assert (n, k) == (16384, 4096)
    lens = [2 * 9, 2 * 17]
    assert all(_families(16000, 5334, sl) == (HUGE, HUGE) for sl in lens)
    rng = np.random.default_rng(917)
    fill, guard = 0x5A, 0xA5
    gap = 6  # between the items, in both buffers
    soff, poff, s0, p0 = [], [], 2, 1
    for sl in lens:
        soff.append(s0)
        poff.append(p0)
        s0 += n * sl + gap
        p0 += (sl // 2) * 2 * k + gap
    before = np.full(s0, fill, np.uint8)
    pres = np.zeros((2, n), np.uint8)
    want_out = np.full(p0, guard, np.uint8)
    flags = np.zeros((2, n), np.uint8)
    for i, sl in enumerate(lens):
        pay = rng.integers(0, 256, (sl // 2) * 2 * k - 1, dtype=np.uint8).tobytes()  # an odd payload tail
        st, enc = oracle.encode(pay, n, k, wn)
        assert st == 0 and all(len(r) == sl for r in enc)
        rows = np.frombuffer(b"".join(enc), np.uint8).reshape(wn, sl).copy()
        pres[i, :wn] = 1
        pres[i, rng.choice(wn, (wn - k) // (i + 2), replace=False)] = 0
        hit = int(rng.choice(np.flatnonzero(pres[i, k:wn]) + k))  # one present parity row altered
        rows[hit, int(rng.integers(0, sl))] ^= 0x41
        view = before[soff[i]:soff[i] + n * sl].reshape(n, sl)
        view[:wn][pres[i, :wn] != 0] = rows[pres[i, :wn] != 0]
    restored = before.copy()
    counts = []
    for i, sl in enumerate(lens):
        view = before[soff[i]:soff[i] + n * sl].reshape(n, sl)
        recv = [view[v].tobytes() if pres[i, v] else None for v in range(n)]
        st, pay = oracle.reconstruct(recv, n, k)
        assert st == 0 and len(pay) == (sl // 2) * 2 * k
        want_out[poff[i]:poff[i] + len(pay)] = np.frombuffer(pay, np.uint8)
        st, enc = oracle.encode(pay, n, k, wn)
        assert st == 0
        rview = restored[soff[i]:soff[i] + n * sl].reshape(n, sl)
        for v in range(wn):
            if not pres[i, v]:
                rview[v] = np.frombuffer(enc[v], np.uint8)
            elif enc[v] != recv[v]:
                flags[i, v] = 1
        counts.append(int(flags[i].sum()))
    assert all(c > 0 for c in counts), counts  # the verdict is not trivial
    items = [(poff[i], 0, soff[i], lens[i]) for i in range(2)]
    buf = torch.from_numpy(before).cuda()
    dpres = torch.from_numpy(pres).cuda()
    out = torch.full((64 + p0 + 64,), guard, dtype=torch.uint8, device="cuda")
    cnt = torch.full((64 + 8 + 64,), guard, dtype=torch.uint8, device="cuda")
    mp = torch.full((64 + 2 * n + 64,), guard, dtype=torch.uint8, device="cuda")
    st_d = torch.full((2, 2), -1, dtype=torch.int32, device="cuda")
    npa.recover_ragged_dev(p, buf.data_ptr(), s0, dpres.data_ptr(), items, d_out=out.data_ptr() + 64, out_size=p0,
                           restore=True, d_bad_rows=cnt.data_ptr() + 64, d_mismatch=mp.data_ptr() + 64,
                           d_status=st_d.data_ptr(), ctx=gpu, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got, o, c, m, stat = (t.cpu().numpy() for t in (buf, out, cnt, mp, st_d))
    for i, sl in enumerate(lens):
        a, b = got[soff[i]:soff[i] + n * sl].reshape(n, sl), restored[soff[i]:soff[i] + n * sl].reshape(n, sl)
        bad = np.flatnonzero((a != b).any(axis=1))
        assert bad.size == 0, (i, bad.size, bad[:8].tolist())
    assert np.array_equal(got, restored), "shard bytes outside the items"
    for a in (o, c, m):
        assert (a[:64] == guard).all() and (a[-64:] == guard).all()
    for i, sl in enumerate(lens):
        ln = (sl // 2) * 2 * k
        assert np.array_equal(o[64 + poff[i]:64 + poff[i] + ln], want_out[poff[i]:poff[i] + ln]), i
    assert np.array_equal(o[64:-64], want_out), "output bytes outside the items"
    assert c[64:-64].copy().view(np.uint32).tolist() == counts
    assert np.array_equal(m[64:-64].reshape(2, n), flags)
    assert [tuple(int(x) for x in r) for r in stat] == [(0, int(pres[i].sum())) for i in range(2)]


# --------------------------------------------------------------- parents ----
_DEAD = []  # why no further child is started
_SUMMARY = re.compile(r"^=*\s*((?:\d+ [a-z]+(?:, )?)+) in [0-9.]+s", re.M)
_FAULT_WORDS = ("illegal memory access", "hipErrorIllegalAddress", "Memory access fault", "HSA_STATUS_ERROR",
                "+++ Timeout +++", "Timeout >")


def _child_env(tag, build):
    key, val = SWITCH[tag]
    e = {k: v for k, v in os.environ.items() if k not in ("NP_RES", "NP_HUGE", "NP_HUGE_PAIR", "NP_REC_RES256")}
    e.update({key: val, "NP_FAMILY_CHILD": tag})
    if build == "checked":
        # one launch at a time, as the checked child of tests/test_gpu_bounds.py
        e.update(NP_LIB_PATH=CHK_LIB, NP_BOUNDS_CHILD="1", NP_PIPE_SLOTS="1")
    return e


assert N_CASES == {"res0": 11, "huge1": 7, "huge0": 5, "pair0": 5}, N_CASES


@pytest.mark.skipif(bool(FAMILY), reason="the parent of the family children")
@pytest.mark.timeout(max(LIMITS.values()) + 60)
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("tag", list(SWITCH))
def test_family_child(tag, build):
    assert not _DEAD, f"no further child is started on the GPU: {_DEAD[0]}"
    if build == "checked":
        assert os.path.exists(CHK_LIB), "run `make -C reed-solomon-novelpoly_amd chk` (__graft_entry__.build does)"
    cmd = [sys.executable, "-u", "-m", "pytest", "tests/test_gpu_families.py", "-m", "gpu", "-x", "-q",
           "-p", "no:cacheprovider", "--timeout", "120", "--timeout-method", "thread"]
    t0 = time.monotonic()
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=_child_env(tag, build), capture_output=True, text=True,
                           timeout=LIMITS[(tag, build)])
    except subprocess.TimeoutExpired as e:
        _DEAD.append(f"the {tag} child ({build}) ran into its {LIMITS[(tag, build)]} s limit")
        text = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
        pytest.fail(_DEAD[0] + "\n" + "\n".join(text.splitlines()[-30:]))
    text = r.stdout + r.stderr
    print(f"{tag} child ({build}): {time.monotonic() - t0:.1f} s of a {LIMITS[(tag, build)]} s limit")
    tail = "\n".join(text.splitlines()[-40:])
    if r.returncode in (134, 139) or r.returncode < 0:
        _DEAD.append(f"the {tag} child ({build}) died with exit status {r.returncode}")
    elif r.returncode != 0 and any(w in text for w in _FAULT_WORDS):
        _DEAD.append(f"the {tag} child ({build}) reported a device fault or a hung test")
    assert r.returncode == 0, tail
    m = _SUMMARY.findall(text)
    assert m, tail
    counts = {word: int(num) for num, word in re.findall(r"(\d+) ([a-z]+)", m[-1])}
    assert counts.get("passed") == N_CASES[tag], (counts, N_CASES[tag], tail)
    assert not counts.get("failed") and not counts.get("error") and not counts.get("errors"), tail

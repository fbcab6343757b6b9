"""np_kernel_family on the host (no GPU): the kernel family the engine's
dispatch (engine.cpp enc_path / rec_path) picks for a shape and a direction,
in the default process and, read in a fresh child, under each of the switches
of DESIGN.md §8a.  The expected table below restates that section; it calls
nothing of the library."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import novelpoly_amd as npa
from novelpoly_amd import synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
G, SMALL, FAST, RES, BIG, HUGE = (npa.FAMILY_GENERIC, npa.FAMILY_SMALL, npa.FAMILY_FAST, npa.FAMILY_RES,
                                  npa.FAMILY_BIG, npa.FAMILY_HUGE)
SL = 2 * 300
# every (n, k) the parameter check admits: powers of two, 2k <= n <= 65536
SHAPES = [(1 << a, 1 << b) for a in range(1, 17) for b in range(0, a)]


def expected(n, k, reconstruct, res=True, huge=None, res256=False):
    """DESIGN.md §8a.  res: NP_RES != 0; huge: NP_HUGE as set ("0", "1") or
    None; res256: NP_REC_RES256=1."""
    q = n // k
    if reconstruct and q not in (2, 4, 8):
        return G
    if k <= 32:
        return SMALL if q <= 8 else G
    if k <= 256:
        return RES if reconstruct and res256 and k == 256 else FAST
    if k in (512, 1024):
        return RES if res and q in (2, 4, 8) else BIG
    if k == 2048:
        return HUGE if huge == "1" else BIG
    if k <= 16384:
        return G if huge == "0" else HUGE
    return G


def table():
    return [[npa.kernel_family(npa.CodeParams(n, k, n), SL, rec) for rec in (False, True)] for n, k in SHAPES]


def fast_path_flags():
    return [npa.CodeParams(n, k, n).is_faster8() for n, k in SHAPES]


def test_constants_match_the_header():
    import re

    hdr = open(os.path.join(ROOT, "include", "novelpoly.h")).read()
    want = dict((name, int(v)) for name, v in re.findall(r"\bNP_(FAMILY_[A-Z]+)\s*=\s*(\d+)", hdr))
    assert len(want) == 6
    assert {name: getattr(npa, name) for name in want} == want
    assert [npa.FAMILY_NAMES[v] for v in range(6)] == ["GENERIC", "SMALL", "FAST", "RES", "BIG", "HUGE"]


def test_default_table_known_answers():
    """The rows of the issue's table, spelled out."""
    kat = [
        # (n, k, encode, reconstruct)
        (2, 1, SMALL, SMALL), (128, 32, SMALL, SMALL), (256, 32, SMALL, SMALL),
        (128, 64, FAST, FAST), (1024, 256, FAST, FAST), (2048, 256, FAST, FAST),
        (1024, 512, RES, RES), (4096, 512, RES, RES), (2048, 1024, RES, RES), (8192, 1024, RES, RES),
        (4096, 2048, BIG, BIG), (8192, 2048, BIG, BIG), (16384, 2048, BIG, BIG),
        (8192, 4096, HUGE, HUGE), (16384, 4096, HUGE, HUGE), (32768, 4096, HUGE, HUGE),
        (16384, 8192, HUGE, HUGE), (65536, 8192, HUGE, HUGE), (32768, 16384, HUGE, HUGE), (65536, 16384, HUGE, HUGE),
        # n / k >= 16: the encode by k, the decode generic
        (512, 32, G, G), (4096, 256, FAST, G), (65536, 256, FAST, G), (8192, 512, BIG, G), (32768, 1024, BIG, G),
        (32768, 2048, BIG, G), (65536, 2048, BIG, G), (65536, 4096, HUGE, G),
        (65536, 32768, G, G),
    ]
    for n, k, enc, rec in kat:
        p = npa.CodeParams(n, k, n)
        assert (npa.kernel_family(p, SL, False), npa.kernel_family(p, SL, True)) == (enc, rec), (n, k)


def test_default_table_every_shape():
    got = table()
    for (n, k), (enc, rec) in zip(SHAPES, got):
        assert (enc, rec) == (expected(n, k, False), expected(n, k, True)), (n, k)


def test_wanted_n_and_short_rows_do_not_matter():
    for n, k in [(1024, 256), (4096, 1024), (16384, 2048), (65536, 16384)]:
        for sl in (0, 2, SL):
            for wn in (k + 1, n - 1, n):
                p = npa.CodeParams(n, k, wn)
                assert npa.kernel_family(p, sl, False) == expected(n, k, False), (n, k, wn, sl)
                assert npa.kernel_family(p, sl, True) == expected(n, k, True), (n, k, wn, sl)


def test_invalid_params_answer_minus_one():
    L = npa.lib()
    assert L.np_kernel_family(None, SL, 0) == -1
    for n, k, wn in [(12, 3, 12), (1024, 300, 1024), (1000, 256, 1000), (256, 256, 256), (131072, 1024, 1024),
                     (1024, 256, 1025), (1024, 0, 1024)]:
        for rec in (0, 1):
            assert L.np_kernel_family(C.byref(npa._Params(n, k, wn)), SL, rec) == -1, (n, k, wn)


def test_sub_transform_scratch_limit():
    """The sub-transform kernels keep one 128 KiB slot per 1024 rows and
    64-column tile: n / 1024 slots per tile in the encode, (n + k) / 1024 in the
    decode.  One payload's slots may fill the 2 GiB every context has in the
    encode and half of that in the decode (engine.cpp kBigScratchMin); beyond,
    k = 4096 .. 16384 has only the generic kernels."""
    p = npa.CodeParams(65536, 16384, 65536)
    enc_tiles = (2 << 30) // ((65536 // 1024) * (128 << 10))
    rec_tiles = (1 << 30) // (((65536 + 16384) // 1024) * (128 << 10))
    assert (enc_tiles, rec_tiles) == (256, 102)
    assert npa.kernel_family(p, 2 * 64 * enc_tiles, False) == HUGE
    assert npa.kernel_family(p, 2 * 64 * enc_tiles + 2, False) == G
    assert npa.kernel_family(p, 2 * 64 * rec_tiles, True) == HUGE
    assert npa.kernel_family(p, 2 * 64 * rec_tiles + 2, True) == G
    # k = 2048 with NP_HUGE unset never asks: big at any length
    p = npa.CodeParams(16384, 2048, 16384)
    assert npa.kernel_family(p, 1 << 24, False) == BIG and npa.kernel_family(p, 1 << 24, True) == BIG


def _fast_path_consistent(shapes, fams_1mib, flags):
    for (n, k), (enc, rec), flag in zip(shapes, fams_1mib, flags):
        assert flag == (enc != G and rec != G), (n, k, enc, rec, flag)


def _families_1mib():
    out = []
    for n, k in SHAPES:
        p = npa.CodeParams(n, k, n)
        sl = npa.lib().np_shard_len(C.byref(p._c()), 1 << 20)
        out.append([npa.kernel_family(p, sl, rec) for rec in (False, True)])
    return out


def test_is_fast_path_agrees_with_the_table():
    _fast_path_consistent(SHAPES, _families_1mib(), fast_path_flags())
    for cfg in synth.CONFIGS.values():
        p = npa.CodeParams.derive_parameters(cfg["n_wanted"], cfg["k_wanted"])
        assert p.is_faster8() and G not in (npa.kernel_family(p, SL, False), npa.kernel_family(p, SL, True)), cfg


_CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import test_families_cpu as t
print(json.dumps({{"table": t.table(), "mib": t._families_1mib(), "fast": t.fast_path_flags()}}))
"""


def _child(env):
    """The tables as a fresh process reads them with `env` set (the switches
    are read once per process)."""
    paths = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "reed-solomon-novelpoly_amd", "python")]
    e = {k: v for k, v in os.environ.items() if k not in ("NP_RES", "NP_HUGE", "NP_HUGE_PAIR", "NP_REC_RES256")}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=e, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("env,kw", [({"NP_RES": "0"}, {"res": False}), ({"NP_HUGE": "1"}, {"huge": "1"}),
                                    ({"NP_HUGE": "0"}, {"huge": "0"}), ({"NP_REC_RES256": "1"}, {"res256": True}),
                                    ({"NP_RES": "0", "NP_HUGE": "1"}, {"res": False, "huge": "1"}),
                                    ({"NP_HUGE_PAIR": "0"}, {}), ({"NP_RES": "1"}, {})],
                         ids=["NP_RES=0", "NP_HUGE=1", "NP_HUGE=0", "NP_REC_RES256=1", "NP_RES=0,NP_HUGE=1",
                              "NP_HUGE_PAIR=0", "NP_RES=1"])
def test_table_under_a_switch(env, kw):
    got = _child(env)
    for (n, k), (enc, rec) in zip(SHAPES, got["table"]):
        assert (enc, rec) == (expected(n, k, False, **kw), expected(n, k, True, **kw)), (env, n, k)
    _fast_path_consistent(SHAPES, got["mib"], got["fast"])
    by = dict(zip(SHAPES, got["table"]))
    # the rows the switch is there for
    if env == {"NP_RES": "0"}:
        assert all(by[(q * k, k)] == [BIG, BIG] for k in (512, 1024) for q in (2, 4, 8))
    if env == {"NP_HUGE": "1"}:
        assert all(by[(q * 2048, 2048)] == [HUGE, HUGE] for q in (2, 4, 8)) and by[(32768, 2048)] == [HUGE, G]
    if env == {"NP_HUGE": "0"}:
        assert all(by[(q * k, k)] == [G, G] for k in (4096, 8192, 16384) for q in (2, 4, 8) if q * k <= 65536)
        assert not any(got["fast"][i] for i, (n, k) in enumerate(SHAPES) if k >= 4096)
    if env == {"NP_REC_RES256": "1"}:
        assert all(by[(q * 256, 256)] == [FAST, RES] for q in (2, 4, 8)) and by[(4096, 256)] == [FAST, G]


def test_res256_is_read_per_call(monkeypatch):
    p = npa.CodeParams(1024, 256, 1024)
    assert npa.kernel_family(p, SL, True) == FAST
    monkeypatch.setenv("NP_REC_RES256", "1")
    assert npa.kernel_family(p, SL, True) == RES and npa.kernel_family(p, SL, False) == FAST
    monkeypatch.delenv("NP_REC_RES256")
    assert npa.kernel_family(p, SL, True) == FAST

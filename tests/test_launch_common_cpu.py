"""csrc/launch_common.hpp on the CPU: tests/launch_common/check.cpp is compiled
as plain host C++17 with -fsanitize=address,undefined (a stand-alone program,
nothing preloaded), run, and its answers compared with what the launchers it
replaced computed -- each expectation names that launcher, as it stood in
kernels_fast.hip, kernels_small.hip, kernels_res.hip and kernels_huge.hip
before the dispatch and the grid arithmetic were written once.  And a source
check: the engine's table of kernel units names every unit's bounds record."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "reed-solomon-novelpoly_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "launch_common", "check.cpp")

T31, T32 = 1 << 31, 1 << 32


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_common") / "check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.stdout, r.stderr)
    return r.stdout.strip().splitlines()


def test_with_k_reaches_every_listed_k_and_nothing_else(answers):
    got = {(f[1], int(f[2])): int(f[3]) for f in (l.split() for l in answers) if f[0] == "with_k"}
    lists = {
        "fast": (64, 128, 256),  # the switch (a.k) ladders of kernels_fast.hip (launch_encode_masked, ...)
        "small": (1, 2, 4, 8, 16, 32),  # launch_encode_small / launch_reconstruct_small
        "huge_m": (2, 4, 8, 16),  # kernels_huge.hip with_m
        "records": (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024),  # launch_prefix_locator's eleven cases
    }
    for name, ks in lists.items():
        for k in ks:
            assert got[(name, k)] == k
        for k in (0, 3, 96, 2048 if name == "records" else 512):
            assert got[(name, k)] == -1  # the ladders' default
    assert "k_in 1 0 0" in answers


def test_with_nq_serves_2_4_8_and_rejects_the_rest(answers):
    got = {(int(f[1]), int(f[2])): (int(f[3]), int(f[4])) for f in (l.split() for l in answers)
           if f[0] == "with_nq" and len(f) == 5}
    for k in (1, 64, 1024):
        for nq in (2, 4, 8):  # by_nq, reconstruct_by_nq, launch_reconstruct_ragged_nq, kernels_huge.hip with_nq
            assert got[(nq * k, k)] == (nq, 1)
        # kernels_huge.hip with_nq rejected these; the others took NQ = 2, behind
        # *_supported predicates that are false here (n == 2k || n == 4k || n == 8k)
        for n in (k, 16 * k, 2 * k + 1) + ((3 * k,) if k > 1 else ()):
            assert got[(n, k)] == (-1, 0)
    assert got[(3, 1)] == (-1, 0)  # n = 3k and n = 2k + 1 at k = 1
    assert "with_nq 8 0 -1" in answers


def grid(answers, name):
    out = {}
    for f in (l.split() for l in answers):
        if f[0] == name:
            vals = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in f[5:]}
            out[(int(f[1]), int(f[2]), int(f[3]))] = (f[4], vals)
    return out


@pytest.mark.parametrize("w", [256, 64])
def test_tile_grid_one_tile_per_workgroup(answers, w):
    """with_encode_grid with one_tile and launch_reconstruct_k at tpw = 1
    (kernels_fast.hip, width 256); launch_encode_res_k and
    launch_reconstruct_res_k (kernels_res.hip, width 64): nothing to do for 0
    columns or batch 0, hipErrorInvalidValue for more than 2^32 - 1 columns or
    more than 2^31 - 1 workgroups, tiles = ceil(count / width), blocks =
    batch * tiles."""
    g = grid(answers, "grid")
    assert g[(0, w, 1)][0] == "empty" and g[(1, w, 0)][0] == "empty"
    for count in (1, 64, 65, 256, 257):
        tiles = -(-count // w)
        assert g[(count, w, 1)] == ("ok", {"count": count, "tiles": tiles, "per": 1, "blocks": tiles})
    assert {c: g[(c, 256, 1)][1]["tiles"] for c in (1, 256, 257)} == {1: 1, 256: 1, 257: 2}
    assert g[(T32 - 1, w, 1)] == ("ok", {"count": T32 - 1, "tiles": T32 // w, "per": 1, "blocks": T32 // w})
    assert g[(T32, w, 1)][0] == "invalid"
    assert g[(1, w, T31 - 1)] == ("ok", {"count": 1, "tiles": 1, "per": 1, "blocks": T31 - 1})
    assert g[(1, w, T31)][0] == "invalid"
    assert g[(3 * w, w, 715827882)] == ("ok", {"count": 3 * w, "tiles": 3, "per": 1, "blocks": T31 - 2})
    assert g[(3 * w, w, 715827883)][0] == "invalid"


@pytest.mark.parametrize("w", [256, 64])
def test_tile_grid_consecutive_tiles_per_workgroup(answers, w):
    """with_encode_grid and launch_reconstruct_k of kernels_fast.hip with tpw
    tiles per workgroup: blocks = batch * ceil(tiles / tpw), checked against
    2^31 - 1."""
    g = grid(answers, "grid2")
    assert g[(5 * w, w, 3)] == ("ok", {"count": 5 * w, "tiles": 5, "per": 2, "blocks": 9})
    assert g[(5 * w, w, T31 // 3 + 1)][0] == "invalid"  # 3 * (2^31 / 3 + 1) > 2^31 - 1


@pytest.mark.parametrize("w", [256, 64])
def test_tile_grid_four_tiles_per_workgroup_across_the_batch(answers, w):
    """launch_encode_k and launch_reconstruct_k of kernels_small.hip: blocks =
    ceil(batch * tiles / 4), hipErrorInvalidValue when batch * tiles exceeds
    2^32 - 1 (the tile number is a 32-bit value)."""
    g = grid(answers, "packed")
    assert g[(1, w, 0)][0] == "empty" and g[(0, w, 1)][0] == "empty"
    for batch, blocks in ((1, 1), (4, 1), (5, 2)):
        assert g[(1, w, batch)] == ("ok", {"count": 1, "tiles": 1, "per": 4, "blocks": blocks})
    assert g[(5 * w, w, 1)] == ("ok", {"count": 5 * w, "tiles": 5, "per": 4, "blocks": 2})
    assert g[(1, w, T32 - 1)] == ("ok", {"count": 1, "tiles": 1, "per": 4, "blocks": T32 // 4})
    assert g[(1, w, T32)][0] == "invalid"
    assert g[(2 * w, w, T31)][0] == "invalid"  # batch * tiles = 2^32
    assert g[(T32 - 1, w, 1)][0] == "ok" and g[(T32, w, 1)][0] == "invalid"


def test_engine_unit_table_names_every_bounds_record_and_lds_setup():
    """np_ctx_create and np_debug_bounds_check walk one table (engine.cpp
    kKernelUnits): a kernel file whose bounds record were missing from it would
    make the checked tests pass blind."""
    engine = open(os.path.join(CSRC, "engine.cpp")).read()
    table = re.search(r"kKernelUnits\[\] = \{(.*?)\n\};", engine, re.S).group(1)
    takes, configures = set(), set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")):
        src = open(path).read()
        takes |= set(re.findall(r"^hipError_t (bounds_take_\w+)\(uint32_t out\[8\]\) \{", src, re.M))
        configures |= set(re.findall(r"^hipError_t (configure_\w+_kernels)\(\) \{", src, re.M))
    assert len(takes) >= 10 and len(configures) >= 6
    for name in sorted(takes | configures):
        assert re.search(r"np::%s\b" % name, table), name
    # and nothing else configures or takes on the side
    assert len(re.findall(r"np::bounds_take_\w+", engine)) == len(takes)
    assert len(re.findall(r"np::configure_\w+_kernels", engine)) == len(configures)

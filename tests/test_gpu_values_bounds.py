"""tests/test_gpu_values.py in the checked build (lib/libnovelpoly_hip_chk.so,
-DNP_BOUNDS_CHECK=1; tests/test_gpu_bounds.py): degenerate symbols, presence
flags of every nonzero spelling, a d_present one byte past an aligned base on
the resident shapes and one flipped bit per byte position run through the
instrumented kernels of every family, and conftest.py's `_bounds_checked`
fixture asserts after every test of the child that no access fell outside.
The child runs the module without its multi-context tests, as
tests/test_gpu_recover_host_bounds.py does: the checked build keeps one extent
record per code object and device, so it supports one launch at a time and no
concurrent contexts (device_common.hpp); two contexts re-arm each other's
extents, and a flagged access is redirected to a sink.

Time limits: 120 s per test in the child, as the other children of the suite;
the subprocess five times the child's first measured run on an MI355X, at
least 60 s (as tests/test_gpu_families.py sets its LIMITS).  First measured
run of the whole child process (start of python, imports, the oracle's answers
and the GPU work of its 89 tests): 14.8 s, so the limit is 74 s; the product
library ran the whole module, 102 tests, in 14.0 s."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHK_LIB = os.path.join(ROOT, "reed-solomon-novelpoly_amd", "lib", "libnovelpoly_hip_chk.so")

MEASURED = 14.8  # first measured run of the child on an MI355X, seconds
LIMIT = max(60, int(5 * MEASURED + 0.999))


def _child_env():
    # as tests/test_gpu_bounds.py: one launch at a time
    return dict(os.environ, NP_LIB_PATH=CHK_LIB, NP_BOUNDS_CHILD="1", NP_PIPE_SLOTS="1")


@pytest.mark.timeout(LIMIT + 20)
def test_value_cases_in_bounds():
    assert os.path.exists(CHK_LIB), "run `make -C reed-solomon-novelpoly_amd chk` (__graft_entry__.build does)"
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "tests/test_gpu_values.py", "-m", "gpu",
                        "-k", "not multi", "-x", "-q", "-p", "no:cacheprovider", "--timeout", "120",
                        "--timeout-method", "thread"],
                       cwd=ROOT, env=_child_env(), capture_output=True, text=True, timeout=LIMIT)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and " error" not in tail, tail

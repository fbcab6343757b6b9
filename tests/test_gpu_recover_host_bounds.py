"""np_recover_batch_host in the checked build (lib/libnovelpoly_hip_chk.so,
-DNP_BOUNDS_CHECK=1; tests/test_gpu_bounds.py): the recover kernels run on the
pipeline slots' n-row device layouts and output blocks, with the extents they
arm there, and conftest.py's `_bounds_checked` fixture asserts after every test
of the child that no access fell outside.  The child runs
tests/test_gpu_recover_host.py without the multi-context tests: one context
and, with one pipeline slot, one launch at a time."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHK_LIB = os.path.join(ROOT, "reed-solomon-novelpoly_amd", "lib", "libnovelpoly_hip_chk.so")


def _child_env():
    # as tests/test_gpu_recover_bounds.py: one launch at a time
    return dict(os.environ, NP_LIB_PATH=CHK_LIB, NP_BOUNDS_CHILD="1", NP_PIPE_SLOTS="1")


@pytest.mark.timeout(600)
def test_host_recover_kernels_in_bounds():
    assert os.path.exists(CHK_LIB), "run `make -C reed-solomon-novelpoly_amd chk` (__graft_entry__.build does)"
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "tests/test_gpu_recover_host.py", "-m", "gpu",
                        "-k", "not multi", "-x", "-q", "-p", "no:cacheprovider", "--timeout", "120",
                        "--timeout-method", "thread"],
                       cwd=ROOT, env=_child_env(), capture_output=True, text=True, timeout=580)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and " error" not in tail, tail

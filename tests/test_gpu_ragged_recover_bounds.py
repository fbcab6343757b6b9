"""np_recover_ragged_dev in the checked build (lib/libnovelpoly_hip_chk.so,
-DNP_BOUNDS_CHECK=1; tests/test_gpu_bounds.py): the ragged recover encode arms
the shard extent with the size the caller passed, the payload extent -- the
scratch, or with d_out the caller's output buffer at the size it passed --
and those of the item records, the block table, the plan at the recover plan's
stride, the present flags, the status and the flag map; the ragged masked and
verify encodes and the ragged decode run on the same records with d_out.
conftest.py's `_bounds_checked` fixture asserts after every test of the child
that no access fell outside.  The child runs tests/test_gpu_ragged_recover.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHK_LIB = os.path.join(ROOT, "reed-solomon-novelpoly_amd", "lib", "libnovelpoly_hip_chk.so")


def _child_env():
    # as tests/test_gpu_restore_bounds.py: one launch at a time
    return dict(os.environ, NP_LIB_PATH=CHK_LIB, NP_BOUNDS_CHILD="1", NP_PIPE_SLOTS="1")


@pytest.mark.timeout(600)
def test_ragged_recover_kernels_in_bounds():
    assert os.path.exists(CHK_LIB), "run `make -C reed-solomon-novelpoly_amd chk` (__graft_entry__.build does)"
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "tests/test_gpu_ragged_recover.py", "-m", "gpu", "-x", "-q",
                        "-p", "no:cacheprovider", "--timeout", "120", "--timeout-method", "thread"],
                       cwd=ROOT, env=_child_env(), capture_output=True, text=True, timeout=580)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and " error" not in tail, tail

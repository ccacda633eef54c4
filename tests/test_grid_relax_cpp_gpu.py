"""stencil::hip::relax and sor (include/StencilStream/hip/Relax.hpp) through tests/cpp_relax/grid_relax_test.hip: a plane
of floats as a whole, with SOR and a right-hand side, on a rectangle with parity 1; members of struct cells of two cell
types with another member as right-hand side, doubles; all against the same half-sweeps in host C++ built with
-ffp-contract=off, as equal bits; std::range_error and std::invalid_argument; and the validity flags between relax and the
GridAccessor."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_relax_against_a_host_loop_errors_and_flags():
    path = os.path.join(ROOT, "build", "tests", "grid_relax_test")
    if not os.path.exists(path):
        pytest.fail("build/tests/grid_relax_test missing: run __graft_entry__.build()")
    res = subprocess.run([path], capture_output=True, timeout=300)
    text = (res.stdout + res.stderr).decode()[-3000:]
    assert res.returncode == 0, text
    assert b"grid_relax_test:" in res.stdout and b" 0 failures" in res.stdout, text
    assert b"flag protocol:" in res.stdout

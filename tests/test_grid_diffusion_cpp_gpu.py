"""stencil::hip::diffuse, jacobi_step and diagonal_solve (include/StencilStream/hip/Diffusion.hpp) through
tests/cpp_diffusion/grid_diffusion_test.hip: planes of floats and of doubles as a whole and on a rectangle, with and
without a right-hand side (also the destination itself); members of struct cells of two cell types with the faces and
the right-hand side as other members; all against the same formula in host C++ built with -ffp-contract=off, as equal
bits; std::range_error and std::invalid_argument; and the validity flags between the calls and the GridAccessor."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_diffusion_against_a_host_loop_errors_and_flags():
    path = os.path.join(ROOT, "build", "tests", "grid_diffusion_test")
    if not os.path.exists(path):
        pytest.fail("build/tests/grid_diffusion_test missing: run __graft_entry__.build()")
    res = subprocess.run([path], capture_output=True, timeout=300)
    text = (res.stdout + res.stderr).decode()[-3000:]
    assert res.returncode == 0, text
    assert b"grid_diffusion_test:" in res.stdout and b" 0 failures" in res.stdout, text
    assert b"flag protocol:" in res.stdout

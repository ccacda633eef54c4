"""stencil::hip::combine / restrict_mean / prolong_bilinear (include/StencilStream/hip/Algebra.hpp) through
tests/cpp_algebra/grid_algebra_test.hip: planes of floats and members of struct cells of two cell types against the same
formulas in plain host C++ (built with -ffp-contract=off), bit for bit; std::range_error for rectangles outside a grid,
std::invalid_argument for element types that differ and for a wrong number of terms; and the validity flags between these
calls and the GridAccessor (write through an accessor, combine, read through an accessor)."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_algebra_against_host_formulas_errors_and_flags():
    path = os.path.join(ROOT, "build", "tests", "grid_algebra_test")
    if not os.path.exists(path):
        pytest.fail("build/tests/grid_algebra_test missing: run __graft_entry__.build()")
    res = subprocess.run([path], capture_output=True, timeout=300)
    text = (res.stdout + res.stderr).decode()[-3000:]
    assert res.returncode == 0, text
    assert b"grid_algebra_test:" in res.stdout and b" 0 failures" in res.stdout, text
    assert b"flag protocol:" in res.stdout

"""stencil::hip::apply (include/StencilStream/hip/Operator.hpp) through tests/cpp_operator/grid_operator_test.hip: a
plane of floats and members of struct cells of two cell types against the same formula in plain host C++ (built with
-ffp-contract=off), bit for bit; std::range_error for rectangles outside a grid, std::invalid_argument for element types
that differ and for a cross with corner weights; and the validity flags between apply and the GridAccessor (write through
an accessor, apply, read through an accessor)."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_apply_against_host_formulas_errors_and_flags():
    path = os.path.join(ROOT, "build", "tests", "grid_operator_test")
    if not os.path.exists(path):
        pytest.fail("build/tests/grid_operator_test missing: run __graft_entry__.build()")
    res = subprocess.run([path], capture_output=True, timeout=300)
    text = (res.stdout + res.stderr).decode()[-3000:]
    assert res.returncode == 0, text
    assert b"grid_operator_test:" in res.stdout and b" 0 failures" in res.stdout, text
    assert b"flag protocol:" in res.stdout

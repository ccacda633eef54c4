"""stencil::hip::read / write / fill / copy (include/StencilStream/hip/Region.hpp) through
tests/cpp_regions/grid_regions_test.hip: a Grid<float> and a grid of three-member struct cells against host loops, the
validity flags between the region calls and the GridAccessor, std::range_error for rectangles outside the grid, and a
five-point functor on 64 x 64 with a source filled in between two StencilUpdate calls against stencil::cpu doing the
same through accessors, bit for bit."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_regions_flags_and_the_source_between_two_updates():
    path = os.path.join(ROOT, "build", "tests", "grid_regions_test")
    if not os.path.exists(path):
        pytest.fail("build/tests/grid_regions_test missing: run __graft_entry__.build()")
    res = subprocess.run([path], capture_output=True, env=dict(os.environ, OMP_NUM_THREADS="4"), timeout=300)
    text = (res.stdout + res.stderr).decode()[-3000:]
    assert res.returncode == 0, text
    assert b"grid_regions_test:" in res.stdout and b" 0 failures" in res.stdout, text
    assert b"source between two updates:" in res.stdout

"""stencil::hip::norms / stencil::hip::distance (include/StencilStream/hip/Reduce.hpp) through
tests/cpp_norms/grid_norms_test.hip: a Grid<float> and a grid of two-field struct cells against a host loop with the
same definitions, and the documentation's "run until converged" loop (a five-point functor on 64 x 64, 8 generations
per call) against the same loop on stencil::cpu with a host scan: as many calls, the same cells."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_norms_distance_and_the_converging_loop():
    path = os.path.join(ROOT, "build", "tests", "grid_norms_test")
    if not os.path.exists(path):
        pytest.fail("build/tests/grid_norms_test missing: run __graft_entry__.build()")
    res = subprocess.run([path], capture_output=True, env=dict(os.environ, OMP_NUM_THREADS="4"), timeout=300)
    text = (res.stdout + res.stderr).decode()[-3000:]
    assert res.returncode == 0, text
    assert b"grid_norms_test:" in res.stdout and b" 0 failures" in res.stdout, text
    assert b"run until converged:" in res.stdout

"""Which waves call a transition function's row form (Sweep.hpp: row form, edge waves), through
tests/cpp_edge_rows/edge_rows_test.hip: a canary whose row_at_level adds a constant to every result.  One launch on a
71 x 701 grid in row chunks of sixteen rows, at depth 1 and at depth 4 on four stages: every cell of the grid carries
the constant, in edge units and check-free units alike; with SweepTuning::row_form_edges = false exactly the cells of
the edge units do not (the rectangles are predicted from Sweep::entry's condition)."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_edge_units_call_the_row_form_unless_the_tuning_says_no():
    path = os.path.join(ROOT, "build", "tests", "edge_rows_test")
    if not os.path.exists(path):
        pytest.fail("build/tests/edge_rows_test missing: run __graft_entry__.build()")
    res = subprocess.run([path], capture_output=True, timeout=300)
    text = (res.stdout + res.stderr).decode()[-3000:]
    print(text)
    assert res.returncode == 0, text
    assert b"edge_rows_test: 0 failures" in res.stdout, text
    assert res.stdout.count(b" 0 wrong") == 4, text

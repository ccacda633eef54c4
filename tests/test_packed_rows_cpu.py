"""The packed row form of the uniform Jacobi kernel on the host (tests/cpp_packed/packed_rows_test.cpp, built by
__graft_entry__.build() with the ROCm installation's clang and -ffp-contract=off): Jacobi5Uniform::row_at_level on rows
in lane order (c0, c2, c1, c3) against at_level cell by cell -- bit for bit, NaNs by position -- for each of the four
launch variants, at the first, a middle, the last and the only level of a launch, on rows of five lanes whose shifts
hand over the neighbouring lanes' cells, with random values and planted subnormals, +-0, +-inf and NaN."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("variant", ["middle", "first", "last", "only"])
def test_row_form_equals_the_cell_form_bit_for_bit(variant):
    path = os.path.join(ROOT, "build", "tests", "packed_rows_test")
    if not os.path.exists(path):
        pytest.fail("build/tests/packed_rows_test missing: run __graft_entry__.build()")
    res = subprocess.run([path, variant, "20000"], capture_output=True, timeout=120)
    text = (res.stdout + res.stderr).decode()[-3000:]
    assert res.returncode == 0, text
    assert b"packed_rows_test: 0 failures" in res.stdout, text

"""User functors of every pipeline shape SweepTuning's rule produces (hip/internal/Sweep.hpp), swept through
stencil::hip::StencilUpdate and compared with stencil::cpu::StencilUpdate field by field
(tests/cpp_shapes/shape_cases.hpp: the shapes, static asserts on each and the driver; DESIGN.md, tests section).

Each binary holds three cases and sweeps, per case, ten widths around the strip seams of the default and the narrow
form, each at two of four heights (one row ... several row chunks), for 1, 2, 3, T-1, T, T+1 and 2T+3 generations,
then a run from iteration 5 and a second call resumed through get_params(); and the grids on which units of the wave
grid run the check-free code (their whole footprint inside the grid), which the widths above never reach: 2 OW + GX - 1
columns (strip 1 just misses), 2 OW + GX (just fits) and 3 OW + GX + 1 (two such strips and a ragged third), for the
narrow form as well, at a + 8 + G - 1 rows (a = G rounded up to 8: with chunks of eight rows no chunk qualifies),
a + 8 + G (one does) and 4 G + 7.  tests/test_template_hooks_gpu.py proves with a canary which units of those grids
run that code.  Every functor is a position-sensitive
hash of its neighbourhood, so a neighbour from the wrong lane, row, level or generation changes cells; a mismatch
prints the functor, the grid, the generations, the depth and the first differing (row, column, field).

The environments: none (small grids take the narrow form where a shape has one); the default shape; the default shape
with the one-word functor's depth 16 outright (unmeasured launches run 8); the default shape with row chunks of eight
rows (chunk seams at every height); the default shape with row chunks of sixteen rows, a taper of two entries and
renumbered workgroups (tapered-xcd).  The taper needs tiers of at least four rows that are shorter than the chunk, so
it engages at the taller heights only.  Of a functor's four heights 1, 3, G + 1 and 4 G + 7 (G = radius x
sub-iterations x depth) `build/tests/launch_plan_test plan 0 <h> <h> <G>` prints, under that environment: one chunk for
1 and 3 and for G + 1 up to 16 rows (F3x1 4, D2x1 5, the fat cells and Quad1 9, D1 13); two 16-row chunks in one tier
for G + 1 = 17 (U16, Mixed2) and 19 (F3); two tiers (16 / 4) for F2x2's G + 1 = 25 and D2x1's 4 G + 7 = 23; one tier
for F3x1's 4 G + 7 = 19; and three tiers (16 / 8 / 4) for every other 4 G + 7: 39 (Tri1, Quad1, Octo1, Penta1), 55
(D1), 71 (U16, Mixed2), 79 (F3) and 103 (F2x2).  STSTHIP_ALLOW_SPILLING_DEPTHS=1 is for binaries whose report names a
spill-free depth below the compiled one (SPILLING below), so that the deep kernels are compared as well: on gfx950
every case reports its compiled depth as spill-free (U16 16, F3 6, D1 12, the fat cells 8, F2x2 6, F3x1 1, D2x1 2), so
no binary is listed and the environment is left out; each test asserts the reported depths, and a case that drops
below its compiled depth fails there until its binary is listed."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

OUT = os.path.join(ROOT, "build", "tests")
BINARIES = {
    "shape_test_a": ["U16", "Quad1/split-request", "Tri1/aos"],
    "shape_test_b": ["F3", "D1", "Tri1/planes"],
    "shape_test_c": ["Octo1", "Penta1", "Mixed2/planes"],
    "shape_test_d": ["F2x2", "F3x1", "D2x1"],
}
WIDE = {"STSTHIP_NARROW_FORM_KCELLS": "0"}
ENVIRONMENTS = {
    "narrow-form": {},
    "default-shape": WIDE,
    "chunks-of-8-rows": dict(WIDE, STSTHIP_CHUNK_ROWS="8"),
    "tapered-xcd": dict(WIDE, STSTHIP_CHUNK_ROWS="16", STSTHIP_TAPER="500:2,250:4", STSTHIP_XCD_REMAP="1"),
}
# the binary that holds the one-word functor (U16: compiled 16 deep, 8 by default)
DEPTH_16 = ("shape_test_a", dict(WIDE, STSTHIP_TUNE_DEPTH="16"))
# binaries with a case whose spill-free depth is below its compiled depth
SPILLING = []

CASES = [pytest.param(b, env, id=f"{b}-{name}") for b in BINARIES for name, env in ENVIRONMENTS.items()]
CASES.append(pytest.param(*DEPTH_16, id=f"{DEPTH_16[0]}-depth-16"))
CASES += [pytest.param(b, {"STSTHIP_ALLOW_SPILLING_DEPTHS": "1"}, id=f"{b}-spilling-depths") for b in SPILLING]

KNOBS = ("STSTHIP_NARROW_FORM_KCELLS", "STSTHIP_TUNE_DEPTH", "STSTHIP_CHUNK_ROWS", "STSTHIP_ALLOW_SPILLING_DEPTHS",
         "STSTHIP_MAX_GENERATIONS", "STSTHIP_NARROW_BAND_ROWS", "STSTHIP_TAPER", "STSTHIP_XCD_REMAP",
         "STSTHIP_LAST_CHUNK_EARLY")


def binary(name):
    path = os.path.join(OUT, name)
    if not os.path.exists(path):
        pytest.fail(f"build/tests/{name} missing: run __graft_entry__.build()")
    return path


def run(cmd, **env):
    env = dict({k: v for k, v in os.environ.items() if k not in KNOBS}, OMP_NUM_THREADS="4", **env)
    res = subprocess.run(cmd, capture_output=True, env=env, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr).decode()[-3000:]
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", CASES)
def test_every_shape_equals_the_cpu_backend(name, env):
    res = run([binary(name)], **env)
    text = res.stdout.decode()
    assert f"{name}:" in text and " 0 failures" in text, (res.stdout + res.stderr).decode()[-3000:]
    for functor in BINARIES[name]:
        report = re.search(rf"^shape {re.escape(functor)}: K=\d+ T=(\d+) .* depth=(\d+)$", text, re.M)
        assert report, f"no report line for {functor}\n" + text[-3000:]
        if env.get("STSTHIP_ALLOW_SPILLING_DEPTHS") == "1" or name not in SPILLING:
            assert report.group(1) == report.group(2), (
                f"{report.group(0)}: the compiled depth is not swept; list {name} in SPILLING")
    assert b"MISMATCH" not in res.stderr, res.stderr.decode()[-3000:]

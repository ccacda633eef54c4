"""What a transition function may add to the plain protocol, swept through stencil::hip::StencilUpdate and compared with
stencil::cpu::StencilUpdate field by field (tests/cpp_shapes/hook_cases.hpp: the functors, their tunings and the static
asserts; DESIGN.md, tests section).  The grids, the generations and the comparison are the shape matrix's
(tests/test_template_shapes_gpu.py), the grids that reach the check-free code included.

shape_test_e, the hooks: interior() that is right only for cells off the rim of the grid (Rim), at_level<level, levels>()
that is right only when the sweep names the level it computes (Levels), the column hint against the check-free promise
on one-cell lanes (OneWayRim), and the canary.  shape_test_f, the column hint (halo_columns_per_generation): one-way
reads as AoS (OneWay) and on two planes with a constant field over five passes (OneWayPlanes), and a functor whose
hint is wrong (Liar).  Both run in every environment of the shape matrix.

shape_test_g / _h, explicit tunings: no `stages` at depth 8 (Lone8), depth 12 on four and three stages (Twelve),
batches of eight rows with every toggle off (Batch8), a 32-byte cell with every toggle on (FatOn).  shape_test_i / _j,
the function object: no state, 7, 16 (a double), 36, 40 and 64 bytes (a table indexed at run time) -- scalar registers
take it at 16 and 36 bytes only; and the shape matrix's F3 with its time-dependent values evaluated by the kernel and
precomputed on the device.  These run in the default shape and with row chunks of eight rows.

The canary's interior() returns a value that is never operator()'s.  After ONE launch the cells that differ from the cpu
backend must be exactly the output rectangles of the units Sweep::entry() hands the check-free code; the binary
restates that predicate for row chunks of eight rows (the plan is deterministic there) and prints the number of such
units per grid.  Strip 1 of a grid has its footprint inside from 2 OW + GX columns on, the chunk [a, a + 8) its warm-up
rows from a + 8 + G rows on (a = G rounded up to eight): the sets are empty one column or one row below, and hold one
or two strips of one chunk at 2 OW + GX and 3 OW + GX + 1 columns -- so the check-free grids of every case run the
check-free code.  The liar's result must differ from the cpu backend at 2 OW + 3 columns and must not at OW: the
widths put a seam where the hint matters."""
import re

import pytest

from test_template_shapes_gpu import ENVIRONMENTS, binary, run

EVERYWHERE = {
    "shape_test_e": ["Rim", "Levels", "OneWayRim"],
    "shape_test_f": ["OneWay", "OneWayPlanes/planes"],
}
TWICE = {
    "shape_test_g": ["Lone8", "Twelve"],
    "shape_test_h": ["Batch8", "FatOn"],
    "shape_test_i": ["Stateless", "State7", "State16", "State36"],
    "shape_test_j": ["State40", "StateTable", "F3/inline", "F3/on-device"],
}
BINARIES = dict(EVERYWHERE, **TWICE)
# Binaries with a case whose spill-free depth is below its compiled depth (tests/test_template_shapes_gpu.py has the
# mechanism): OneWayPlanes.  Its kernels that store the constant plane hold 32 bytes of private memory per lane at every
# depth (no register spills; the variants that skip the plane hold none), so the depth rule sweeps it one generation
# deep -- where the hint changes nothing.  Each of its environments therefore runs a second time with
# STSTHIP_ALLOW_SPILLING_DEPTHS=1, and there the compiled depth must be the swept one.
SPILLING = ["shape_test_f"]
ALLOW = {"STSTHIP_ALLOW_SPILLING_DEPTHS": "1"}
ALL_ENVIRONMENTS = dict(ENVIRONMENTS, **{f"{name}-spilling-depths": dict(env, **ALLOW) for name, env in ENVIRONMENTS.items()})
CASES = [pytest.param(b, e, id=f"{b}-{e}") for b in EVERYWHERE for e in ENVIRONMENTS]
CASES += [pytest.param(b, f"{e}-spilling-depths", id=f"{b}-{e}-spilling-depths") for b in SPILLING for e in ENVIRONMENTS]
CASES += [pytest.param(b, e, id=f"{b}-{e}") for b in TWICE for e in ("default-shape", "chunks-of-8-rows")]

# the canary's shape (static_assert in hook_cases.hpp): K 4, T 4 on four stages, radius 1
CANARY = dict(OW=248, GX=4, LW=256, G=4)


def check_free_units(height, width, OW, GX, LW, G, chunk=8):
    """Sweep::entry()'s predicate for whole rows in one tier of `chunk`-row chunks"""
    units = 0
    for strip in range(-(-width // OW)):
        for ya in range(0, height, chunk):
            yb = min(ya + chunk, height)
            xw0 = strip * OW - GX
            units += xw0 > 0 and xw0 + LW <= width and ya - G >= 0 and yb + G <= height
    return units


@pytest.mark.gpu
@pytest.mark.parametrize("name,environment", CASES)
def test_hooks_hints_and_tunings_equal_the_cpu_backend(name, environment):
    env = ALL_ENVIRONMENTS[environment]
    res = run([binary(name)], **env)
    text = res.stdout.decode()
    assert f"{name}:" in text and " 0 failures" in text, (res.stdout + res.stderr).decode()[-3000:]
    for functor in BINARIES[name]:
        report = re.search(rf"^shape {re.escape(functor)}: K=\d+ T=(\d+) .* depth=(\d+)$", text, re.M)
        assert report, f"no report line for {functor}\n" + text[-3000:]
        if name not in SPILLING or env.get("STSTHIP_ALLOW_SPILLING_DEPTHS") == "1":
            assert report.group(1) == report.group(2), (
                f"{report.group(0)}: the compiled depth is not swept; list {name} in SPILLING")
    assert b"MISMATCH" not in res.stderr, res.stderr.decode()[-3000:]

    if name == "shape_test_e" and environment == "chunks-of-8-rows":
        OW, GX, G = CANARY["OW"], CANARY["GX"], CANARY["G"]
        a = -(-G // 8) * 8
        widths = [2 * OW + GX - 1, 2 * OW + GX, 3 * OW + GX + 1]
        heights = [a + 8 + G - 1, a + 8 + G, 4 * G + 7]
        want = {(h, w): check_free_units(h, w, **CANARY) for h in heights for w in widths}
        # strip 1 just misses at the first width, no chunk qualifies at the first height; one chunk of one strip and
        # of two at the others
        assert all((n == 0) == (w == widths[0] or h == heights[0]) for (h, w), n in want.items())
        assert want[(heights[1], widths[1])] == 1 and want[(heights[2], widths[2])] == 2
        line = f"canary: depth {G}, units" + "".join(f" {h}x{w}:{want[(h, w)]}" for h in heights for w in widths)
        assert line in text.splitlines(), f"want {line!r}\n" + text[-3000:]
    if name == "shape_test_f":
        liar = re.search(r"^liar: K=1 T=2 OW=60 depth=2, cells that differ at width 60: 0, at width 123: (\d+)$", text, re.M)
        assert liar and int(liar.group(1)) > 0, text[-3000:]

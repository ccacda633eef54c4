"""The user functors of every pipeline shape (tests/cpp_shapes/shape_cases.hpp) through the drivers that cut a grid over
several GPUs: stencil::hip::StripUpdate on 1, 2 and 3 ranks and stencil::hip::BlockUpdate on meshes 1 x 1, 1 x 2, 2 x 1,
2 x 2, 1 x 3, 3 x 1 and 3 x 3, the ranks as threads of one process with an in-process mailbox whose waits are bounded
(tests/cpp/mesh_harness.hpp), the owned cells assembled and compared field by field with stencil::cpu::StencilUpdate on
the whole grid (tests/cpp_shapes/mesh_cases.hpp: the second mode of shape_test_a ... shape_test_d; DESIGN.md, tests
section).

Every extent is derived from the sweep's description (D generations per launch, hpg halo cells per generation,
g = D * hpg): per cut axis n * 2 * g (every rank owns exactly two ghost depths) and a ragged extent with a sweep seam
inside at STSTHIP_EXCHANGE_EVERY=1; extents that keep the rule's interval (4 for strips, 2 for blocks) with nothing
set; 8 * g per rank (keeps 2) and 8 * g - 1 (must fall to 1) at STSTHIP_EXCHANGE_EVERY=2.  Generations: 1, m * D + 1
and 2 * m * D + 3, a run from iteration 5 and a second call resumed through get_params() after an odd number of
launches.  Every run asserts from the drivers' counters that the interval it meant to test was in effect; at
STSTHIP_EXCHANGE_EVERY=1 grids one row or column thinner than two ghost depths must be refused.  "substrips": strips of
3 ranks swept as two sub-strips with a moving boundary, at the smallest height the driver accepts for them, for more
generations than the boundary's span; the launch counters show that every pass ran as two launches.

shape_test_f holds the two functors that declare halo_columns_per_generation (tests/cpp_shapes/hook_cases.hpp: one-way
reads as AoS and on planes with a constant field); its mesh mode runs at STSTHIP_EXCHANGE_EVERY=1, where the drivers'
ghost depth is radius x sub-iterations per generation while the kernel's column halo is the hint's.

Options are read once per process, so each environment is one case per binary.  A mismatch prints the functor, the
mesh, every rank's rows and columns, the interval, the generations and the first differing (row, column, field)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_template_shapes_gpu import BINARIES, KNOBS, OUT, WIDE

ENVIRONMENTS = {
    "exchange-every-launch": dict(WIDE, STSTHIP_EXCHANGE_EVERY="1"),
    "exchange-by-the-rule": WIDE,
    "exchange-every-2": dict(WIDE, STSTHIP_EXCHANGE_EVERY="2"),
}
# the functors with a column hint: every launch exchanges; at every compiled depth, because the spill-free depth of the
# one on planes is 1 (tests/test_template_hooks_gpu.py, SPILLING), where the hint changes nothing
HINTED = {"shape_test_f": ["OneWay", "OneWayPlanes/planes"]}
ENVIRONMENTS["exchange-every-launch-hinted"] = dict(ENVIRONMENTS["exchange-every-launch"], STSTHIP_ALLOW_SPILLING_DEPTHS="1")
MESH_CASES = [pytest.param(b, e, id=f"{b}-{e}") for b in BINARIES for e in ENVIRONMENTS if not e.endswith("-hinted")]
MESH_CASES += [pytest.param(b, "exchange-every-launch-hinted", id=f"{b}-exchange-every-launch") for b in HINTED]
INTERVAL = {"exchange-every-launch": "1", "exchange-every-launch-hinted": "1", "exchange-by-the-rule": "rule", "exchange-every-2": "2"}
SUBSTRIPS = dict(WIDE, STSTHIP_EXCHANGE_EVERY="2", STSTHIP_STRIP_SUBSTRIPS="2", STSTHIP_SKEWED_STRIPS="1")
MESH_KNOBS = KNOBS + ("STSTHIP_EXCHANGE_EVERY", "STSTHIP_STRIP_SUBSTRIPS", "STSTHIP_SKEWED_STRIPS", "STSTHIP_VIRTUAL_STRIPS")


def run_mode(name, mode, env):
    path = os.path.join(OUT, name)
    if not os.path.exists(path):
        pytest.fail(f"build/tests/{name} missing: run __graft_entry__.build()")
    env = dict({k: v for k, v in os.environ.items() if k not in MESH_KNOBS}, OMP_NUM_THREADS="16", **env)
    # (the mailbox ends a mesh whose ranks disagree after 30 s of waiting; the limit here is for everything else)
    res = subprocess.run([path, mode], capture_output=True, env=env, timeout=300)
    text = res.stdout.decode()
    tail = (res.stdout + res.stderr).decode()[-4000:]
    assert res.returncode == 0, tail
    assert f"{name}:" in text and " 0 failures" in text, tail
    for word in (b"MISMATCH", b"INTERVAL", b"LAUNCHES", b"mailbox"):
        assert word not in res.stderr, tail
    return text


def report_of(text, mode, functor):
    report = re.search(rf"^{mode} shape {re.escape(functor)}: D=(\d+) hpg=(\d+) g=(\d+) interval=(\S+) runs=(\d+) .* "
                       rf"extents:(.*) exchanges:(.*)$", text, re.M)
    assert report, f"no {mode} report line for {functor}\n" + text[-3000:]
    return report


@pytest.mark.gpu
@pytest.mark.parametrize("name,environment", MESH_CASES)
def test_every_shape_on_strips_and_meshes_equals_the_cpu_backend(name, environment):
    text = run_mode(name, "mesh", ENVIRONMENTS[environment])
    for functor in dict(BINARIES, **HINTED)[name]:
        report = report_of(text, "mesh", functor)
        D, hpg, g = (int(report.group(i)) for i in (1, 2, 3))
        assert g == D * hpg and report.group(4) == INTERVAL[environment]
        extents, exchanges = report.group(6), report.group(7)
        for decomposition in ("strips1", "strips2", "strips3", "mesh1x1", "mesh1x2", "mesh2x1", "mesh2x2", "mesh1x3",
                              "mesh3x1", "mesh3x3"):
            assert f" {decomposition}:" in extents, f"{functor}: {decomposition} did not run\n{report.group(0)}"
        if environment.startswith("exchange-every-launch"):
            # at the limit: every rank owns exactly two ghost depths along every cut axis
            assert f" strips2:{4 * g}x" in extents and f" strips3:{6 * g}x" in extents, report.group(0)
            assert f" mesh2x2:{4 * g}x{4 * g}" in extents and f" mesh3x3:{6 * g}x{6 * g}" in extents, report.group(0)
            assert "/m1/" in exchanges and "/m2/" not in exchanges and "/m4/" not in exchanges, report.group(0)
        elif environment == "exchange-by-the-rule":
            assert f" strips3:{3 * 16 * g}x" in extents and f" mesh3x3:{3 * 8 * g}x{3 * 8 * g}" in extents, report.group(0)
            assert re.search(r" strips3:\S*/m4/", exchanges) and re.search(r" mesh3x3:\S*/m2/", exchanges), report.group(0)
        else:
            # 8 g per rank keeps two launches per exchange, 8 g - 1 falls to one
            assert re.search(rf" strips3:{24 * g}x\d+/m2/", exchanges), report.group(0)
            assert re.search(rf" strips3:{3 * (8 * g - 1)}x\d+/m1/", exchanges), report.group(0)
            assert re.search(rf" mesh3x3:{24 * g}x{24 * g}/m2/", exchanges), report.group(0)
            assert re.search(rf" mesh3x3:{24 * g}x{3 * (8 * g - 1)}/m1/", exchanges), report.group(0)
            assert re.search(rf" mesh3x3:{3 * (8 * g - 1)}x{24 * g}/m1/", exchanges), report.group(0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BINARIES))
def test_every_shape_on_two_substrips_with_a_moving_boundary(name):
    text = run_mode(name, "substrips", SUBSTRIPS)
    for functor in BINARIES[name]:
        report = report_of(text, "substrips", functor)
        assert report.group(4) == "2" and int(report.group(5)) == 1 and " strips3:" in report.group(6), report.group(0)

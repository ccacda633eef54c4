"""Single sweep launches (ststhip_app_sweep) of EVERY registered transition function under every kind of launch plan.

Every result of the library comes out of launch_sweep (hip/internal/Sweep.hpp): it cuts the rows of a launch into
chunks (pick_chunk_rows), cuts the tail finer in up to four tiers (plan_tiers), may dispatch the bottom chunk second
(last_chunk_early) and renumber the workgroups per XCD (xcd_remap); the kernel's entry() decodes blockIdx back into a
strip and a row range and picks the check-free or the edge code from it.  The plan a grid gets by default is an
accident of the occupancy model, so the plans are FORCED here through the STSTHIP_* knobs (PLANS below), and each case
first asks `build/tests/launch_plan_test plan` (tests/cpp/launch_plan_test.hip: the same planner on the host, no GPU)
what plan its environment gives and asserts that it is the one the case is for: three tiers, four tiers, a ragged last
chunk, the bottom chunk early or not.  A case whose precondition does not hold fails.

The grid has 157 rows and 701 columns (700 for conway_packed: words of four cells): an odd width and a multiple of
four, both wide enough that the widest kernels (256-cell strips, 16 halo columns) have a strip that touches neither
side edge, and with 16-row chunks there are chunks 16 rows away from the top and the bottom, so that the check-free
code runs.  Row ranges: the whole grid, (23, 131) and (60, 157) -- the last one reaches the last rows, where
last_chunk_early applies -- with the whole grid in the source buffers, and (23, 131) again as a row band: the buffers
hold rows 23 - G ... 131 + G only, row_origin is not 0 and the pitch is larger than the width.  Every compiled depth
of the function runs.  The destination planes are filled with a sentinel (a NaN with a payload for float planes, 0xA5
for the Game of Life); afterwards the rows of the range equal the oracle's bits and every other byte -- rows outside,
the padding beyond the width, the rows of a hole -- still is the sentinel.

Coverage rule: the cases are capi.list_apps().  A registered name without a workload in tests/sweep_workloads.py fails
the tests that carry its name.  NO_ORACLE lists names whose launches are compared with their own one-chunk launch
because the oracle has no routine for them (at most two; none today).

What these cases found: jacobi5general_fma, the build with fused multiply-adds, depended on the plan.  With
-ffp-contract=fast the compiler picked per kernel instantiation which product of c0*N + c1*W it fused, and the
check-free code, the edge code and the stages of the default shape are instantiations of their own: on this grid 1319
to 6941 of 110 057 cells differed from the oracle built with fused multiply-adds (at most 3 ulp) under every plan but
`narrow`, and the plans differed from each other.  The functor spells the fusion out since (csrc/apps/jacobi.hpp, the
order gcc gives the oracle's fused build): every plan at every depth equals that oracle bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from mesh_threads import split_planes
from pass_schedule import halvings
from sweep_workloads import UNIFORM_CHAIN, LaunchWorkload

pytestmark = pytest.mark.gpu

PLAN_TOOL = os.path.join(ROOT, "build", "tests", "launch_plan_test")
H, W_ODD, W_FOURS = 157, 701, 700
RANGES = {"whole": (0, 157), "middle": (23, 131), "bottom": (60, 157)}
BAND = RANGES["middle"]
PAD = 11  # elements between the width and the pitch of a padded buffer

NO_ORACLE = ()  # (name, reason) pairs; at most two
assert len(NO_ORACLE) <= 2

KNOBS = ("STSTHIP_CHUNK_ROWS", "STSTHIP_TAPER", "STSTHIP_LAST_CHUNK_EARLY", "STSTHIP_XCD_REMAP", "STSTHIP_TAIL_PERMILLE",
         "STSTHIP_NARROW_FORM_KCELLS", "STSTHIP_NARROW_BAND_ROWS")
WIDE = {"STSTHIP_NARROW_FORM_KCELLS": "0"}
THREE = dict(WIDE, STSTHIP_CHUNK_ROWS="16", STSTHIP_TAPER="500:2,250:4")
FOUR = dict(WIDE, STSTHIP_CHUNK_ROWS="40", STSTHIP_TAPER="600:2,300:4,150:8")
PLANS = {
    "default": WIDE,                                                                       # the model's own plan
    "three-tiers": THREE,                                                                  # tiers of 16 / 8 / 4 rows
    "four-tiers": FOUR,                                                                    # 40 / 20 / 10 / 5 on 157 and 108 rows
    "sevens": dict(WIDE, STSTHIP_CHUNK_ROWS="7", STSTHIP_TAPER="", STSTHIP_LAST_CHUNK_EARLY="0"),  # ragged end, natural order
    "single-rows": dict(WIDE, STSTHIP_CHUNK_ROWS="1"),                                     # shorter than a stage's batch
    "one-chunk": dict(WIDE, STSTHIP_CHUNK_ROWS="1000000", STSTHIP_TAPER=""),               # a single unit per strip
    "three-tiers-xcd": dict(THREE, STSTHIP_XCD_REMAP="1"),                                 # tiers no longer dispatched last
    "four-tiers-xcd": dict(FOUR, STSTHIP_XCD_REMAP="1", STSTHIP_LAST_CHUNK_EARLY="0"),
    "thin-tail": dict(WIDE, STSTHIP_TAIL_PERMILLE="50", STSTHIP_XCD_REMAP="1"),            # the model with other weights
    "fat-tail": dict(WIDE, STSTHIP_TAIL_PERMILLE="2000", STSTHIP_XCD_REMAP="1"),
    "narrow": {k: v for k, v in THREE.items() if k != "STSTHIP_NARROW_FORM_KCELLS"},       # the one-cell-per-lane form
}


def registered():
    from stencilstream_amd import capi

    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return [name for name in capi.list_apps() if not name.startswith("x_")]  # (x_: experiments of an EXPERIMENTS=1 build)


APPS = registered()


def has_narrow_form(info, app):
    """has_narrow_form of Sweep.hpp: the default shape holds several cells per lane, explicit shapes (the registered
    independent-wave ones) are launched as they are, and a narrow wave must still produce sixteen lanes of columns."""
    k = 1
    while k < info.stencil_radius:
        k *= 2
    g = info.halo_depth_per_generation * info.max_generations
    return (not app.endswith("_independent") and info.cells_per_lane > k
            and 64 * k - 2 * ((g + k - 1) // k * k) >= 16 * k)


_workloads, _plans, _references = {}, {}, {}


def workload(oracle, app):
    if app not in _workloads:
        _workloads[app] = LaunchWorkload(oracle, app, (H, W_FOURS // 4 if app == "conway_packed" else W_ODD))
    return _workloads[app]


def use_plan(monkeypatch, env):
    """The environment of a plan, and the library's options re-read from it."""
    from stencilstream_amd import capi

    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    for knob, value in env.items():
        monkeypatch.setenv(knob, value)
    capi.reload_options()
    o = capi.options()
    assert o.chunk_rows == int(env.get("STSTHIP_CHUNK_ROWS", 0))
    assert o.n_taper == (len(env["STSTHIP_TAPER"].split(",")) if env.get("STSTHIP_TAPER") else
                         (0 if "STSTHIP_TAPER" in env else -1))
    if o.n_taper > 0:
        spec = [tuple(int(v) for v in entry.split(":")) for entry in env["STSTHIP_TAPER"].split(",")]
        assert [(o.taper_permille[i], o.taper_split[i]) for i in range(o.n_taper)] == spec
    assert o.xcd_remap == int(env.get("STSTHIP_XCD_REMAP", 0))
    assert o.last_chunk_early == int(env.get("STSTHIP_LAST_CHUNK_EARLY", 1))
    assert o.tail_permille == int(env.get("STSTHIP_TAIL_PERMILLE", 0))
    assert o.narrow_form_kcells == int(env.get("STSTHIP_NARROW_FORM_KCELLS", 6000)) and o.narrow_band_rows == 0


def stages_at(info, depth):
    w = max(int(info.stages), 1)
    while (depth * info.n_subiterations) % w:
        w -= 1
    return w


def plan_of(env, info, depth, a, b):
    """What `launch_plan_test plan` prints for rows [a, b) of the grid under `env` (a process of its own: opens no GPU)."""
    g = depth * info.halo_depth_per_generation
    stages = stages_at(info, depth)
    overhead = 2 * g + (stages - 1) * info.prefetch_rows
    key = (tuple(sorted(env.items())), a, b, g, overhead, stages > 1)
    if key not in _plans:
        if not os.path.exists(PLAN_TOOL):
            pytest.fail("build/tests/launch_plan_test missing: run __graft_entry__.build()")
        clean = {k: v for k, v in os.environ.items() if k not in KNOBS}
        out = subprocess.run([PLAN_TOOL, "plan", str(a), str(b), str(H), str(g), str(overhead), "2",
                              "1" if stages > 1 else "4"], env=dict(clean, **env), capture_output=True, timeout=60)
        assert out.returncode == 0, (out.stdout + out.stderr).decode()
        _plans[key] = json.loads(out.stdout)
    return _plans[key]


def assert_precondition(plan_id, env, info, depth, where, a, b):
    """The plan of this launch is the one the case is for."""
    plan = plan_of(env, info, depth, a, b)
    rows = [t[1] for t in plan["tiers"]]
    what = f"{plan_id} {where} ({a}, {b}) depth {depth}: {plan}"
    # tiers tile the range in the order of their tables
    assert plan["tiers"][0][2] == a and plan["tiers"][0][0] == 0, what
    early_wanted = env.get("STSTHIP_LAST_CHUNK_EARLY", "1") == "1" and b == H
    assert plan["last_chunk_early"] == int(early_wanted), what
    if where == "bottom" and "STSTHIP_LAST_CHUNK_EARLY" not in env:
        assert plan["last_chunk_early"] == 1, what
    if where == "middle":
        assert plan["last_chunk_early"] == 0, what
    assert plan["xcd_remap"] == int(env.get("STSTHIP_XCD_REMAP", "0")), what
    if plan_id in ("three-tiers", "three-tiers-xcd", "narrow"):
        assert rows == [16, 8, 4], what
    elif plan_id in ("four-tiers", "four-tiers-xcd"):
        if b - a in (157, 108):
            assert rows == [40, 20, 10, 5], what
        else:  # 97 rows: the first entry's tier would start at row 0 and is skipped
            assert len(rows) >= 3 and rows[0] == 40 and rows[-1] == 5, what
    elif plan_id == "sevens":
        assert rows == [7] and plan["n_chunks"] == -(-(b - a) // 7) and (b - a) % 7 != 0, what
        assert b - a != 157 or plan["n_chunks"] == 23, what
    elif plan_id == "single-rows":
        assert rows == [1] and plan["n_chunks"] == b - a, what
    elif plan_id == "one-chunk":
        assert rows == [b - a] and plan["n_chunks"] == 1, what
    if plan_id in ("three-tiers", "four-tiers", "three-tiers-xcd", "narrow") and plan["last_chunk_early"]:
        assert plan["n_chunks"] >= 3, what  # the permutation of entry() engages
    return plan


def tiled(sentinel, rows, row_bytes):
    assert row_bytes % len(sentinel) == 0
    return np.resize(sentinel, rows * row_bytes).reshape(rows, row_bytes).copy()


def padded(plane, pitch, size, sentinel):
    """`plane` (rows x width * size bytes) in rows of `pitch` elements; the padding holds the sentinel."""
    out = tiled(sentinel, plane.shape[0], pitch * size)
    out[:, :plane.shape[1]] = plane
    return out


def sweep(w, app, src_planes, depth, a, b, lo, hi, pitch, iteration, hole=None):
    """One launch of rows [a, b) from buffers that hold rows [lo, hi) in rows of `pitch` elements; returns the
    destination planes as bytes (rows x pitch * size), which were all sentinel before."""
    import torch

    from stencilstream_amd import capi

    info = capi.app_info(app)
    sizes = [info.plane_elem_size[p] for p in range(info.n_planes)]
    width = w.shape[1]
    src = [torch.from_numpy(padded(plane[lo:hi], pitch, size, w.sentinel) if plane.shape[1] == width * size
                            else np.ascontiguousarray(plane[lo:hi])).cuda() for plane, size in zip(src_planes, sizes)]
    dst = [torch.from_numpy(tiled(w.sentinel, hi - lo, pitch * size)).cuda() for size in sizes]
    for t, size in zip(src, sizes):
        assert tuple(t.shape) == (hi - lo, pitch * size)
    dom = capi.Domain(H, width, lo, hi - lo, pitch)
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()  # (the library's launch is not ordered with torch's copies above)
    if hole is not None:
        capi.check(capi.load().ststhip_set_launch_row_hole(hole[0], hole[1]), "set hole")
    try:
        capi.app_sweep(app, w.params, w.halo, dom, [t.data_ptr() for t in src], [t.data_ptr() for t in dst], a, b,
                       iteration, depth, stream)
    finally:
        if hole is not None:
            capi.check(capi.load().ststhip_set_launch_row_hole(0, 0), "reset hole")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in dst]


def assert_rows(w, info, got, want_planes, a, b, lo, hi, pitch, what, hole=None):
    """Rows [a, b) (without the hole) of `got` are `want_planes`' bits; every other byte still is the sentinel."""
    width = w.shape[1]
    for p, (plane, want) in enumerate(zip(got, want_planes)):
        size = info.plane_elem_size[p]
        expect = tiled(w.sentinel, hi - lo, pitch * size)
        expect[a - lo:b - lo, :width * size] = want[a:b, :width * size]
        if hole is not None:
            expect[hole[0] - lo:hole[1] - lo] = tiled(w.sentinel, hole[1] - hole[0], pitch * size)
        if not np.array_equal(plane, expect):
            bad = np.argwhere(plane != expect)
            r, c = int(bad[0][0]), int(bad[0][1])
            bad_rows = sorted({int(x) + lo for x in bad[:, 0]})
            inside = a <= r + lo < b and c < width * size and not (hole and hole[0] <= r + lo < hole[1])
            raise AssertionError(
                f"{what}, plane {p}: {len(bad)} bytes differ in {len(bad_rows)} rows ({bad_rows[:12]} ...), the first in "
                f"row {r + lo}, element {c // size}: " +
                ("a row of the range differs from the oracle" if inside else "a byte outside the range was written"))


def reference_planes(w, info, depth, monkeypatch, oracle):
    """The planes every plan must reproduce at this depth: the oracle's, once per (function, depth) -- or, for the
    fused-multiply-add build on a CPU without FMA and for the names of NO_ORACLE, the function's own one-chunk launch."""
    key = (w.app, depth)
    if key not in _references:
        own = w.app in [name for name, _ in NO_ORACLE] or (w.fma and not oracle.cpu_has_fma())
        if own:
            use_plan(monkeypatch, PLANS["one-chunk"])
            _references[key] = [plane[:, :w.shape[1] * info.plane_elem_size[p]] for p, plane in enumerate(
                sweep(w, w.app, split_planes(info, w.cells), depth, 0, H, 0, H, w.shape[1], w.offset))]
        else:
            _references[key] = split_planes(info, w.want(depth))
    return _references[key]


def plans_for(app):
    from stencilstream_amd import capi

    narrow = has_narrow_form(capi.app_info(app), app)
    return [plan_id for plan_id in PLANS if plan_id != "narrow" or narrow]


CASES = [pytest.param(app, plan_id, id=f"{app}-{plan_id}") for app in APPS for plan_id in plans_for(app)]


@pytest.mark.parametrize("app,plan_id", CASES)
def test_single_launches_under_a_plan(gpu, oracle, monkeypatch, app, plan_id):
    from stencilstream_amd import capi

    w = workload(oracle, app)
    info, env = w.info, PLANS[plan_id]
    width = w.shape[1]
    depths = sorted(halvings(info.max_generations), reverse=True)
    if app in UNIFORM_CHAIN:
        # product-carrying kernels: first -> middle -> last as three whole-grid launches (raw values in and out), the
        # kernel of this case under the plan, the two others under the model's own plan; compared after the last one
        for depth in depths:
            assert_precondition(plan_id, env, info, depth, "whole", 0, H)
            planes = split_planes(info, w.cells)
            for step, link in enumerate(UNIFORM_CHAIN):
                use_plan(monkeypatch, env if link == app else PLANS["default"])
                planes = sweep(w, link, planes, depth, 0, H, 0, H, width + PAD, step * depth)
            assert_rows(w, info, planes, split_planes(info, w.want(3 * depth)), 0, H, 0, H, width + PAD,
                        f"{app} {plan_id} depth {depth}: the chain of three launches")
        return
    for depth in depths:
        want = reference_planes(w, info, depth, monkeypatch, oracle)
        use_plan(monkeypatch, env)
        source = split_planes(info, w.cells)
        for where, (a, b) in RANGES.items():
            assert_precondition(plan_id, env, info, depth, where, a, b)
            got = sweep(w, app, source, depth, a, b, 0, H, width, w.offset)
            assert_rows(w, info, got, want, a, b, 0, H, width, f"{app} {plan_id} depth {depth} rows ({a}, {b})")
        # the middle range again as a row band: the buffers hold its rows and the ghost rows only
        g = depth * info.halo_depth_per_generation
        a, b = BAND
        lo, hi = max(0, a - g), min(H, b + g)
        assert lo > 0
        got = sweep(w, app, source, depth, a, b, lo, hi, width + PAD, w.offset)
        assert_rows(w, info, got, want, a, b, lo, hi, width + PAD, f"{app} {plan_id} depth {depth} band ({a}, {b})")
    assert capi.launch_row_hole() == (0, 0)


def holes(g):
    """The three bands of test_sweep_with_a_row_hole (tests/test_parity_gpu.py) on this grid: a strip's two boundary
    bands of g rows each, nearly the whole grid as a hole, bands of one row."""
    a, b = BAND
    return ((a, b, (a + g, b - g)), (0, H, (13, H - 10)), (60, 100, (61, 99)))


@pytest.mark.parametrize("app", ["hotspot", "fdtd_coef_grouped", "conway_packed", "selfcheck2"])
def test_row_hole_under_three_tiers_and_xcd_remap(gpu, oracle, monkeypatch, app):
    """ststhip_set_launch_row_hole (the two boundary bands of a row strip as one launch) for kernels other than
    jacobi5general, with 16-row chunks and renumbered workgroups: the rows on both sides equal the oracle, the rows of
    the hole and outside the range keep the sentinel."""
    w = workload(oracle, app)
    info, env = w.info, PLANS["three-tiers-xcd"]
    for depth in sorted(halvings(info.max_generations), reverse=True):
        want = reference_planes(w, info, depth, monkeypatch, oracle)
        use_plan(monkeypatch, env)
        for a, b, hole in holes(depth * info.halo_depth_per_generation):
            assert a < hole[0] < hole[1] < b
            got = sweep(w, app, split_planes(info, w.cells), depth, a, b, 0, H, w.shape[1] + PAD, w.offset, hole=hole)
            assert_rows(w, info, got, want, a, b, 0, H, w.shape[1] + PAD,
                        f"{app} depth {depth} rows ({a}, {b}) without {hole}", hole=hole)


def test_every_registered_name_has_a_workload(gpu, oracle):
    """The coverage rule, in one place: a name of capi.list_apps() that tests/sweep_workloads.py does not know."""
    from stencilstream_amd import capi

    missing = []
    for name in capi.list_apps():
        if name.startswith("x_"):
            continue
        try:
            workload(oracle, name)
        except KeyError:
            missing.append(name)
    assert not missing, missing
    assert sorted(APPS) == sorted(n for n in capi.list_apps() if not n.startswith("x_"))

"""ststhip_grid_relax on the device against numpy, operation by operation in the element's dtype: the model of
tests/test_grid_relax_cpu.py (colour masks over an array padded with the halo; checked there on a case worked by hand,
and shown to change bits when a product-sum is fused).

The comparison is special_values.assert_same_cells over the rectangle -- NaNs in exactly the same cells, every other
cell equal AS BITS, the cells of the inactive colour among them -- and bytes everywhere else.  The buffers are
test_grid_algebra_gpu's: guards in front of and behind the grid, a byte pattern everywhere but in the float members, and
after every call the WHOLE buffer is compared with the host's model: cells outside the rectangle, other members, the
pitch padding and both guards keep their bytes.

The shapes follow from the constants of csrc/relax.hip, which the test reads from the source: a lane of the dense
kernel owns a unit of 16, 8 or 4 bytes, a wave covers relax_wave units, a workgroup walks down relax_chunk_rows rows;
the general kernel takes relax_segment_cells columns of a row per workgroup.  Planes run with and without
STSTHIP_RELAX_GENERAL, which sends them to the general kernel."""
import numpy as np
import pytest
import torch

import large_extents as LE
import special_values as SV
from test_grid_algebra_gpu import Buffer, cell_buffer, combine_model, plane, prolong_model, restrict_model
from test_grid_relax_cpu import (H2, MAX_SWEEPS, MINUS_A, PH, PW, cross_model, poisson_f, poisson_tolerance, red_black,
                                 relax_model, sor)

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype("<f4"), np.dtype("<f8")
# five distinct weights, no symmetry: a swapped tap shows
FIVE = [-0.23, 0.41, -0.53, 0.67, -0.83]

K = LE.kernel_constants("relax.hip")
WAVE, THREADS, CHUNK, SEGMENT = K["relax_wave"], K["relax_threads"], K["relax_chunk_rows"], K["relax_segment_cells"]
assert (WAVE, THREADS, CHUNK, SEGMENT) == (64, 256, 32, 2048)


def widest(dtype):
    """Elements of the widest unit: 4 f32 or 2 f64."""
    return 16 // dtype.itemsize


@pytest.fixture(params=["dense", "general"])
def path(request, monkeypatch):
    """Which kernel planes take."""
    if request.param == "general":
        monkeypatch.setenv("STSTHIP_RELAX_GENERAL", "1")
    else:
        monkeypatch.delenv("STSTHIP_RELAX_GENERAL", raising=False)
    return request.param


# ------------------------------------------------------------------ calls with their model
def relax(u, offset, dtype, cross, n_rows, n_cols, at=(0, 0), halo=0.0, rhs=None, rhs_coef=1.0, first_colour=0,
          half_sweeps=2, parity=0):
    """rhs: (buffer, offset, (row, col)).  Returns (description, what the rectangle must hold)."""
    from stencilstream_amd import capi

    view = u.field(offset, dtype)[:u.height, :u.width]
    assert at[0] + n_rows <= u.height and at[1] + n_cols <= u.width, "the rectangle leaves the view"
    f, f_view, f_at = None, None, (0, 0)
    if rhs is not None:
        buf, off, f_at = rhs
        f = buf.field(off, dtype)[:buf.height, :buf.width][f_at[0]:f_at[0] + n_rows, f_at[1]:f_at[1] + n_cols].copy()
        assert f.shape == (n_rows, n_cols), "the rectangle leaves the right-hand side's view"
        f_view = buf.view(off)
    after = relax_model(dtype, cross, view, at, n_rows, n_cols, halo, first_colour, half_sweeps, parity, f, rhs_coef)
    rows, cols = slice(at[0], at[0] + n_rows), slice(at[1], at[1] + n_cols)
    kept = after.copy()
    kept[rows, cols] = view[rows, cols]
    assert kept.tobytes() == view.tobytes(), "the model changed a cell outside the rectangle"
    desc = capi.grid_relax_desc(u.view(offset), dtype.str, cross, n_rows, n_cols, at, halo, f_view, rhs_coef, f_at,
                                first_colour, half_sweeps, parity)
    return desc, after[rows, cols]


def run(u, offset, dtype, cross, n_rows, n_cols, at=(0, 0), halo=0.0, rhs=None, rhs_coef=1.0, first_colour=0, half_sweeps=2,
        parity=0, what="relax"):
    from stencilstream_amd import capi

    desc, want = relax(u, offset, dtype, cross, n_rows, n_cols, at, halo, rhs, rhs_coef, first_colour, half_sweeps, parity)
    capi.grid_relax([desc])
    u.settle(offset, dtype, (at[0], at[0] + n_rows), (at[1], at[1] + n_cols), want, what)
    if rhs is not None and rhs[0] is not u:
        rhs[0].unchanged(f"{what}: the right-hand side")
    return want


def unit_of(dtype, u, u_at, n_rows, rhs=None, rhs_at=(0, 0)):
    """The unit the dense kernel takes, in bytes, for dense planes: the rule of csrc/relax.hip."""
    size = dtype.itemsize
    first = u.base + (u_at[0] * u.pitch + u_at[1]) * size
    apart = 16
    if rhs is not None:
        apart |= (first - (rhs.base + (rhs_at[0] * rhs.pitch + rhs_at[1]) * size)) % 16
        if n_rows > 1:
            apart |= (rhs.pitch * size) % 16
    if u.height > 1:
        apart |= (u.pitch * size) % 16
    return apart & -apart


# ------------------------------------------------------------------ planes: widths, heights, alignments
def layouts(dtype):
    """name -> (bytes of the unit, u's pitch as a function of the least pitch, elements rhs is shifted against u)."""
    per16 = widest(dtype)
    even = lambda least: -(-least // per16) * per16                      # rows 16 bytes apart
    half = lambda least: -(-least // per16) * per16 + per16 // 2         # rows 8 bytes apart (mod 16)
    odd = lambda least: least | 1
    out = {"16": (16, even, 0), "8 by the rows": (8, half, 0), "8 by the right-hand side": (8, even, per16 // 2),
           "odd pitch": (dtype.itemsize, odd, 1)}
    if dtype == F32:
        out["4 by the right-hand side"] = (4, even, 1)
    return out


@pytest.mark.parametrize("has_rhs", [False, True], ids=["plain", "rhs"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_planes_at_every_unit_and_span(gpu, path, dtype, has_rhs):
    """Whole views of 3 rows (the halo on all four sides) for every unit the dense kernel has -- the row distance and
    the shift of rhs against u pick it -- with u beginning 0, 1, 2 and 3 elements into its buffer (heads and tails of
    every length) and the widths 1, 2, 3, unit +- 1 and around a wave's span.  With an odd pitch the alignment of a row
    alternates and rhs is shifted by one element against u.  Then the inside of the same view, whose neighbours are
    cells."""
    seen = set()
    for name, (unit, pitch_of, rel) in layouts(dtype).items():
        if not has_rhs and "right-hand side" in name:
            continue
        per_unit = unit // dtype.itemsize
        span = WAVE * per_unit
        widths = sorted({1, 2, 3, widest(dtype) - 1, widest(dtype) + 1, span - 1, span, span + 1, 2 * span + 3} - {0})
        for number, width in enumerate(widths):
            shift = number % 4
            pitch = pitch_of(width + 5)
            seed = 1000 * unit + width
            u = plane(gpu, dtype, 3, pitch, seed, width=width, shift=shift)
            f = plane(gpu, dtype, 3, pitch, seed + 1, width=width, shift=shift + rel) if has_rhs else None
            got = unit_of(dtype, u, (0, 0), 3, f)
            assert got == unit, (name, got)
            seen.add(unit)
            halo = (0.0, 1.5, float("nan"))[number % 3]
            run(u, 0, dtype, FIVE, 3, width, halo=halo, rhs=(f, 0, (0, 0)) if has_rhs else None, rhs_coef=-0.3,
                first_colour=number % 2, half_sweeps=2 + number % 2,
                what=f"{path}: whole 3 x {width} view, {name}, shift {shift}, halo {halo}")
            if width >= 3:
                run(u, 0, dtype, FIVE, 1, width - 2, (1, 1), halo, rhs=(f, 0, (1, 1)) if has_rhs else None, rhs_coef=0.7,
                    parity=number % 2, what=f"{path}: inside of a 3 x {width} view, {name}")
    assert seen == ({16, 8, 4} if dtype == F32 else {16, 8})


@pytest.mark.parametrize("has_rhs", [False, True], ids=["plain", "rhs"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_planes_at_every_height(gpu, path, dtype, has_rhs):
    """Heights 1, 2, 3 and around one and two chunks of rows: warm-up rows and chunk seams, where a workgroup reads rows
    that its neighbour stores; span + 1 columns in 16-byte units (two waves and a tail).  Whole views, then rows
    1 .. h-1 of the same view from column 1 on (units of one element: the rectangle's rows begin 4 bytes further)."""
    width = WAVE * widest(dtype) + 1
    pitch = -(-(width + 2) // 4) * 4
    for number, height in enumerate([1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]):
        u = plane(gpu, dtype, height, pitch, 50 + height, width=width)
        f = plane(gpu, dtype, height + 1, pitch, 52 + height) if has_rhs else None
        halo = -2.5 if number % 2 == 0 else float("nan")
        assert unit_of(dtype, u, (0, 0), height, f, (1, 0)) == 16
        run(u, 0, dtype, FIVE, height, width, halo=halo, rhs=(f, 0, (1, 0)) if has_rhs else None, rhs_coef=0.25,
            half_sweeps=3, what=f"{path}: whole {height} x {width} view, halo {halo}")
        if height >= 3:
            run(u, 0, dtype, FIVE, height - 2, width - 1, (1, 1), halo, rhs=(f, 0, (0, 0)) if has_rhs else None,
                first_colour=1, what=f"{path}: rows 1 .. {height - 1} of a {height} x {width} view")


def test_colours_parities_and_counts(gpu, path):
    """u_row, u_col, parity and first_colour each 0 and 1, with 1, 2, 3 and 5 half-sweeps: which cells a half-sweep takes
    depends on the VIEW's coordinates, never on the rectangle."""
    u = plane(gpu, F32, 11, 76, seed=70, width=75)
    f = plane(gpu, F32, 11, 76, seed=71, width=75)
    for u_row in (0, 1):
        for u_col in (0, 1):
            for parity in (0, 1):
                for first_colour in (0, 1):
                    for half_sweeps in (1, 2, 3, 5):
                        run(u, 0, F32, FIVE, 9, 70, (u_row, u_col), 0.75, (f, 0, (1 - u_row, u_col)), 0.125, first_colour,
                            half_sweeps, parity,
                            f"{path}: at {(u_row, u_col)}, parity {parity}, colour {first_colour} first, {half_sweeps} half-sweeps")
    # one half-sweep of each colour is two half-sweeps
    a, b = plane(gpu, F64, 7, 40, seed=72), plane(gpu, F64, 7, 40, seed=72)
    run(a, 0, F64, FIVE, 7, 40, half_sweeps=2, first_colour=1, parity=1, what=f"{path}: two half-sweeps")
    run(b, 0, F64, FIVE, 7, 40, half_sweeps=1, first_colour=1, parity=1, what=f"{path}: the first")
    run(b, 0, F64, FIVE, 7, 40, half_sweeps=1, first_colour=0, parity=1, what=f"{path}: the second")
    assert a.model.tobytes() == b.model.tobytes()


@pytest.mark.parametrize("halo", [3.25, float("nan")], ids=["value", "nan"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_rectangles_at_each_border(gpu, path, dtype, halo):
    """Rectangles of a 40 x 150 view that touch exactly one border, two, all or none: outside the view the halo,
    outside the rectangle the view, which keeps its bytes."""
    u = plane(gpu, dtype, 40, 152, seed=31, width=150)
    f = plane(gpu, dtype, 40, 152, seed=33)
    rects = {"top": (0, 35, 4, 140), "bottom": (6, 40, 4, 140), "left": (3, 36, 0, 133), "right": (3, 36, 8, 150),
             "top left": (0, 2, 0, 2), "bottom right": (37, 40, 141, 150), "inside": (2, 37, 3, 148), "whole": (0, 40, 0, 150),
             "one cell inside": (4, 5, 5, 6), "its neighbour": (4, 5, 6, 7), "a corner cell": (39, 40, 0, 1),
             "a column": (0, 40, 149, 150), "a row": (39, 40, 0, 150)}
    for number, (name, (r0, r1, c0, c1)) in enumerate(rects.items()):
        has_rhs = number % 3 != 1
        run(u, 0, dtype, FIVE, r1 - r0, c1 - c0, (r0, c0), halo, rhs=(f, 0, (r0, c0)) if has_rhs else None, rhs_coef=0.5,
            first_colour=number % 2, half_sweeps=1 + number % 3, parity=(number // 2) % 2,
            what=f"{path}: the {name} of a 40 x 150 view, halo {halo}")
    # the right-hand side from another place
    run(u, 0, dtype, FIVE, 30, 100, (7, 13), halo, rhs=(f, 0, (5, 2)), rhs_coef=2.0, what=f"{path}: the right-hand side from elsewhere")


def test_more_rows_than_workgroups(gpu, path):
    """4100 x 5: more rows than a launch of the general kernel has workgroups, so a workgroup walks several rows; and
    129 chunks of the dense kernel."""
    for dtype in (F32, F64):
        u, f = plane(gpu, dtype, 4100, 8, seed=21, width=5), plane(gpu, dtype, 4100, 8, seed=22, width=5)
        run(u, 0, dtype, FIVE, 4100, 5, halo=0.5, rhs=(f, 0, (0, 0)), half_sweeps=3, what=f"{path}: 4100 x 5 planes")
    if path == "dense":
        cells = cell_buffer(gpu, "fdtd", 4100, 5, seed=25)
        run(cells, 8, F32, FIVE, 4100, 5, halo=1.0, rhs=(cells, 12, (0, 0)), half_sweeps=3, what="4100 x 5 members")


# ------------------------------------------------------------------ members of cells
@pytest.mark.parametrize("width", [1, 3, SEGMENT - 1, SEGMENT, SEGMENT + 1])
def test_members_of_cells(gpu, width):
    """temp and power of 8-byte cells, hz / hz_sum / db of 32-byte cells, doubles in 16-byte cells: the right-hand side
    another member of the same cells, a member of other cells, a plane.  The other members and the padding keep their
    bytes (Buffer.settle)."""
    hot = cell_buffer(gpu, "hotspot", 5, width + 2, seed=7 * width + 1, width=width + 1)
    run(hot, 0, F32, FIVE, 5, width + 1, halo=0.5, rhs=(hot, 4, (0, 0)), rhs_coef=-1.0, half_sweeps=3,
        what="hotspot: temp, rhs power")
    run(hot, 4, F32, FIVE, 3, width, (1, 1), float("nan"), first_colour=1, parity=1, what="hotspot: power on a rectangle")

    fdtd = cell_buffer(gpu, "fdtd", 4, width + 1, seed=7 * width + 3, width=width)
    p = plane(gpu, F32, 4, width + 4, seed=7 * width + 4, shift=1)
    run(fdtd, 8, F32, FIVE, 4, width, halo=-1.0, rhs=(fdtd, 28, (0, 0)), rhs_coef=0.25, what="fdtd: hz, rhs db")
    run(fdtd, 12, F32, FIVE, 4, width, rhs=(fdtd, 8, (0, 0)), half_sweeps=5, first_colour=1, what="fdtd: hz_sum, rhs hz")
    run(fdtd, 28, F32, FIVE, 3, width, (1, 0), 2.0, rhs=(p, 0, (0, 3)), what="fdtd: db, rhs a plane")
    run(p, 0, F32, FIVE, 4, width, (0, 2), rhs=(fdtd, 8, (0, 0)), half_sweeps=1, what="a plane, rhs hz")
    run(fdtd, 8, F32, FIVE, 4, width, rhs=(hot, 4, (1, 0)), parity=1, what="fdtd: hz, rhs a member of other cells")

    doubles = cell_buffer(gpu, "hotspot f64", 4, width + 1, seed=7 * width + 7, width=width)
    run(doubles, 0, F64, FIVE, 4, width, halo=float("nan"), rhs=(doubles, 8, (0, 0)), rhs_coef=1.0 / 3.0, half_sweeps=3,
        what="f64 pairs: member 0, rhs member 1")
    run(doubles, 8, F64, FIVE, 4, width, halo=0.125, first_colour=1, what="f64 pairs: member 1")


# ------------------------------------------------------------------ special values
def lay(dtype, kind):
    """(u, f, cross, the cell the kind is about): 12 x 134 planes' values."""
    h, w = 12, 134
    rng = np.random.default_rng(600 + len(kind))
    u = (2.0 * rng.random((h, w)) - 1.0).astype(dtype)
    f = (2.0 * rng.random((h, w)) - 1.0).astype(dtype)
    cross = list(FIVE)
    if kind == "inf":     # an infinite cell under a zero weight: 0 * inf is NaN, every tap is multiplied
        u[5, 70], cross[3] = np.inf, 0.0
    elif kind == "nan":
        u[5, 70] = np.nan
    elif kind == "tiny":
        u, f = SV.tiny((h, w), 61, dtype=dtype).astype(dtype), SV.tiny((h, w), 62, dtype=dtype).astype(dtype)
        cross = [w_ / 16 for w_ in FIVE]  # the sums stay around the smallest normal
    elif kind == "negzero":
        u, f = SV.negzero((h, w), dtype=dtype).astype(dtype), SV.negzero((h, w), dtype=dtype).astype(dtype)
        cross = [0.5, 0.25, 1.0, 0.25, 2.0]
    return u, f, cross


@pytest.mark.parametrize("kind", ["inf", "nan", "tiny", "negzero"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_special_values(gpu, path, dtype, kind):
    """inf under a zero weight gives NaN; a planted NaN spreads over three half-sweeps exactly as in the model; results
    below the smallest normal stay what they are; -0.0 stays -0.0."""
    values, rhs_values, cross = lay(dtype, kind)
    h, w = values.shape
    u = plane(gpu, dtype, h, w, seed=60, values=lambda shape, seed, dt: values)
    f = plane(gpu, dtype, h, w, seed=61, values=lambda shape, seed, dt: rhs_values)
    colour = (5 + 70) & 1  # of the planted cell
    if kind == "inf":
        want = run(u, 0, dtype, cross, h, w, first_colour=1 - colour, half_sweeps=1, what=f"{path}: inf under a zero weight")
        # the cell to the west has the infinite cell as its east tap, whose weight is zero; the three others turn infinite
        assert np.isnan(want[5, 69]) and np.isnan(want).sum() == 1, "0 * inf is NaN: every tap is multiplied"
        assert np.isinf(want[5, 71]) and np.isinf(want[4, 70]) and np.isinf(want[6, 70])
    elif kind == "nan":
        want = run(u, 0, dtype, cross, h, w, rhs=(f, 0, (0, 0)), first_colour=colour, half_sweeps=3, what=f"{path}: a NaN spreads")
        there = np.argwhere(np.isnan(want))
        assert len(there) == 13 and all(abs(r - 5) + abs(c - 70) <= 2 for r, c in there)
    elif kind == "tiny":
        want = run(u, 0, dtype, cross, h, w, halo=float(np.finfo(dtype).smallest_subnormal), rhs=(f, 0, (0, 0)),
                   rhs_coef=1.0 / 16, half_sweeps=3, what=f"{path}: subnormals")
        assert SV.classify(want)["subnormal"] > 0.1
    else:
        want = run(u, 0, dtype, cross, h, w, halo=-0.0, rhs=(f, 0, (0, 0)), rhs_coef=3.0, what=f"{path}: -0.0")
        assert np.signbit(want).all() and (want == 0).all()
        run(u, 0, dtype, [-w_ for w_ in cross], h, w, halo=-0.0, half_sweeps=1, what=f"{path}: -0.0 under negative weights")
    run(u, 0, dtype, cross, h - 2, w - 3, (1, 2), float("inf"), rhs=(f, 0, (0, 0)), rhs_coef=-1.0, half_sweeps=3, parity=1,
        what=f"{path}, {kind}: an infinite halo")


def test_weights_are_rounded_once_on_the_host(gpu, path):
    """0.1 is no float: the model multiplies by np.float32(0.1), and by 0.1 for doubles; a weight below the smallest
    float is a zero that is still multiplied."""
    for dtype in (F32, F64):
        u, f = plane(gpu, dtype, 5, 72, seed=3, width=70), plane(gpu, dtype, 5, 72, seed=4, width=70)
        for weight in (0.1, 1.0 / 3.0, -0.7, 1e-50, -0.0):
            run(u, 0, dtype, [weight] * 5, 5, 70, halo=0.1, rhs=(f, 0, (0, 0)), rhs_coef=weight, half_sweeps=3,
                what=f"{path}: weight {weight!r}")


# ------------------------------------------------------------------ several entries
@pytest.mark.parametrize("n", [2, 5, 8])
def test_several_entries_in_one_call(gpu, path, n):
    from stencilstream_amd import capi

    kinds = [F32 if k % 2 == 0 else F64 for k in range(n)]
    us = [plane(gpu, kinds[k], 6, 140 + k, seed=80 + k) for k in range(n)]
    fs = [plane(gpu, kinds[k], 6, 140 + k, seed=90 + k) for k in range(n)]
    made = []
    for k in range(n):
        rhs = (fs[k], 0, (0, 0)) if k % 3 != 1 else None
        made.append(relax(us[k], 0, kinds[k], FIVE, 6 - k % 3, 140 + k - k % 5, (k % 3, k % 5), float(k), rhs, 0.5, k % 2,
                          1 + k % 4, (k // 2) % 2))
    capi.grid_relax([desc for desc, _ in made])
    for k, (_, want) in enumerate(made):
        us[k].settle(0, kinds[k], (k % 3, 6), (k % 5, 140 + k), want, f"{path}: entry {k} of {n}")
    # disjoint tiles of ONE plane, one half-sweep: the colours of the tiles agree, and a neighbour in another tile is a
    # cell of the other colour, which nobody writes
    u = plane(gpu, F32, 16, 300, seed=100)
    whole = relax_model(F32, FIVE, u.field(0, F32), (0, 0), 16, 300, 1.0, 1, 1)
    tiles = [(r, c) for r in (0, 9) for c in (0, 75, 151, 225)][:n]
    tall, wide = {0: 9, 9: 7}, {0: 75, 75: 76, 151: 74, 225: 75}
    made = [relax(u, 0, F32, FIVE, tall[r], wide[c], (r, c), 1.0, None, 1.0, 1, 1) for r, c in tiles]
    capi.grid_relax([desc for desc, _ in made])
    torch.cuda.synchronize()
    got = u.device.cpu().numpy()
    for (r, c), (_, want) in zip(tiles, made):
        rows, cols = slice(r, r + tall[r]), slice(c, c + wide[c])
        SV.assert_same_cells(want, whole[rows, cols], "tiles compose: a neighbour outside the rectangle reads the view")
        there = u.field(0, F32, of=got)[rows, cols]
        SV.assert_same_cells(there, want, f"{path}: tile at {(r, c)}")
        u.field(0, F32)[rows, cols] = there
    assert np.array_equal(got, u.model), "bytes outside the tiles changed"


# ------------------------------------------------------------------ repeatability
def test_a_large_plane_three_times(gpu, path):
    """1500 x 1100 floats: several workgroups in both directions, chunk seams and wave seams everywhere, five
    half-sweeps; three runs from the same cells equal the model every time."""
    u = plane(gpu, F32, 1500, 1104, seed=200, width=1100)
    f = plane(gpu, F32, 1500, 1100, seed=201)
    first = u.model.copy()
    desc, want = relax(u, 0, F32, FIVE, 1500, 1100, halo=0.25, rhs=(f, 0, (0, 0)), rhs_coef=0.5, half_sweeps=5)
    from stencilstream_amd import capi

    for attempt in range(3):
        u.model[...] = first
        u.device.copy_(torch.from_numpy(first))
        capi.grid_relax([desc])
        u.settle(0, F32, (0, 1500), (0, 1100), want, f"{path}: run {attempt}")


# ------------------------------------------------------------------ update.Grid
@pytest.fixture(scope="module")
def poisson():
    """f, the tolerance, and per omega (sweeps, u) of the model's red-black SOR from zero."""
    f = poisson_f()
    return f, poisson_tolerance(f), {omega: red_black(f, omega) for omega in (1.0, 1.5)}


@pytest.mark.parametrize("omega", [1.0, 1.5])
def test_red_black_sor_through_update_grid(gpu, poisson, omega):
    """relax, apply_stencil and norms only: the loop stops at the model's sweep count with the model's bits."""
    from stencilstream_amd import update as U

    f_host, tolerance, solved = poisson
    count, want = solved[omega]
    f = U.Grid.from_numpy(f_host, device=gpu)
    u, r = U.Grid(PH, PW, "<f4", device=gpu), U.Grid(PH, PW, "<f4", device=gpu)
    sweeps = 0
    while sweeps < MAX_SWEEPS:
        u.relax(cross=sor(omega), rhs=f, rhs_coef=omega * H2 / 4)
        sweeps += 1
        r.apply_stencil(u, cross=MINUS_A, rhs=f)  # r = f - A u
        if r.norms()[None].max_abs <= tolerance:
            break
    print(f"omega {omega}: {sweeps} sweeps on the device, {count} in the model")
    assert sweeps == count
    got = u.to_numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("layout", ["planes", "cells"])
def test_a_two_grid_cycle_through_update_grid(gpu, layout):
    """Pre-smooth, residual, restrict, relax the coarse error from zero, prolong, correct, post-smooth: relax with
    apply_stencil, restrict_from, prolong_from and combine equals the numpy chain bit for bit; on planes, and with u and f
    as temp and power of HotSpot cells."""
    from stencilstream_amd import update as U

    h, w = 64, 96
    rng = np.random.default_rng(0x26D)
    u_host = (rng.random((h, w), dtype=np.float32) - 0.5).astype(F32)
    f_host = (200.0 * (rng.random((h, w), dtype=np.float32) - 0.5)).astype(F32)
    gs = sor(1.0)
    if layout == "planes":
        u, f, uf, ff = U.Grid.from_numpy(u_host, device=gpu), U.Grid.from_numpy(f_host, device=gpu), None, None
    else:
        cells = np.zeros((h, w), dtype=U.HOTSPOT_CELL)
        cells["temp"], cells["power"] = u_host, f_host
        u = f = U.Grid.from_numpy(cells, device=gpu)
        uf, ff = "temp", "power"
    r, e = U.Grid(h, w, "<f4", device=gpu), U.Grid(h, w, "<f4", device=gpu)
    rc, ec = U.Grid(h // 2, w // 2, "<f4", device=gpu), U.Grid(h // 2, w // 2, "<f4", device=gpu)

    u.relax(cross=gs, rhs=f, rhs_coef=H2 / 4, field=uf, rhs_field=ff, half_sweeps=4)
    r.apply_stencil(u, cross=MINUS_A, rhs=f, src_field=uf, rhs_field=ff)
    rc.restrict_from(r)
    ec.fill(0.0)
    ec.relax(cross=gs, rhs=rc, rhs_coef=4 * H2 / 4, half_sweeps=8, first_colour=1)
    e.prolong_from(ec)
    u.combine([(1.0, u, uf), (1.0, e)], field=uf)
    u.relax(cross=gs, rhs=f, rhs_coef=H2 / 4, field=uf, rhs_field=ff, half_sweeps=4, first_colour=1, rows=(1, h - 1), cols=(0, w - 2))

    m = relax_model(F32, gs, u_host, (0, 0), h, w, 0.0, 0, 4, 0, f_host, H2 / 4)
    m_r = cross_model(F32, MINUS_A, m, 0.0, f_host, 1.0)
    m_rc = restrict_model(F32, m_r)
    m_ec = relax_model(F32, gs, np.zeros((h // 2, w // 2), F32), (0, 0), h // 2, w // 2, 0.0, 1, 8, 0, m_rc, 4 * H2 / 4)
    m_e = prolong_model(F32, m_ec, (0, 0), h // 2, w // 2, 0.0)
    m = combine_model(F32, [1.0, 1.0], [m, m_e])
    m = relax_model(F32, gs, m, (1, 0), h - 2, w - 2, 0.0, 1, 4, 0, f_host[1:h - 1, 0:w - 2], H2 / 4)
    assert np.array_equal(r.to_numpy().view(np.uint32), m_r.view(np.uint32)), "the residual"
    assert np.array_equal(ec.to_numpy().view(np.uint32), m_ec.view(np.uint32)), "the coarse error"
    got = u.to_numpy()
    if layout == "cells":
        assert np.array_equal(got["power"].view(np.uint32), f_host.view(np.uint32)), "power changed"
        got = got["temp"]
    assert np.abs(m - u_host).max() > 1e-3, "the cycle moved nothing"
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), m.view(np.uint32))


# ------------------------------------------------------------------ rows 2^32 + 16 bytes apart
@pytest.mark.parametrize("kernel", ["dense", "general"])
def test_rows_beyond_four_gigabytes(gpu, monkeypatch, kernel):
    """Three rows 2^32 + 16 bytes apart, u and the right-hand side alike, behind the front guard of
    tests/large_extents.py: a row offset cut to 32 bits (or sign-extended from them) lands inside the allocation and
    shows as a wrong value or as a changed sentinel, not as a fault.  Coded values and dyadic weights: every product and
    every sum is exact.  The dense kernel takes 16-byte units with a head of three elements."""
    from stencilstream_amd import capi

    if kernel == "general":
        monkeypatch.setenv("STSTHIP_RELAX_GENERAL", "1")
    else:
        monkeypatch.delenv("STSTHIP_RELAX_GENERAL", raising=False)
    P, Q = LE.plane("P", 0, LE.P30 + 4, 3, 9000), LE.plane("Q", 1, LE.P30 + 4, 3, 9000)
    assert P.row_bytes == (1 << 32) + 16
    all_u, all_f = LE.Rect(P, 0, 0, 3, 9000), LE.Rect(Q, 0, 0, 3, 9000)
    LE.require(LE.arena_bytes(P) + LE.arena_bytes(Q) + (16 << 20))
    try:
        u, f = LE.Arena(gpu, P), LE.Arena(gpu, Q)
        u.put_coded(all_u)
        f.put_coded(all_f)
        rows, cols = np.indices((3, 9000))
        u_host, f_host = LE.code_of(0, rows, cols).astype(F32), LE.code_of(1, rows, cols).astype(F32)
        cross, coef, at, n_rows, n_cols = (-2.0, 1.0, -0.5, 2.0, 0.125), 0.25, (1, 5), 2, 8200
        want = relax_model(F32, cross, u_host, at, n_rows, n_cols, LE.HALO, 1, 2, 0, f_host[1:3, 5:8205], coef)
        capi.grid_relax([capi.grid_relax_desc(u.capi_view(P), "<f4", cross, n_rows, n_cols, at, LE.HALO, f.capi_view(Q), coef,
                                              at, 1, 2, 0)])
        torch.cuda.synchronize()
        got = u.cells(all_u).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{kernel}: rows 2^32 + 16 bytes apart"
        assert np.array_equal(f.cells(all_f).cpu().numpy(), f_host), "the right-hand side changed"
        u.clear(all_u)
        f.clear(all_f)
        u.assert_clean(f"{kernel}: u")
        f.assert_clean(f"{kernel}: the right-hand side")
        del u, f
    finally:
        LE.release(f"relax, {kernel}")

"""ststhip_grid_stencil on the device against numpy, operation by operation in the element's dtype: the source padded
with the halo, the taps of the shape in row-major order, `acc = T(w_first) * s_first`, then `acc = acc + T(w_k) * s_k`,
then `acc = acc + T(rhs_coef) * rhs` -- the formula of ststhip.h verbatim, under np.errstate(all="ignore").

The comparison is special_values.assert_same_cells: NaNs in exactly the same cells, every other cell equal AS BITS;
there is no tolerance anywhere.  The buffers are test_grid_algebra_gpu's: guards in front of and behind the grid, a byte
pattern everywhere but in the float members, and after every call the WHOLE buffer is compared with the host's model.

The shapes follow from the constants of csrc/stencil.hip, which the test reads from the source: a wave of the dense
kernel covers stencil_wave units of 16, 8 or 4 bytes, a workgroup stencil_threads of them, and walks down
stencil_chunk_rows rows; the general kernel takes stencil_segment_cells elements of a row per workgroup.  Planes run
with and without STSTHIP_STENCIL_GENERAL, which sends them to the general kernel: BOX9 through both kernels, CROSS5
(which has no dense kernel) through the general one twice."""
import os
import re

import numpy as np
import pytest
import torch

import special_values as SV
from conftest import ROOT
from test_grid_algebra_gpu import Buffer, cell_buffer, plane

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype("<f4"), np.dtype("<f8")
CROSS5, BOX9 = 0, 1
TAPS = {BOX9: [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)],
        CROSS5: [(-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)]}
# nine distinct weights, no symmetry: a swapped tap shows
NINE = [0.11, -0.23, 0.37, 0.41, -0.53, 0.67, 0.71, -0.83, 0.97]
WEIGHTS = {BOX9: NINE, CROSS5: [0.0 if k in (0, 2, 6, 8) else w for k, w in enumerate(NINE)]}


def kernel_constant(name):
    source = open(os.path.join(ROOT, "stencilstream_amd", "csrc", "stencil.hip")).read()
    return int(re.search(rf"constexpr unsigned {name} = (\d+)( \* stencil_threads)?;", source).group(1))


WAVE = kernel_constant("stencil_wave")                      # units of a wave's span
THREADS = kernel_constant("stencil_threads")                # units of a workgroup's span
CHUNK = kernel_constant("stencil_chunk_rows")               # rows a workgroup walks down
SEGMENT = kernel_constant("stencil_segment_cells") * THREADS  # elements of a row per workgroup, general kernel
assert (WAVE, THREADS, CHUNK, SEGMENT) == (64, 256, 32, 1024)


@pytest.fixture(params=["dense", "general"])
def path(request, monkeypatch):
    """Which kernel planes take."""
    if request.param == "general":
        monkeypatch.setenv("STSTHIP_STENCIL_GENERAL", "1")
    else:
        monkeypatch.delenv("STSTHIP_STENCIL_GENERAL", raising=False)
    return request.param


# ------------------------------------------------------------------ the model, operation by operation
def stencil_model(dtype, shape, weights, view, at, n_rows, n_cols, halo, rhs=None, rhs_coef=1.0):
    """view: the whole source view (height x width); the rectangle begins at `at`; rhs: its n_rows x n_cols values."""
    T = dtype.type
    padded = np.full((view.shape[0] + 2, view.shape[1] + 2), T(halo), dtype=dtype)
    padded[1:-1, 1:-1] = view
    r, q = at[0] + 1, at[1] + 1  # the rectangle in `padded`

    def s(a, b):
        return padded[r + a:r + a + n_rows, q + b:q + b + n_cols]

    with np.errstate(all="ignore"):
        taps = TAPS[shape]
        a, b = taps[0]
        acc = T(weights[3 * (a + 1) + (b + 1)]) * s(a, b)
        for a, b in taps[1:]:
            acc = acc + T(weights[3 * (a + 1) + (b + 1)]) * s(a, b)
        if rhs is not None:
            acc = acc + T(rhs_coef) * rhs
    assert acc.dtype == dtype and acc.shape == (n_rows, n_cols)
    return acc


def stencil(dst, dst_offset, src, src_offset, dtype, shape, weights, n_rows, n_cols, dst_at=(0, 0), src_at=(0, 0), halo=0.0,
            rhs=None, rhs_coef=1.0):
    """rhs: (buffer, offset, (row, col)).  Returns (description, what the rectangle must hold)."""
    from stencilstream_amd import capi

    view = src.field(src_offset, dtype)[:src.height, :src.width]
    assert src_at[0] + n_rows <= src.height and src_at[1] + n_cols <= src.width, "the rectangle leaves the source view"
    f, f_view, f_at = None, None, (0, 0)
    if rhs is not None:
        buf, off, f_at = rhs
        f = buf.field(off, dtype)[:buf.height, :buf.width][f_at[0]:f_at[0] + n_rows, f_at[1]:f_at[1] + n_cols].copy()
        f_view = buf.view(off)
    want = stencil_model(dtype, shape, weights, view, src_at, n_rows, n_cols, halo, f, rhs_coef)
    desc = capi.grid_stencil_desc(dst.view(dst_offset), src.view(src_offset), dtype.str, shape, weights, n_rows, n_cols,
                                  dst_at, src_at, halo, f_view, rhs_coef, f_at)
    return desc, want


def run(dst, dst_offset, src, src_offset, dtype, shape, weights, n_rows, n_cols, dst_at=(0, 0), src_at=(0, 0), halo=0.0,
        rhs=None, rhs_coef=1.0, what="stencil"):
    from stencilstream_amd import capi

    desc, want = stencil(dst, dst_offset, src, src_offset, dtype, shape, weights, n_rows, n_cols, dst_at, src_at, halo, rhs,
                         rhs_coef)
    capi.grid_stencil([desc])
    dst.settle(dst_offset, dtype, (dst_at[0], dst_at[0] + n_rows), (dst_at[1], dst_at[1] + n_cols), want, what)
    return want


def unit_of(dtype, n_rows, *sides):
    """The unit the dense kernel takes, in bytes: sides are (buffer, (row, col)) of dense planes."""
    first = [buf.base + (at[0] * buf.pitch + at[1]) * dtype.itemsize for buf, at in sides]
    apart = 16
    for address in first[1:]:
        apart |= (first[0] - address) % 16
    if n_rows > 1:
        for buf, _ in sides:
            apart |= (buf.pitch * dtype.itemsize) % 16
    return apart & -apart


def test_the_model_on_a_case_worked_by_hand():
    """3 x 3 view, the centre cell and a corner cell; BOX9 and CROSS5; halo 10."""
    view = np.arange(1, 10, dtype=F32).reshape(3, 3)
    w = [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert stencil_model(F32, BOX9, w, view, (1, 1), 1, 1, 10.0)[0, 0] == sum(k * k for k in range(1, 10))
    assert stencil_model(F32, CROSS5, w, view, (1, 1), 1, 1, 10.0)[0, 0] == 2 * 2 + 4 * 4 + 5 * 5 + 6 * 6 + 8 * 8
    # cell (0, 0): north-west, north, north-east, west and south-west are halo
    assert stencil_model(F32, BOX9, w, view, (0, 0), 1, 1, 10.0)[0, 0] == 10 * (1 + 2 + 3 + 4 + 7) + 5 * 1 + 6 * 2 + 8 * 4 + 9 * 5
    assert stencil_model(F32, CROSS5, w, view, (0, 0), 1, 1, 10.0, np.full((1, 1), 2, F32), 0.5)[0, 0] == 10 * (2 + 4) + 5 + 12 + 32 + 1


# ------------------------------------------------------------------ planes: widths, heights, alignments
def units(dtype):
    return (16, 8, 4) if dtype == F32 else (16, 8)


def span_widths(dtype, unit):
    """1, 2, 3 and w - 1, w, w + 1 for the columns a wave and a workgroup of the dense kernel cover with this unit."""
    per_unit = unit // dtype.itemsize
    edges = (WAVE * per_unit, THREADS * per_unit)
    return [1, 2, 3] + [w + d for w in edges for d in (-1, 0, 1)]


@pytest.mark.parametrize("has_rhs", [False, True], ids=["plain", "rhs"])
@pytest.mark.parametrize("shape", [CROSS5, BOX9], ids=["cross5", "box9"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_planes_at_every_unit_and_span(gpu, path, dtype, shape, has_rhs):
    """Whole views of 3 rows (the halo on all four sides, pitch > width) for every unit the dense kernel has -- the
    bases of dst, src and rhs shifted against each other pick it -- and the widths around a wave's and a workgroup's
    span; the destination's own shift (0..3 elements, i.e. 0, 4, 8, 12 bytes for floats) gives heads and tails of
    every length.  Then the inside of the same view, whose neighbours are cells."""
    per16 = 16 // dtype.itemsize
    seen = set()
    for unit in units(dtype):
        rel = {16: 0, 8: per16 // 2, 4: 1}[unit]  # elements between the bases that limit the unit
        for number, width in enumerate(span_widths(dtype, unit)):
            shift = number % per16
            pitch = -(-(width + 5) // per16) * per16  # rows 16 bytes apart in every plane
            seed = 1000 * unit + width
            dst = plane(gpu, dtype, 3, pitch, seed, width=width, shift=shift)
            # the source limits the unit where there is no right-hand side, else the right-hand side does
            src = plane(gpu, dtype, 3, pitch + per16, seed + 1, width=width, shift=shift + (0 if has_rhs else rel))
            f = plane(gpu, dtype, 3, pitch, seed + 2, width=width, shift=shift + rel) if has_rhs else None
            sides = [(dst, (0, 0)), (src, (0, 0))] + ([(f, (0, 0))] if has_rhs else [])
            assert unit_of(dtype, 3, *sides) == unit
            seen.add(unit)
            halo = (0.0, 1.5, float("nan"))[number % 3]
            rhs = (f, 0, (0, 0)) if has_rhs else None
            run(dst, 0, src, 0, dtype, shape, WEIGHTS[shape], 3, width, halo=halo, rhs=rhs, rhs_coef=-0.3,
                what=f"{path}: whole 3 x {width} view, unit {unit}, shift {shift}, halo {halo}")
            if width >= 3:
                run(dst, 0, src, 0, dtype, shape, WEIGHTS[shape], 1, width - 2, (1, 1), (1, 1), halo,
                    rhs=(f, 0, (1, 1)) if has_rhs else None, rhs_coef=0.7, what=f"{path}: inside of a 3 x {width} view")
            src.unchanged("a stencil's source")
    assert seen == set(units(dtype))


@pytest.mark.parametrize("has_rhs", [False, True], ids=["plain", "rhs"])
@pytest.mark.parametrize("shape", [CROSS5, BOX9], ids=["cross5", "box9"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_planes_at_every_height(gpu, path, dtype, shape, has_rhs):
    """Heights 1, 2, 3 and around one and two chunks of rows: warm-up rows and chunk seams; 70 columns (units and a
    tail).  Whole views with a non-zero halo and a NaN halo, then rows 1 .. h-1 of the same view from column 1 on."""
    for number, height in enumerate([1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1]):
        dst = plane(gpu, dtype, height, 72, 50 + height)
        src = plane(gpu, dtype, height, 76, 51 + height, width=70)
        f = plane(gpu, dtype, height + 1, 72, 52 + height) if has_rhs else None
        halo = -2.5 if number % 2 == 0 else float("nan")
        run(dst, 0, src, 0, dtype, shape, WEIGHTS[shape], height, 70, halo=halo, rhs=(f, 0, (1, 2)) if has_rhs else None,
            rhs_coef=0.25, what=f"{path}: whole {height} x 70 view, halo {halo}")
        if height >= 3:
            run(dst, 0, src, 0, dtype, shape, WEIGHTS[shape], height - 2, 69, (1, 0), (1, 1), halo,
                rhs=(f, 0, (0, 0)) if has_rhs else None, what=f"{path}: rows 1 .. {height - 1} of a {height} x 70 view")


@pytest.mark.parametrize("halo", [3.25, float("nan")], ids=["value", "nan"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_rectangles_at_each_border(gpu, path, dtype, halo):
    """Rectangles of a 40 x 150 view that touch exactly one border, two, all or none: outside the view the halo,
    outside the rectangle the view."""
    src = plane(gpu, dtype, 40, 152, seed=31, width=150)
    dst = plane(gpu, dtype, 40, 152, seed=32)
    f = plane(gpu, dtype, 40, 152, seed=33)
    rects = {"top": (0, 35, 4, 140), "bottom": (6, 40, 4, 140), "left": (3, 36, 0, 133), "right": (3, 36, 8, 150),
             "top left": (0, 2, 0, 2), "bottom right": (37, 40, 141, 150), "inside": (2, 37, 3, 148), "whole": (0, 40, 0, 150),
             "one cell inside": (4, 5, 5, 6), "a corner cell": (39, 40, 0, 1), "a column": (0, 40, 149, 150), "a row": (39, 40, 0, 150)}
    for number, (name, (r0, r1, c0, c1)) in enumerate(rects.items()):
        shape, has_rhs = (BOX9, CROSS5)[number % 2], number % 3 == 0
        run(dst, 0, src, 0, dtype, shape, WEIGHTS[shape], r1 - r0, c1 - c0, (r0, c0), (r0, c0), halo,
            rhs=(f, 0, (r0, c0)) if has_rhs else None, what=f"{path}: the {name} of a 40 x 150 view, halo {halo}")
    # a rectangle that lands elsewhere, with the right-hand side from a third place
    run(dst, 0, src, 0, dtype, BOX9, NINE, 30, 100, (7, 13), (2, 31), halo, rhs=(f, 0, (5, 2)), rhs_coef=2.0,
        what=f"{path}: a rectangle moved between the planes")


def test_more_rows_than_workgroups(gpu):
    """2051 x 3: more rows than the general kernel's launch has workgroups, so a workgroup walks several rows; and
    2051 x 70 through the dense kernel: 65 chunks."""
    for dtype in (F32, F64):
        x, y = plane(gpu, dtype, 2051, 5, seed=21, width=4), plane(gpu, dtype, 2051, 3, seed=22)
        run(y, 0, x, 0, dtype, BOX9, NINE, 2051, 3, (0, 0), (0, 1), 0.5, what="2051 x 3 planes")
        x, y = plane(gpu, dtype, 2051, 72, seed=23, width=70), plane(gpu, dtype, 2051, 72, seed=24)
        run(y, 0, x, 0, dtype, CROSS5, WEIGHTS[CROSS5], 2051, 70, halo=0.5, rhs=(y, 0, (0, 0)), what="2051 x 70 planes")
    cells = cell_buffer(gpu, "fdtd", 2051, 3, seed=25)
    run(cells, 8, cells, 28, F32, BOX9, NINE, 2051, 3, halo=1.0, rhs=(cells, 12, (0, 0)), what="2051 x 3 members")


# ------------------------------------------------------------------ members of cells
def pair_cells(device, height, pitch, seed, width=None):
    return Buffer(device, height, pitch, 8, seed, {0: F32, 4: F32}, width)  # {f32, f32}


def triple_cells(device, height, pitch, seed, width=None):
    return Buffer(device, height, pitch, 24, seed, {8: F64}, width)  # an f64 member at byte 8 of 24-byte cells


@pytest.mark.parametrize("width", [1, 3, SEGMENT - 1, SEGMENT, SEGMENT + 1])
@pytest.mark.parametrize("shape", [CROSS5, BOX9], ids=["cross5", "box9"])
def test_members_of_cells(gpu, shape, width):
    """Both members of {f32, f32} cells, hz at byte 8 of 32-byte cells, an f64 at byte 8 of 24-byte cells: src another
    member of the destination's cells, rhs the destination itself, rhs another member; members from and into planes.
    The other members and the padding keep their bytes (Buffer.settle)."""
    w = WEIGHTS[shape]
    pairs = pair_cells(gpu, 5, width + 2, seed=7 * width + 1, width=width + 1)
    other = pair_cells(gpu, 4, width + 3, seed=7 * width + 2)
    run(pairs, 0, pairs, 4, F32, shape, w, 5, width + 1, halo=0.5, what="pairs: member 1 into member 0")
    run(pairs, 4, pairs, 0, F32, shape, w, 3, width, (1, 1), (1, 1), rhs=(pairs, 4, (1, 1)), rhs_coef=-1.0,
        what="pairs: member 0 into member 1, rhs the destination")
    run(pairs, 0, other, 4, F32, shape, w, 4, width, (1, 0), (0, 2), float("nan"), rhs=(pairs, 4, (1, 0)),
        what="pairs: other cells into member 0, rhs another member")

    fdtd = cell_buffer(gpu, "fdtd", 4, width + 1, seed=7 * width + 3, width=width)
    p = plane(gpu, F32, 4, width + 4, seed=7 * width + 4, shift=1)
    run(fdtd, 8, fdtd, 28, F32, shape, w, 4, width, halo=-1.0, rhs=(fdtd, 8, (0, 0)), rhs_coef=0.25,
        what="fdtd: db into hz, rhs hz itself")
    run(fdtd, 12, fdtd, 8, F32, shape, w, 4, width, rhs=(fdtd, 28, (0, 0)), what="fdtd: hz into hz_sum, rhs another member")
    run(p, 0, fdtd, 8, F32, shape, w, 4, width, (0, 2), (0, 0), 2.0, what="fdtd: hz into a plane")
    run(fdtd, 8, p, 0, F32, shape, w, 3, width, (1, 0), (0, 3), rhs=(p, 0, (1, 1)), what="fdtd: a plane into hz")

    triple = triple_cells(gpu, 4, width + 1, seed=7 * width + 5, width=width)
    doubles = plane(gpu, F64, 4, width + 2, seed=7 * width + 6, shift=1)
    run(doubles, 0, triple, 8, F64, shape, w, 4, width, (0, 1), (0, 0), 0.125, what="triples: the member into a plane")
    run(triple, 8, doubles, 0, F64, shape, w, 4, width, (0, 0), (0, 1), rhs=(triple, 8, (0, 0)), rhs_coef=1.0 / 3.0,
        what="triples: a plane into the member, rhs the member itself")
    f64cells = cell_buffer(gpu, "hotspot f64", 4, width + 1, seed=7 * width + 7, width=width)
    run(f64cells, 0, f64cells, 8, F64, shape, w, 4, width, halo=float("nan"), rhs=(triple, 8, (0, 0)),
        what="f64 pairs: member 1 into member 0")


# ------------------------------------------------------------------ special values
@pytest.mark.parametrize("kind", ["planted", "tiny", "huge", "negzero"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_special_values(gpu, path, dtype, kind):
    """Subnormal, non-finite and signed-zero sources: products that underflow, sums that overflow, inf - inf, and a
    zero weight on an infinite cell, which is NaN in BOX9 -- every tap is multiplied -- and nothing in CROSS5, whose
    corners are not read."""
    make = {"planted": lambda shape, seed, dt: SV.planted(shape, seed, dtype=dt),
            "tiny": lambda shape, seed, dt: SV.tiny(shape, seed, dtype=dt),
            "huge": lambda shape, seed, dt: SV.huge(shape, seed, dtype=dt),
            "negzero": lambda shape, seed, dt: SV.negzero(shape, seed, dtype=dt)}[kind]
    h, w = 12, 134  # wider than 128, so that `planted` has its seam
    src = plane(gpu, dtype, h, w, seed=60, values=make)
    f = plane(gpu, dtype, h, w, seed=61, values=make)
    out = plane(gpu, dtype, h, w, seed=62)
    zero_corners = [0.0, 0.5, 0.0, -0.25, 1.0, 0.25, -0.0, 2.0, 0.0]  # the same weights serve both shapes
    wants = {}
    for shape in (BOX9, CROSS5):
        for halo in (0.0, float("inf"), float(np.finfo(dtype).smallest_subnormal)):
            wants[shape] = run(out, 0, src, 0, dtype, shape, zero_corners, h, w, halo=halo, what=f"{path}, {kind}: halo {halo}")
        run(out, 0, src, 0, dtype, shape, WEIGHTS[shape], h, w, halo=-0.0, rhs=(f, 0, (0, 0)), rhs_coef=-1.0,
            what=f"{path}, {kind}: with a right-hand side")
        run(out, 0, src, 0, dtype, shape, [0.1 * x for x in WEIGHTS[shape]], h, w, rhs=(out, 0, (0, 0)), rhs_coef=0.1,
            what=f"{path}, {kind}: small weights, rhs in place")
    if kind == "planted":
        r, c = SV.planted_sites((h, w))["+inf"][1]  # +inf at (r, c), -inf at (r, c + 1), inside the grid
        assert 0 < r < h - 1 and 1 < c and np.isposinf(src.field(0, dtype)[r, c])
        # the cell below and right of the pair sees the -inf in its north-west corner and nothing else that is special
        around = src.field(0, dtype)[r:r + 3, c + 1:c + 4].copy()
        assert np.isneginf(around[0, 0]) and np.isfinite(around.reshape(-1)[1:]).all()
        assert np.isnan(wants[BOX9][r + 1, c + 2]), "0 * inf is NaN: every tap of BOX9 is multiplied"
        assert np.isfinite(wants[CROSS5][r + 1, c + 2]), "CROSS5 does not touch its corners"
    if kind == "tiny":  # a result below the smallest normal stays what it is
        assert SV.classify(wants[CROSS5])["subnormal"] > 0.1
    members = cell_buffer(gpu, "fdtd" if dtype == F32 else "fdtd f64", h, w, seed=63, values=make)
    offsets = (8, 12, 28) if dtype == F32 else (0, 16, 24)
    for shape in (BOX9, CROSS5):
        run(members, offsets[0], members, offsets[1], dtype, shape, zero_corners, h, w, halo=float("inf"),
            rhs=(members, offsets[2], (0, 0)), what=f"{kind}: members")


def test_weights_are_rounded_once_on_the_host(gpu, path):
    """0.1 is no float: the model multiplies by np.float32(0.1), and by 0.1 for doubles; a weight below the smallest
    float is a zero that is still multiplied."""
    for dtype in (F32, F64):
        x, y = plane(gpu, dtype, 5, 70, seed=3), plane(gpu, dtype, 5, 70, seed=4)
        for weight in (0.1, 1.0 / 3.0, -0.7, 1e-50, -0.0):
            run(y, 0, x, 0, dtype, BOX9, [weight] * 9, 5, 70, halo=0.1, rhs=(x, 0, (0, 0)), rhs_coef=weight,
                what=f"weight {weight!r}")


# ------------------------------------------------------------------ several entries
@pytest.mark.parametrize("n", [2, 5, 8])
def test_several_entries_in_one_call(gpu, path, n):
    from stencilstream_amd import capi

    kinds = [F32 if k % 2 == 0 else F64 for k in range(n)]
    outs = [plane(gpu, kinds[k], 6, 140 + k, seed=80 + k) for k in range(n)]
    ins = [plane(gpu, kinds[k], 6, 140 + k, seed=90 + k) for k in range(n)]
    made = []
    for k in range(n):
        shape = (BOX9, CROSS5)[k % 2]
        rhs = (outs[k], 0, (k % 3, k % 5)) if k % 3 == 0 else None  # (the destination itself)
        made.append(stencil(outs[k], 0, ins[k], 0, kinds[k], shape, WEIGHTS[shape], 6 - k % 3, 140 + k - k % 5, (k % 3, k % 5),
                            (0, 0), float(k), rhs, 0.5))
    capi.grid_stencil([desc for desc, _ in made])
    for k, (_, want) in enumerate(made):
        outs[k].settle(0, kinds[k], (k % 3, 6), (k % 5, 140 + k), want, f"entry {k} of {n}")
    # disjoint rectangles of ONE plane, from one source
    src, dst = plane(gpu, F32, 16, 300, seed=100), plane(gpu, F32, 16, 300, seed=101)
    tiles = [(r, c) for r in (0, 8) for c in (0, 75, 150, 225)][:n]
    made = [stencil(dst, 0, src, 0, F32, BOX9, NINE, 8, 75, at, at, 1.0) for at in tiles]
    capi.grid_stencil([desc for desc, _ in made])
    torch.cuda.synchronize()
    whole = stencil_model(F32, BOX9, NINE, src.field(0, F32), (0, 0), 16, 300, 1.0)
    got = dst.device.cpu().numpy()
    for (r, c), (_, want) in zip(tiles, made):
        SV.assert_same_cells(want, whole[r:r + 8, c:c + 75], "tiles compose: a neighbour outside the rectangle reads the view")
        there = dst.field(0, F32, of=got)[r:r + 8, c:c + 75]
        SV.assert_same_cells(there, want, f"tile at {(r, c)}")
        dst.field(0, F32)[r:r + 8, c:c + 75] = there
    assert np.array_equal(got, dst.model), "bytes outside the tiles changed"


# ------------------------------------------------------------------ update.Grid
H, W, SWEEPS = 65, 63, 40
H2 = 1.0 / 4096.0  # h = 1 / 64
RELAX = (0.25, 0.25, 0.0, 0.25, 0.25)
MINUS_A = (1.0 / H2, 1.0 / H2, -4.0 / H2, 1.0 / H2, 1.0 / H2)  # A u = (4 u - N - W - E - S) / h^2


def cross_weights(cross):
    n, w, c, e, s = cross
    return [0.0, n, 0.0, w, c, e, 0.0, s, 0.0]


@pytest.fixture(scope="module")
def relaxed():
    """f, and u after 40 relaxations u <- 1/4 (N + W + E + S) + 1/4 h^2 f from zero with a zero halo: the numpy loop."""
    rng = np.random.default_rng(0x57E)
    f = (200.0 * (rng.random((H, W), dtype=np.float32) - 0.5)).astype(F32)
    u = np.zeros((H, W), dtype=F32)
    for _ in range(SWEEPS):
        u = stencil_model(F32, CROSS5, cross_weights(RELAX), u, (0, 0), H, W, 0.0, f, 0.25 * H2)
    return f, u


def test_relaxation_with_a_source_through_update_grid(gpu, relaxed):
    from stencilstream_amd import update as U

    f_host, want = relaxed
    f = U.Grid.from_numpy(f_host, device=gpu)
    a, b = U.Grid(H, W, "<f4", device=gpu), U.Grid(H, W, "<f4", device=gpu)
    for _ in range(SWEEPS):
        b.apply_stencil(a, cross=RELAX, rhs=f, rhs_coef=0.25 * H2)
        a, b = b, a
    got = a.to_numpy()
    assert np.abs(want).max() > 1e-3, "the relaxation moved nothing"
    SV.assert_same_cells(got, want, "40 relaxations")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_residual_through_update_grid(gpu, relaxed):
    from stencilstream_amd import update as U

    f_host, u_host = relaxed
    f, u = U.Grid.from_numpy(f_host, device=gpu), U.Grid.from_numpy(u_host, device=gpu)
    r = U.Grid(H, W, "<f4", device=gpu)
    r.apply_stencil(u, cross=MINUS_A, rhs=f)  # r = f - A u
    want = stencil_model(F32, CROSS5, cross_weights(MINUS_A), u_host, (0, 0), H, W, 0.0, f_host, 1.0)
    got = r.to_numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    norms = r.norms()[None]
    assert norms.n_nonfinite == 0 and norms.max_abs == float(np.abs(want).max())
    # the same as a box with zero corners, on members of cells and on an inner rectangle: the rest keeps its bytes
    cells = np.zeros((H, W), dtype=U.HOTSPOT_CELL)
    cells["temp"], cells["power"] = u_host, f_host
    grid = U.Grid.from_numpy(cells, device=gpu)
    out = U.Grid.from_numpy(cells, device=gpu)
    out.apply_stencil(grid, box=np.array(cross_weights(MINUS_A)).reshape(3, 3), rhs=out, field="power", src_field="temp",
                      rhs_field="power", rows=(1, H - 1), cols=(2, W))
    there = out.to_numpy()
    inner = stencil_model(F32, BOX9, cross_weights(MINUS_A), u_host, (1, 2), H - 2, W - 2, 0.0, f_host[1:H - 1, 2:W], 1.0)
    expect = f_host.copy()
    expect[1:H - 1, 2:W] = inner
    SV.assert_same_cells(there["power"], expect, "the residual on members")
    assert np.array_equal(there["temp"].view(np.uint32), u_host.view(np.uint32)), "temp changed"

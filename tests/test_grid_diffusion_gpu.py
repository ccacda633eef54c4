"""ststhip_grid_diffusion on the device against numpy, operation by operation in the element's dtype: the model of
tests/test_grid_diffusion_cpu.py, which is the formula of ststhip.h verbatim (u padded with the halo, kx and ky with
k_halo by their own extents, every product, sum, difference and quotient rounded once).

The comparison is special_values.assert_same_cells: NaNs in exactly the same cells, every other cell equal AS BITS;
there is no tolerance anywhere.  The buffers are test_grid_algebra_gpu's: guards in front of and behind the grid, a byte
pattern everywhere but in the float members, and after every call the WHOLE buffer of the destination is compared with
the host's model; the sources are checked unchanged.

The shapes follow from the constants of csrc/diffusion.hip, which the test reads from the source: a wave of the dense
kernel covers diffusion_wave units of 16, 8 or 4 bytes, a workgroup diffusion_threads of them, and walks down
diffusion_chunk_rows rows; the general kernel takes diffusion_segment_cells elements of a row per workgroup.  Planes run
as the library routes them ("routed": APPLY without a right-hand side through the dense kernel, every other mode through
the general one, which is all they have) and, APPLY without a right-hand side only, under STSTHIP_DIFFUSION_GENERAL,
which sends it to the general kernel too."""
import math

import numpy as np
import pytest
import torch

import large_extents as LE
import special_values as SV
from test_grid_algebra_gpu import Buffer, cell_buffer, plane
from test_grid_diffusion_cpu import (APPLY, JACOBI, SOLVE_DIAG, TOLERANCE, PH, PW, MAX_ITERATIONS, diffusion_model, pcg_model,
                                     pcg_problem, whole)

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype("<f4"), np.dtype("<f8")
MODES = {"apply": (APPLY, False), "apply with rhs": (APPLY, True), "jacobi": (JACOBI, True), "solve_diag": (SOLVE_DIAG, True)}
SCALARS = dict(sigma=0.3, scale=0.7, omega=0.8, rhs_coef=-0.3)

K = LE.kernel_constants("diffusion.hip")
WAVE, THREADS, CHUNK, SEGMENT = (K[f"diffusion_{name}"] for name in ("wave", "threads", "chunk_rows", "segment_cells"))
CAP = K["diffusion_block_cap"]  # workgroups of a launch
assert (WAVE, THREADS, CHUNK, SEGMENT, CAP) == (64, 256, 32, 1024, 2048)


@pytest.fixture(params=["routed", "general"])
def path(request, monkeypatch):
    """Which kernel planes take: the library's choice, or the general kernel for everything."""
    if request.param == "general":
        monkeypatch.setenv("STSTHIP_DIFFUSION_GENERAL", "1")
    else:
        monkeypatch.delenv("STSTHIP_DIFFUSION_GENERAL", raising=False)
    return request.param


def modes_on(path):
    """The modes a pass runs: all of them as the library routes planes; under the switch APPLY without a right-hand side
    alone, the one mode whose kernel the switch changes."""
    return sorted(MODES) if path == "routed" else ["apply"]


# every mode as the library routes it, and the one mode that has a second kernel through that one
ROUTES = [(mode, "routed") for mode in sorted(MODES)] + [("apply", "general")]


class Side:
    """A view of a buffer's member and where the rectangle begins in it."""

    def __init__(self, buf, offset=0, at=(0, 0)):
        self.buf, self.offset, self.at = buf, offset, at

    def values(self, dtype):
        return self.buf.field(self.offset, dtype)[:self.buf.height, :self.buf.width]

    def view(self):
        return self.buf.view(self.offset)


def side(x):
    return x if isinstance(x, Side) or x is None else Side(*x) if isinstance(x, tuple) else Side(x)


def diffuse(dtype, mode, dst, u, kx, ky, n_rows, n_cols, rhs=None, **scalars):
    """dst, u, kx, ky, rhs: a Buffer, (buffer, offset) or (buffer, offset, (row, col)).  Returns (description, what the
    rectangle must hold)."""
    from stencilstream_amd import capi

    dst, u, kx, ky, rhs = (side(x) for x in (dst, u, kx, ky, rhs))
    for s in (dst, u, kx, ky, rhs):
        if s is not None:
            assert s.at[0] + n_rows <= s.buf.height and s.at[1] + n_cols <= s.buf.width, "the rectangle leaves a view"
    f = None
    if rhs is not None:
        f = rhs.values(dtype)[rhs.at[0]:rhs.at[0] + n_rows, rhs.at[1]:rhs.at[1] + n_cols].copy()
    want = diffusion_model(dtype, mode, None if u is None else u.values(dtype), kx.values(dtype), ky.values(dtype), n_rows,
                           n_cols, (0, 0) if u is None else u.at, kx.at, ky.at, rhs=f, **scalars)
    desc = capi.grid_diffusion_desc(dst.view(), None if u is None else u.view(), kx.view(), ky.view(), dtype.str, mode,
                                    n_rows, n_cols, dst.at, (0, 0) if u is None else u.at, kx.at, ky.at,
                                    rhs=None if rhs is None else rhs.view(), rhs_at=(0, 0) if rhs is None else rhs.at,
                                    **scalars)
    return desc, want, dst


def run(dtype, mode, dst, u, kx, ky, n_rows, n_cols, rhs=None, what="diffusion", **scalars):
    from stencilstream_amd import capi

    desc, want, to = diffuse(dtype, mode, dst, u, kx, ky, n_rows, n_cols, rhs, **scalars)
    capi.grid_diffusion([desc])
    to.buf.settle(to.offset, dtype, (to.at[0], to.at[0] + n_rows), (to.at[1], to.at[1] + n_cols), want, what)
    for source in (u, kx, ky, rhs):
        source = side(source)
        if source is not None and source.buf is not to.buf:
            source.buf.unchanged(what)
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


def units(dtype):
    return (16, 8, 4) if dtype == F32 else (16, 8)


def span_widths(dtype, unit):
    """1, 2, 3 and w - 1, w, w + 1 for the columns a wave and a workgroup of the dense kernel cover with this unit."""
    per_unit = unit // dtype.itemsize
    edges = (WAVE * per_unit, THREADS * per_unit)
    return [1, 2, 3] + [w + d for w in edges for d in (-1, 0, 1)]


# ------------------------------------------------------------------ planes: modes, widths, heights, alignments
@pytest.mark.parametrize("mode,path", ROUTES, indirect=["path"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_planes_at_every_unit_and_span(gpu, path, dtype, mode):
    """Whole views of 3 rows (the halo on all four sides, pitch > width) for every unit the dense kernel has -- the
    base of kx, of ky or of rhs (of u where there is no right-hand side) shifted against the destination's picks it, in
    turn -- and the widths around a wave's and a workgroup's span; the destination's own shift (0..3 elements) gives
    heads and tails of every length.  Then the inside of the same views, whose neighbours are cells."""
    which, has_rhs = MODES[mode]
    per16 = 16 // dtype.itemsize
    seen = set()
    for unit in units(dtype):
        rel = {16: 0, 8: per16 // 2, 4: 1}[unit]  # elements between the bases that limit the unit
        for number, width in enumerate(span_widths(dtype, unit)):
            shift = number % per16
            pitch = -(-(width + 5) // per16) * per16  # rows 16 bytes apart in every plane
            seed = 1000 * unit + width
            limiting = ("kx", "ky", "rhs" if has_rhs else "u")[number % 3]
            if which == SOLVE_DIAG and limiting == "u":
                limiting = "ky"
            moved = {name: shift + (rel if name == limiting else 0) for name in ("u", "kx", "ky", "rhs")}
            dst = plane(gpu, dtype, 3, pitch, seed, width=width, shift=shift)
            u = plane(gpu, dtype, 3, pitch + per16, seed + 1, width=width, shift=moved["u"])
            kx = plane(gpu, dtype, 3, pitch, seed + 2, width=width, shift=moved["kx"])
            ky = plane(gpu, dtype, 3, pitch + 2 * per16, seed + 3, width=width, shift=moved["ky"])
            f = plane(gpu, dtype, 3, pitch, seed + 4, width=width, shift=moved["rhs"]) if has_rhs else None
            sides = [dst, kx, ky] + ([u] if which != SOLVE_DIAG else []) + ([f] if has_rhs else [])
            assert unit_of(dtype, 3, *[(s, (0, 0)) for s in sides]) == unit
            seen.add(unit)
            halo, k_halo = (0.0, 1.5, float("nan"))[number % 3], (1.0, 0.0, -2.5)[number % 3]
            source = None if which == SOLVE_DIAG else u
            run(dtype, which, dst, source, kx, ky, 3, width, f, halo=halo, k_halo=k_halo, **SCALARS,
                what=f"{path} {mode}: whole 3 x {width} view, unit {unit} by {limiting}, shift {shift}, halo {halo}")
            if width >= 3:
                inner = [(s, 0, (1, 1)) if s is not None else None for s in (dst, source, kx, ky, f)]
                run(dtype, which, inner[0], inner[1], inner[2], inner[3], 1, width - 2, inner[4], halo=halo, k_halo=k_halo,
                    **SCALARS, what=f"{path} {mode}: inside of a 3 x {width} view")
    assert seen == set(units(dtype))


@pytest.mark.parametrize("mode,path", ROUTES, indirect=["path"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_planes_at_every_height(gpu, path, dtype, mode):
    """Heights 1, 2, 3 and around one and two chunks of rows: the warm-up rows of u and the kn that is carried from row
    to row across a chunk's seam; 70 columns (units and a tail).  Whole views, then rows 1 .. h-1 of the same views."""
    which, has_rhs = MODES[mode]
    for number, height in enumerate([1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]):
        dst = plane(gpu, dtype, height, 72, 50 + height)
        u = None if which == SOLVE_DIAG else plane(gpu, dtype, height, 76, 51 + height, width=70)
        kx = plane(gpu, dtype, height, 72, 52 + height, width=70)
        ky = plane(gpu, dtype, height, 80, 53 + height, width=70)
        f = plane(gpu, dtype, height + 1, 72, 54 + height) if has_rhs else None
        halo = -2.5 if number % 2 == 0 else float("nan")
        run(dtype, which, dst, u, kx, ky, height, 70, (f, 0, (1, 2)) if has_rhs else None, halo=halo, k_halo=0.5, **SCALARS,
            what=f"{path} {mode}: whole {height} x 70 view, halo {halo}")
        if height >= 3:
            run(dtype, which, (dst, 0, (1, 0)), None if u is None else (u, 0, (1, 1)), (kx, 0, (1, 1)), (ky, 0, (1, 1)),
                height - 2, 69, (f, 0, (0, 0)) if has_rhs else None, halo=halo, k_halo=float("nan"), **SCALARS,
                what=f"{path} {mode}: rows 1 .. {height - 1} of a {height} x 70 view")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_rectangles_at_each_border(gpu, path, dtype):
    """Rectangles of 40 x 150 views that touch exactly one border, two, all or none: outside the view the halo and
    k_halo, outside the rectangle the view."""
    u = plane(gpu, dtype, 40, 152, seed=31, width=150)
    kx = plane(gpu, dtype, 40, 152, seed=32, width=150)
    ky = plane(gpu, dtype, 40, 156, seed=33, width=150)
    f = plane(gpu, dtype, 40, 152, seed=34)
    dst = plane(gpu, dtype, 40, 152, seed=35)
    rects = {"top": (0, 35, 4, 140), "bottom": (6, 40, 4, 140), "left": (3, 36, 0, 133), "right": (3, 36, 8, 150),
             "top left": (0, 2, 0, 2), "bottom right": (37, 40, 141, 150), "inside": (2, 37, 3, 148), "whole": (0, 40, 0, 150),
             "one cell inside": (4, 5, 5, 6), "a corner cell": (39, 40, 0, 1), "a column": (0, 40, 149, 150), "a row": (39, 40, 0, 150)}
    for number, (name, (r0, r1, c0, c1)) in enumerate(rects.items()):
        mode = sorted(MODES)[number % 4] if path == "routed" else "apply"
        which, has_rhs = MODES[mode]
        at = (r0, c0)
        run(dtype, which, (dst, 0, at), None if which == SOLVE_DIAG else (u, 0, at), (kx, 0, at), (ky, 0, at), r1 - r0,
            c1 - c0, (f, 0, at) if has_rhs else None, halo=3.25, k_halo=float("nan") if number % 2 else 0.75, **SCALARS,
            what=f"{path} {mode}: the {name} of a 40 x 150 view")
    # a rectangle that lands elsewhere, every side from another place
    run(dtype, APPLY, (dst, 0, (7, 13)), (u, 0, (2, 31)), (kx, 0, (9, 0)), (ky, 0, (0, 50)), 30, 100, halo=3.25, k_halo=0.75,
        **SCALARS, what=f"{path}: a rectangle moved between the planes")
    if path == "routed":
        run(dtype, JACOBI, (dst, 0, (7, 13)), (u, 0, (2, 31)), (kx, 0, (9, 0)), (ky, 0, (0, 50)), 30, 100, (f, 0, (5, 2)),
            halo=3.25, k_halo=0.75, **SCALARS, what="a rectangle moved between the planes, with a right-hand side")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_face_views_of_other_extents_and_origins(gpu, path, dtype):
    """"Outside the view" differs per view: the rectangle is the whole of kx's view (its west face is k_halo), begins
    in ky's first row but not in its first column (kn is k_halo, ky is read from column 3 on), and lies inside u's view
    (no halo at all); then the other way round."""
    u = plane(gpu, dtype, 12, 140, seed=41, width=137)
    kx = plane(gpu, dtype, 9, 132, seed=42, width=130)
    ky = plane(gpu, dtype, 10, 136, seed=43, width=134)
    f, dst = plane(gpu, dtype, 9, 132, seed=44), plane(gpu, dtype, 12, 140, seed=45)
    for mode in modes_on(path):
        which, has_rhs = MODES[mode]
        rhs = (f, 0, (0, 0)) if has_rhs else None
        run(dtype, which, (dst, 0, (2, 5)), None if which == SOLVE_DIAG else (u, 0, (2, 5)), kx, (ky, 0, (0, 3)), 9, 130, rhs,
            halo=7.0, k_halo=-1.25, **SCALARS, what=f"{path} {mode}: all of kx, the top of ky, the inside of u")
        run(dtype, which, (dst, 0, (0, 0)), None if which == SOLVE_DIAG else (u, 0, (3, 0)), (kx, 0, (1, 1)), (ky, 0, (1, 0)),
            8, 129, rhs, halo=7.0, k_halo=-1.25, **SCALARS, what=f"{path} {mode}: the left of u, the inside of kx and ky")
        run(dtype, which, (dst, 0, (0, 0)), None if which == SOLVE_DIAG else (u, 0, (0, 7)), (kx, 0, (0, 0)), (ky, 0, (0, 0)),
            9, 130, rhs, halo=7.0, k_halo=-1.25, **SCALARS, what=f"{path} {mode}: the top of u, the corners of kx and ky")


def test_more_rows_than_workgroups(gpu, path):
    """A workgroup that walks on: 2051 x 3 has more rows than a launch of the general kernel has workgroups (JACOBI as
    routed, APPLY under the switch); APPLY without a right-hand side on 2051 x 70 is 65 chunks of the dense kernel, one
    per workgroup, and on (CAP + 1) * CHUNK + 1 rows of 6 columns one chunk more than a launch has workgroups, so that
    workgroup 0 takes a second chunk (chunk += gridDim.y) and the last chunk is a single row."""
    tall = (CAP + 1) * CHUNK + 1
    for dtype in (F32, F64):
        for height, width in ((2051, 3), (2051, 70), (tall, 6)):
            u, kx, ky, f, dst = (plane(gpu, dtype, height, width + 2, seed=21 + k, width=width) for k in range(5))
            run(dtype, APPLY, dst, u, kx, ky, height, width, halo=0.5, k_halo=1.0, **SCALARS,
                what=f"{path}: apply on {height} x {width} planes")
            if path == "routed" and height == 2051:
                run(dtype, JACOBI, dst, u, kx, ky, height, width, f, halo=0.5, k_halo=1.0, **SCALARS,
                    what=f"jacobi on {height} x {width} planes")
    if path == "routed":
        cells = five_floats(gpu, 2051, 3, seed=29)
        run(F32, APPLY, (cells, 16), (cells, 0), (cells, 4), (cells, 8), 2051, 3, what="2051 x 3 members")


# ------------------------------------------------------------------ members of cells
def five_floats(device, height, pitch, seed, width=None):
    return Buffer(device, height, pitch, 32, seed, {0: F32, 4: F32, 8: F32, 12: F32, 16: F32}, width)


def three_doubles(device, height, pitch, seed, width=None):
    return Buffer(device, height, pitch, 24, seed, {0: F64, 8: F64, 16: F64}, width)


@pytest.mark.parametrize("width", [1, 3, SEGMENT - 1, SEGMENT, SEGMENT + 1])
def test_members_of_cells(gpu, width):
    """u, kx, ky, rhs and dst as five members of one 32-byte cell; spread over two kinds of cells and a plane; f64
    members.  The other members and the padding keep their bytes (Buffer.settle)."""
    one = five_floats(gpu, 5, width + 2, seed=7 * width + 1, width=width + 1)
    for mode in sorted(MODES):
        which, has_rhs = MODES[mode]
        run(F32, which, (one, 16), None if which == SOLVE_DIAG else (one, 0), (one, 4), (one, 8), 5, width + 1,
            (one, 12) if has_rhs else None, halo=0.5, k_halo=2.0, **SCALARS, what=f"{mode}: five members of one cell")
    run(F32, JACOBI, (one, 0, (1, 1)), (one, 4, (1, 1)), (one, 8, (1, 1)), (one, 12, (1, 1)), 3, width, (one, 0, (1, 1)),
        halo=float("nan"), k_halo=0.0, **SCALARS, what="jacobi: the right-hand side is the destination, an inner rectangle")
    fdtd = cell_buffer(gpu, "fdtd", 4, width + 1, seed=7 * width + 3, width=width)
    hot = cell_buffer(gpu, "hotspot", 5, width + 3, seed=7 * width + 4, width=width + 2)
    p = plane(gpu, F32, 4, width + 4, seed=7 * width + 5, shift=1)
    run(F32, APPLY, (fdtd, 8), (hot, 0, (1, 1)), (hot, 4, (0, 2)), (fdtd, 28), 4, width, (p, 0, (0, 3)), halo=-1.0, k_halo=1.0,
        **SCALARS, what="apply: members of two kinds of cells and a plane")
    run(F32, SOLVE_DIAG, (p, 0, (0, 1)), None, (fdtd, 12), (hot, 4, (1, 0)), 4, width, (fdtd, 8), k_halo=0.25, **SCALARS,
        what="solve_diag: members into a plane")
    triple = three_doubles(gpu, 4, width + 1, seed=7 * width + 6, width=width)
    doubles = plane(gpu, F64, 5, width + 2, seed=7 * width + 7, shift=1)
    run(F64, JACOBI, (triple, 16), (triple, 0), (triple, 8), (doubles, 0, (1, 1)), 4, width, (triple, 16), halo=0.125, k_halo=3.0,
        **SCALARS, what="jacobi: f64 members, rhs the destination")
    run(F64, APPLY, (doubles, 0, (0, 1)), (triple, 16), (triple, 0), (triple, 8), 4, width, halo=float("nan"), k_halo=1.0,
        **SCALARS, what="apply: f64 members into a plane")


# ------------------------------------------------------------------ special values
@pytest.mark.parametrize("kind", ["planted", "tiny", "huge", "negzero"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_special_values(gpu, path, dtype, kind):
    """inf and NaN planted in u and in a face (a zero face times an infinite difference is NaN: every face is
    multiplied), subnormal coefficients and results, sums that overflow, -0.0 everywhere, and a diagonal that is zero:
    the quotient is +-inf or NaN as numpy gives it."""
    make = {"planted": lambda shape, seed, dt: SV.planted(shape, seed, dtype=dt),
            "tiny": lambda shape, seed, dt: SV.tiny(shape, seed, dtype=dt),
            "huge": lambda shape, seed, dt: SV.huge(shape, seed, dtype=dt),
            "negzero": lambda shape, seed, dt: SV.negzero(shape, seed, dtype=dt)}[kind]
    h, w = 12, 134  # wider than 128, so that `planted` has its seam
    special = [plane(gpu, dtype, h, w, seed=60 + k, values=make) for k in range(4)]
    plain = [plane(gpu, dtype, h, w, seed=70 + k) for k in range(4)]
    out = plane(gpu, dtype, h, w, seed=80)
    # a zero diagonal: a cell whose four faces are zero (sigma = 0), and a whole row of them in negzero
    zero_faces = [plane(gpu, dtype, h, w, seed=90 + k) for k in range(2)]
    for k, buf in enumerate(zero_faces):
        values = buf.field(0, dtype)
        values[5, 60:70] = 0.0
        values[4, 60:70] = 0.0 if k == 1 else values[4, 60:70]
        values[5, 59] = 0.0 if k == 0 else values[5, 59]
        buf.device.copy_(torch.from_numpy(buf.model))
    plain[3].field(0, dtype)[5, 65] = 0.0
    plain[3].device.copy_(torch.from_numpy(plain[3].model))
    wants = {}
    for mode in modes_on(path):
        which, has_rhs = MODES[mode]
        for name, (u, kx, ky, f) in {"special u": (special[0], plain[1], plain[2], plain[3]),
                                     "special faces": (plain[0], special[1], special[2], plain[3]),
                                     "special rhs": (plain[0], plain[1], plain[2], special[3]),
                                     "all special": special,
                                     "a zero diagonal": (special[0], zero_faces[0], zero_faces[1], plain[3])}.items():
            for halo, k_halo in ((0.0, -0.0), (float("inf"), float(np.finfo(dtype).smallest_subnormal))):
                scalars = dict(SCALARS, sigma=0.0) if name == "a zero diagonal" else SCALARS
                wants[mode, name] = run(dtype, which, out, None if which == SOLVE_DIAG else u, kx, ky, h, w, f if has_rhs else None,
                                        halo=halo, k_halo=k_halo, **scalars, what=f"{path} {mode}, {kind}: {name}, halo {halo}")
    if path == "routed":
        # the cells (5, 61 .. 69) have four zero faces, d = 0 + 0.7 * 0, and the right-hand side of (5, 65) is zero
        quotient = wants["solve_diag", "a zero diagonal"][5, 61:70]
        assert np.isnan(quotient[4]) and np.isinf(np.delete(quotient, 4)).all(), "0 / 0 is NaN, x / 0 is +-inf"
    if kind == "planted":
        r, c = SV.planted_sites((h, w))["+inf"][1]  # +inf at (4, 63): the north neighbour of (5, 63), whose kn is zero
        assert (r, c) == (4, 63) and np.isposinf(special[0].field(0, dtype)[r, c])
        assert not np.isfinite(wants["apply", "special u"][r, c])
        assert np.isnan(wants["apply", "a zero diagonal"][5, 63]), "0 * inf is NaN: a zero face is multiplied"
    if kind == "tiny" and path == "routed":  # a result below the smallest normal stays what it is
        assert SV.classify(wants["solve_diag", "special rhs"])["subnormal"] > 0.1


def test_scalars_are_rounded_once_on_the_host(gpu, path):
    """0.1 is no float: the model computes with np.float32(0.1), and with 0.1 for doubles; a scalar below the smallest
    float is a zero that is still multiplied."""
    for dtype in (F32, F64):
        u, kx, ky, f, dst = (plane(gpu, dtype, 5, 70, seed=3 + k) for k in range(5))
        for value in (0.1, 1.0 / 3.0, -0.7, 1e-50, -0.0):
            for mode in modes_on(path):
                which, has_rhs = MODES[mode]
                run(dtype, which, dst, None if which == SOLVE_DIAG else u, kx, ky, 5, 70, f if has_rhs else None, sigma=value,
                    scale=1.0 / 3.0 if value == 0.1 else value, omega=value, rhs_coef=value, halo=0.1, k_halo=0.1,
                    what=f"{path} {mode}: scalars {value!r}")


# ------------------------------------------------------------------ several entries
@pytest.mark.parametrize("n", [2, 5, 8])
def test_several_entries_in_one_call(gpu, n):
    """Entries of every mode and both types in one call, as the library routes them; then disjoint tiles of ONE plane
    from one set of sources, through the general kernel (JACOBI) and through the dense one (APPLY without a right-hand
    side): a neighbour or a face outside a tile's rectangle reads the view."""
    from stencilstream_amd import capi

    kinds = [F32 if k % 2 == 0 else F64 for k in range(n)]
    made, alive = [], []  # (the sources must outlive the call: their memory would be handed to the next entry's buffers)
    for k in range(n):
        mode = sorted(MODES)[k % 4]
        which, has_rhs = MODES[mode]
        dst, u, kx, ky, f = (plane(gpu, kinds[k], 6, 140 + k, seed=100 + 10 * k + s) for s in range(5))
        alive += [dst, u, kx, ky, f]
        at = (k % 3, k % 5)
        made.append((kinds[k], at, 6 - k % 3, 140 + k - k % 5) +
                    diffuse(kinds[k], which, (dst, 0, at), None if which == SOLVE_DIAG else u, kx, ky, 6 - k % 3, 140 + k - k % 5,
                            (dst, 0, at) if has_rhs else None, halo=float(k), k_halo=0.5, **SCALARS))
    capi.grid_diffusion([m[4] for m in made])
    for k, (kind, at, n_rows, n_cols, _, want, to) in enumerate(made):
        to.buf.settle(0, kind, (at[0], at[0] + n_rows), (at[1], at[1] + n_cols), want, f"entry {k} of {n}")
    for k, buf in enumerate(alive):
        if k % 5 != 0:
            buf.unchanged(f"a source of entry {k // 5} of {n}")
    # disjoint rectangles of ONE plane, from one set of sources: tiles compose
    u, kx, ky, f, dst = (plane(gpu, F32, 16, 300, seed=200 + s) for s in range(5))
    tiles = [(r, c) for r in (0, 8) for c in (0, 75, 150, 225)][:n]
    for which, rhs in ((JACOBI, f), (APPLY, None)):
        made = [diffuse(F32, which, (dst, 0, at), (u, 0, at), (kx, 0, at), (ky, 0, at), 8, 75, None if rhs is None else (rhs, 0, at),
                        halo=1.0, k_halo=2.0, **SCALARS) for at in tiles]
        capi.grid_diffusion([desc for desc, _, _ in made])
        torch.cuda.synchronize()
        everything = whole(F32, which, u.field(0, F32), kx.field(0, F32), ky.field(0, F32),
                           rhs=None if rhs is None else rhs.field(0, F32), halo=1.0, k_halo=2.0, **SCALARS)
        got = dst.device.cpu().numpy()
        for (r, c), (_, want, _) in zip(tiles, made):
            SV.assert_same_cells(want, everything[r:r + 8, c:c + 75], "a neighbour or a face outside the rectangle reads the view")
            there = dst.field(0, F32, of=got)[r:r + 8, c:c + 75]
            SV.assert_same_cells(there, want, f"mode {which}: tile at {(r, c)}")
            dst.field(0, F32)[r:r + 8, c:c + 75] = there
        assert np.array_equal(got, dst.model), "bytes outside the tiles changed"


# ------------------------------------------------------------------ rows 2^32 + 16 bytes apart
def test_rows_4_gib_apart(gpu, monkeypatch):
    """All five views as f32 planes of 2 rows x 300 columns whose rows lie 2^32 + 16 bytes apart: the row offset of every
    view passes 2^32, and kn and n of row 1 come from there.  The guard and sentinel scheme of tests/large_extents.py:
    everything but the rectangles is a NaN with a payload, in front of the cells lie 2^31 + 4096 bytes, and afterwards
    every buffer is the sentinel again.  APPLY without a right-hand side through the dense kernel and, under the switch,
    through the general one; APPLY with a right-hand side, JACOBI and SOLVE_DIAG through the general kernel."""
    from stencilstream_amd import capi

    views = {name: LE.plane(name, k, LE.P30 + 4, 2, 300) for k, name in enumerate(("dst", "u", "kx", "ky", "rhs"))}
    need = sum(LE.arena_bytes(v) for v in views.values()) + (16 << 20)
    LE.require(need)
    try:
        arenas = {name: LE.Arena(gpu, v) for name, v in views.items()}
        rects = {name: LE.Rect(v, 0, 0, 2, 300) for name, v in views.items()}
        r, q = np.indices((2, 300))
        host = {name: LE.code_of(views[name].k, r, q).astype(F32) for name in views}
        host["kx"], host["ky"] = np.abs(host["kx"]) + 1, np.abs(host["ky"]) + 1  # positive faces: no zero diagonal
        for name in ("u", "kx", "ky", "rhs"):
            arenas[name].cells(rects[name]).copy_(torch.from_numpy(host[name]).to(gpu))
        cv = {name: arenas[name].capi_view(views[name]) for name in views}
        scalars = dict(sigma=0.5, scale=0.25, omega=0.75, rhs_coef=-2.0, halo=LE.HALO, k_halo=3.0)
        for general in (False, True):
            if general:
                monkeypatch.setenv("STSTHIP_DIFFUSION_GENERAL", "1")
            else:
                monkeypatch.delenv("STSTHIP_DIFFUSION_GENERAL", raising=False)
            routed = [(APPLY, True), (JACOBI, True), (SOLVE_DIAG, True)]  # (under the switch they would run twice)
            for which, has_rhs in [(APPLY, False)] + ([] if general else routed):
                capi.grid_diffusion([capi.grid_diffusion_desc(cv["dst"], None if which == SOLVE_DIAG else cv["u"], cv["kx"],
                                                              cv["ky"], "<f4", which, 2, 300,
                                                              rhs=cv["rhs"] if has_rhs else None, **scalars)])
                torch.cuda.synchronize()
                got = arenas["dst"].cells(rects["dst"]).cpu().numpy()
                want = whole(F32, which, host["u"], host["kx"], host["ky"], rhs=host["rhs"] if has_rhs else None, **scalars)
                SV.assert_same_cells(got, want, f"mode {which}, rhs {has_rhs}, {'the switch set' if general else 'as routed'}")
                arenas["dst"].clear(rects["dst"])
        for name in ("u", "kx", "ky", "rhs"):
            assert np.array_equal(arenas[name].cells(rects[name]).cpu().numpy(), host[name]), f"{name} changed"
            arenas[name].clear(rects[name])
        for name, arena in arenas.items():
            arena.assert_clean(name)
    finally:
        arenas = None
        LE.release(f"diffusion on rows 4 GiB apart, need {need}")


# ------------------------------------------------------------------ update.Grid
def test_damped_jacobi_through_update_grid(gpu):
    """50 damped Jacobi steps (omega = 0.8) on the problem of the CPU test, ping-ponging two grids: the model's bytes."""
    from stencilstream_amd import update as U

    kx_host, ky_host, f_host = pcg_problem("<f4")
    want = np.zeros((PH, PW), dtype=F32)
    for _ in range(50):
        want = whole(F32, JACOBI, want, kx_host, ky_host, k_halo=1.0, omega=0.8, rhs=f_host)
    kx, ky, f = (U.Grid.from_numpy(a, device=gpu) for a in (kx_host, ky_host, f_host))
    a, b = U.Grid(PH, PW, "<f4", device=gpu), U.Grid(PH, PW, "<f4", device=gpu)
    for _ in range(50):
        b.diffusion(a, kx, ky, mode="jacobi", omega=0.8, k_halo=1.0, rhs=f)
        a, b = b, a
    got = a.to_numpy()
    assert np.abs(want).max() > 1e-3, "the relaxation moved nothing"
    SV.assert_same_cells(got, want, "50 damped Jacobi steps")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the same on members of cells and on an inner rectangle: the rest keeps its bytes
    cells = np.zeros((PH, PW), dtype=U.FDTD_CELL)
    cells["ex"], cells["ey"], cells["hz"], cells["hz_sum"] = kx_host, ky_host, f_host, got
    grid = U.Grid.from_numpy(cells, device=gpu)
    grid.diffusion(grid, grid, grid, mode="jacobi", omega=0.8, k_halo=1.0, rhs=grid, field="ca", src_field="hz_sum",
                   kx_field="ex", ky_field="ey", rhs_field="hz", rows=(1, PH - 1), cols=(2, PW))
    there = grid.to_numpy()
    inner = diffusion_model(F32, JACOBI, got, kx_host, ky_host, PH - 2, PW - 2, (1, 2), (1, 2), (1, 2), k_halo=1.0, omega=0.8,
                            rhs=f_host[1:PH - 1, 2:PW])
    expect = np.zeros((PH, PW), dtype=F32)
    expect[1:PH - 1, 2:PW] = inner
    SV.assert_same_cells(there["ca"], expect, "a Jacobi step on members")
    for name in ("ex", "ey", "hz", "hz_sum", "cb", "da", "db"):
        assert np.array_equal(there[name].view(np.uint32), cells[name].view(np.uint32)), f"{name} changed"


def pcg_device(gpu, kx_host, ky_host, f_host, tolerance):
    """Jacobi-preconditioned conjugate gradients with diffusion (apply and solve_diag), combine and dot only: the loop
    of pcg_model.  Returns (x, iterations)."""
    from stencilstream_amd import update as U

    kx, ky = U.Grid.from_numpy(kx_host, gpu), U.Grid.from_numpy(ky_host, gpu)
    zero = np.zeros_like(f_host)
    x, r, z, p, ap = (U.Grid.from_numpy(a, gpu) for a in (zero, f_host, zero, zero, zero))
    z.diffusion(None, kx, ky, mode="solve_diag", k_halo=1.0, rhs=r)
    p.combine([(1.0, z)])
    ff, rz = r.dot().dot, r.dot(z).dot
    for iteration in range(1, MAX_ITERATIONS + 1):
        ap.diffusion(p, kx, ky, halo=0.0, k_halo=1.0)
        alpha = rz / p.dot(ap).dot
        x.combine([(1.0, x), (alpha, p)])
        r.combine([(1.0, r), (-alpha, ap)])
        if math.sqrt(r.dot().dot / ff) <= tolerance:
            return x.to_numpy(), iteration
        z.diffusion(None, kx, ky, mode="solve_diag", k_halo=1.0, rhs=r)
        rz_next = r.dot(z).dot
        p.combine([(1.0, z), (rz_next / rz, p)])
        rz = rz_next
    raise AssertionError("preconditioned conjugate gradients on the device have not converged")


@pytest.mark.parametrize("dtype", ["<f8", "<f4"], ids=["f8", "f4"])
def test_preconditioned_conjugate_gradients(gpu, dtype):
    """Device and model run the same loop and differ in the order in which a dot is summed only, so they take the same
    number of iterations within +-2 (the slack of tests/test_grid_dot_gpu.py; the model takes the same number for
    np.dot, math.fsum and a reversed sum), and the true residual |f - A x| / |f|, recomputed in float64 from the
    downloaded x, is below twice the tolerance."""
    tolerance = TOLERANCE[dtype]
    kx, ky, f = pcg_problem(dtype)
    _, model_iterations = pcg_model(kx, ky, f, tolerance)
    x, iterations = pcg_device(gpu, kx, ky, f, tolerance)
    f64 = f.astype(np.float64)
    ax = whole("<f8", APPLY, x.astype(np.float64), kx.astype(np.float64), ky.astype(np.float64), k_halo=1.0)
    true_residual = float(np.linalg.norm(f64 - ax) / np.linalg.norm(f64))
    print(f"{dtype}: {iterations} iterations on the device, {model_iterations} in the model, true residual {true_residual:.3e} "
          f"({true_residual / tolerance:.2f} x the tolerance)")
    assert abs(iterations - model_iterations) <= 2
    assert true_residual < 2 * tolerance

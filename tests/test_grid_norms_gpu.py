"""ststhip_grid_norms / ststhip_grid_distance on the device against numpy on the host (capi.grid_norms, update.Grid.norms).

The per-cell value v is the element converted to float64, or float64(a) - float64(b).  n_cells, n_nonfinite and
max_abs must be equal (max_abs as bits).  The sums are compared with math.fsum over the finite v (the exact sum of
those float64 values):

    |got - exact| <= n * 2^-52 * sum |v|          sum, sum_abs
    |got - exact| <= (n + 1) * 2^-52 * sum v^2    sum_sq

the gamma_n bound of n additions in any order, one more rounding for the square, a factor two of slack: derived, holds
for every order of summation.  Data: seeded, both signs, magnitudes 2^-20 .. 2^20."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NEG_INF = float("-inf")


def wide(rng, shape, dtype="<f4"):
    """Both signs, magnitudes 2^-20 .. 2^20."""
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return (sign * (0.5 + 0.5 * rng.random(shape)) * np.exp2(rng.integers(-20, 21, shape))).astype(dtype)


def on_device(gpu, array):
    import torch

    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).to(gpu)


def reference(a, b=None):
    """The definitions on the host; a, b = the elements of the rectangle."""
    v = a.astype(np.float64)
    if b is not None:
        with np.errstate(invalid="ignore"):
            v = v - b.astype(np.float64)
    v = v.reshape(-1)
    finite = v[np.isfinite(v)]
    return {
        "n_cells": v.size, "n_nonfinite": v.size - finite.size,
        "max_abs": float(np.abs(finite).max()) if finite.size else NEG_INF,
        "sum": math.fsum(finite), "sum_abs": math.fsum(np.abs(finite)), "sum_sq": math.fsum(finite * finite),
    }


def expect(what, got, want):
    """`got`: a ststhip_norm_result or update.Norms.  Prints every figure, then asserts."""
    n = want["n_cells"]
    bounds = {"sum": n * EPS * want["sum_abs"], "sum_abs": n * EPS * want["sum_abs"], "sum_sq": (n + 1) * EPS * want["sum_sq"]}
    print(f"{what}: n_cells {got.n_cells} / {want['n_cells']}, n_nonfinite {got.n_nonfinite} / {want['n_nonfinite']}, "
          f"max_abs {float(got.max_abs).hex()} / {float(want['max_abs']).hex()}")
    for name, bound in bounds.items():
        print(f"    {name}: got {getattr(got, name)!r}, exact {want[name]!r}, off {abs(getattr(got, name) - want[name]):.3e}, bound {bound:.3e}")
    assert got.n_cells == want["n_cells"] and got.n_nonfinite == want["n_nonfinite"]
    assert np.float64(got.max_abs).tobytes() == np.float64(want["max_abs"]).tobytes()
    for name, bound in bounds.items():
        assert abs(getattr(got, name) - want[name]) <= bound, name


def plane_norms(gpu, a, width=None, rows=None, cols=None, b=None):
    """One plane: `a` is the stored array (its row length is the pitch), `width` the columns that belong to the grid."""
    from stencilstream_amd import capi

    height, pitch = a.shape
    width = pitch if width is None else width
    da = on_device(gpu, a)
    db = None if b is None else on_device(gpu, b)
    f = capi.norm_field(da.data_ptr(), a.dtype.str, a.dtype.itemsize, height, width, pitch=pitch, rows=rows, cols=cols)
    return capi.grid_norms([f], None if b is None else [db.data_ptr()])[0]


# ---------------------------------------------------------------------------------------------------- planes
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (1, 63), (1, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", ["<f4", "<f8"])
def test_small_planes(gpu, shape, dtype):
    """Less than a wave; more than one wave with an unaligned tail."""
    a = wide(np.random.default_rng(shape[0] * 1000 + shape[1]), shape, dtype)
    expect(f"{shape} {dtype}", plane_norms(gpu, a), reference(a))


@pytest.fixture(scope="module")
def planes_130x257():
    """130 x 257 stored with pitch 260, as floats and as doubles, and their references over the whole grid and over
    rows [1, 129) x columns [1, 256): computed once."""
    rng = np.random.default_rng(130257)
    out = {}
    for dtype in ("<f4", "<f8"):
        a = wide(rng, (130, 260), dtype)
        out[dtype] = (a, reference(a[:, :257]), reference(a[1:129, 1:256]))
    return out


@pytest.mark.parametrize("dtype", ["<f4", "<f8"])
def test_pitched_plane_and_odd_rectangle(gpu, planes_130x257, dtype):
    """Pitch 260 keeps every row 16-byte aligned and 257 columns leave a tail; the rectangle that starts at row 1 and
    column 1 has a misaligned head in every row."""
    a, whole, inner = planes_130x257[dtype]
    expect("whole grid", plane_norms(gpu, a, width=257), whole)
    expect("rows [1, 129) x cols [1, 256)", plane_norms(gpu, a, width=257, rows=(1, 129), cols=(1, 256)), inner)


@pytest.mark.parametrize("dtype,pitch", [("<f4", 259), ("<f4", 258), ("<f8", 259)])
def test_pitch_that_moves_the_alignment_from_row_to_row(gpu, dtype, pitch):
    """A pitch that is no multiple of a 16-byte vector: head and tail differ from row to row."""
    a = wide(np.random.default_rng(pitch), (37, pitch), dtype)
    expect(f"pitch {pitch}", plane_norms(gpu, a, width=257), reference(a[:, :257]))
    expect(f"pitch {pitch}, odd start", plane_norms(gpu, a, width=257, rows=(2, 30), cols=(3, 250)), reference(a[2:30, 3:250]))


def test_empty_and_clipped_rectangles(gpu, planes_130x257):
    a, whole, _ = planes_130x257["<f4"]
    for rows, cols in (((5, 5), None), ((9, 3), None), (None, (257, 300)), ((130, 140), (0, 10))):
        r = plane_norms(gpu, a, width=257, rows=rows, cols=cols)
        assert (r.n_cells, r.n_nonfinite, r.sum, r.sum_abs, r.sum_sq, r.max_abs) == (0, 0, 0.0, 0.0, 0.0, NEG_INF)
    # reaching past the grid: clipped to it (and not to the pitch)
    expect("clipped", plane_norms(gpu, a, width=257, rows=(0, 1000), cols=(0, 1000)), whole)
    expect("clipped corner", plane_norms(gpu, a, width=257, rows=(100, 1000), cols=(200, 1000)), reference(a[100:130, 200:257]))


@pytest.mark.parametrize("shape,dtype", [((2049, 3), "<f4"), ((1030, 2050), "<f4"), ((1030, 1025), "<f8"), ((2049, 3), "<f8")],
                         ids=["2049x3-f4", "1030x2050-f4", "1030x1025-f8", "2049x3-f8"])
def test_a_workgroup_takes_more_than_one_row_segment(gpu, shape, dtype):
    """A launch has at most 2048 workgroups (norm_block_cap in csrc/norms.hip).  A row of a plane is cut into segments of
    8 KiB (2048 floats, 1024 doubles); with s segments per row, min(rows, 2048 // s) workgroups work side by side down
    the rows and take every (2048 // s)-th row.  2049 x 3: one segment, 2048 workgroups, workgroup 0 takes rows 0 and
    2048.  1030 x 2050 floats and 1030 x 1025 doubles: two segments (the second of two elements and of one), 1024
    workgroups per segment, the first six of each take rows r and r + 1024."""
    a = wide(np.random.default_rng(shape[0] + shape[1]), shape, dtype)
    expect(f"{shape} {dtype}", plane_norms(gpu, a), reference(a))


def test_sum_that_cancels(gpu):
    """sum v is near zero, sum |v| is large: the bound is on sum |v|, and the device must meet it."""
    rng = np.random.default_rng(7)
    half = wide(rng, (64, 257), "<f8")
    a = np.concatenate([half, -half])
    a = a.reshape(-1)[rng.permutation(a.size)].reshape(128, 257)
    a[0, 0] += 2.0 ** -20
    want = reference(a)
    assert abs(want["sum"]) < 1e-3 and want["sum_abs"] > 1e6
    expect("cancelling", plane_norms(gpu, a), want)


# ---------------------------------------------------------------------------------------------------- AoS cells
def grid_of(gpu, cells):
    from stencilstream_amd import update as U

    return U.Grid.from_numpy(cells, gpu)


def aos_cells(rng, shape, cell):
    cells = np.zeros(shape, dtype=cell)
    for name in cell.names:
        if cell.fields[name][0].kind == "f":
            cells[name] = wide(rng, shape, cell.fields[name][0])
    return cells


def test_hotspot_cells_both_fields_in_one_call(gpu):
    from stencilstream_amd import update as U

    cells = aos_cells(np.random.default_rng(11), (67, 1100), U.HOTSPOT_CELL)  # more than one segment of 1024 cells
    got = grid_of(gpu, cells).norms()
    assert list(got) == ["temp", "power"]
    for name in got:
        expect(name, got[name], reference(cells[name]))
    got = grid_of(gpu, cells).norms(rows=(1, 66), cols=(3, 1099))
    for name in got:
        expect(name + " rectangle", got[name], reference(cells[name][1:66, 3:1099]))


@pytest.mark.parametrize("shape", [(2049, 3), (1030, 1030)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_workgroup_takes_more_than_one_row_segment_of_cells(gpu, shape):
    """The same cap of 2048 workgroups for strided fields, whose row segments are 1024 cells: 2049 x 3 has one segment per
    row and 2048 workgroups, workgroup 0 takes rows 0 and 2048; 1030 x 1030 has two segments (the second of six cells)
    and 1024 workgroups per segment, the first six of each take rows r and r + 1024.  Norms and distance."""
    from stencilstream_amd import update as U

    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    a, b = aos_cells(rng, shape, U.HOTSPOT_CELL), aos_cells(rng, shape, U.HOTSPOT_CELL)
    ga = grid_of(gpu, a)
    got, apart = ga.norms(), ga.norms(other=grid_of(gpu, b))
    for name in ("temp", "power"):
        expect(name, got[name], reference(a[name]))
        expect(name + " distance", apart[name], reference(a[name], b[name]))


def test_fdtd_cells_two_of_eight_fields(gpu):
    from stencilstream_amd import update as U

    cells = aos_cells(np.random.default_rng(12), (33, 130), U.FDTD_CELL)
    got = grid_of(gpu, cells).norms(fields=["hz", "ex"])
    assert list(got) == ["hz", "ex"]
    for name in got:
        expect(name, got[name], reference(cells[name]))
    assert len(grid_of(gpu, cells).norms()) == 8


def test_cells_of_eleven_doubles_two_fields_with_their_own_rectangles(gpu):
    """The convection layout: 88-byte cells; the staggered fields have rectangles of their own."""
    from stencilstream_amd import capi

    cell = np.dtype([(f"f{i}", "<f8") for i in range(11)])
    assert cell.itemsize == 88
    H, W = 41, 130
    cells = aos_cells(np.random.default_rng(13), (H, W), cell)
    dev = on_device(gpu, cells)
    fields = [capi.norm_field(dev.data_ptr() + 8 * 2, "<f8", 88, H, W, rows=(0, H - 1), cols=(0, W)),
              capi.norm_field(dev.data_ptr() + 8 * 9, "<f8", 88, H, W, rows=(3, H), cols=(1, W - 2))]
    got = capi.grid_norms(fields)
    expect("f2", got[0], reference(cells["f2"][:H - 1, :]))
    expect("f9", got[1], reference(cells["f9"][3:, 1:W - 2]))


def test_mixed_call_of_planes_and_members(gpu):
    """Contiguous and strided fields in one call; an empty one between them."""
    from stencilstream_amd import capi, update as U

    rng = np.random.default_rng(14)
    cells = aos_cells(rng, (20, 70), U.HOTSPOT_CELL)
    plane = wide(rng, (9, 300), "<f8")
    dc, dp = on_device(gpu, cells), on_device(gpu, plane)
    fields = [capi.norm_field(dc.data_ptr() + 4, "<f4", 8, 20, 70),
              capi.norm_field(dp.data_ptr(), "<f8", 8, 9, 300),
              capi.norm_field(dc.data_ptr(), "<f4", 8, 20, 70, rows=(4, 4)),
              capi.norm_field(dc.data_ptr(), "<f4", 8, 20, 70, cols=(1, 70))]
    got = capi.grid_norms(fields)
    expect("power", got[0], reference(cells["power"]))
    expect("plane", got[1], reference(plane))
    assert got[2].n_cells == 0 and got[2].max_abs == NEG_INF
    expect("temp", got[3], reference(cells["temp"][:, 1:]))


def test_fields_of_another_type_are_refused(gpu):
    from stencilstream_amd import update as U

    cell = np.dtype([("count", "<i4"), ("value", "<f4")])
    cells = np.zeros((5, 7), dtype=cell)
    cells["value"] = wide(np.random.default_rng(15), (5, 7))
    g = grid_of(gpu, cells)
    with pytest.raises(ValueError):
        g.norms(fields=["count"])
    with pytest.raises(ValueError):
        g.norms(fields=["nothing"])
    got = g.norms()  # the default: every float field
    assert list(got) == ["value"]
    expect("value", got["value"], reference(cells["value"]))
    with pytest.raises(ValueError):
        g.norms(other=grid_of(gpu, np.zeros((5, 8), dtype=cell)))
    with pytest.raises(ValueError):
        g.norms(other=grid_of(gpu, np.zeros((5, 7), dtype=U.HOTSPOT_CELL)))


# ---------------------------------------------------------------------------------------------------- distance
def test_distance_of_grids_that_differ_in_known_cells(gpu):
    rng = np.random.default_rng(21)
    a = wide(rng, (130, 257))
    b = a.copy()
    b[0, 0] = a[0, 0] + np.float32(1.0)
    b[77, 256] = np.float32(2.0) * a[77, 256]
    b[129, 1] = -a[129, 1]
    known = max(abs(float(a[r, c]) - float(b[r, c])) for r, c in ((0, 0), (77, 256), (129, 1)))
    ga, gb = grid_of(gpu, a), grid_of(gpu, b)
    got = ga.norms(other=gb)[None]
    assert got.n_cells == 130 * 257 and got.max_abs == known and got.n_nonfinite == 0
    expect("distance", got, reference(a, b))
    same = ga.norms(other=ga)[None]
    assert (same.n_cells, same.n_nonfinite, same.max_abs, same.sum, same.sum_abs, same.sum_sq) == (130 * 257, 0, 0.0, 0.0, 0.0, 0.0)


def test_distance_is_one_rounding_in_double(gpu):
    """2^20 against 2^-20 in f32: the difference in float32 would be 2^20 exactly; in double it is not."""
    rng = np.random.default_rng(22)
    a = (np.exp2(20) * (1 + rng.random((9, 257)))).astype("<f4")
    b = (np.exp2(-20) * (1 + rng.random((9, 257)))).astype("<f4")
    want = reference(a, b)
    assert want["max_abs"] != float(np.abs(a - b).max())  # the float32 difference is another number
    expect("2^20 - 2^-20", plane_norms(gpu, a, b=b), want)
    expect("2^-20 - 2^20", plane_norms(gpu, b, b=a), reference(b, a))


def test_distance_of_hotspot_cells(gpu):
    from stencilstream_amd import update as U

    rng = np.random.default_rng(23)
    a, b = aos_cells(rng, (20, 300), U.HOTSPOT_CELL), aos_cells(rng, (20, 300), U.HOTSPOT_CELL)
    got = grid_of(gpu, a).norms(other=grid_of(gpu, b), rows=(1, 20))
    for name in ("temp", "power"):
        expect(name, got[name], reference(a[name][1:], b[name][1:]))


# ---------------------------------------------------------------------------------------------------- non-finite values
@pytest.mark.parametrize("dtype", ["<f4", "<f8"])
def test_nonfinite_cells_are_counted_and_left_out(gpu, dtype):
    a = wide(np.random.default_rng(31), (130, 257), dtype)
    a[0, 0], a[64, 200], a[129, 256] = np.nan, np.inf, -np.inf
    want = reference(a)
    assert want["n_nonfinite"] == 3
    expect("three planted", plane_norms(gpu, a), want)
    # inf - inf is NaN: counts; inf - 1 is inf: counts; nan against anything too
    b = a.copy()
    b[0, 0], b[5, 5] = 1.0, np.inf
    want = reference(a, b)
    assert want["n_nonfinite"] == 4 and want["max_abs"] == 0.0
    expect("distance with infinities", plane_norms(gpu, a, b=b), want)
    only = np.full((3, 5), np.nan, dtype=dtype)
    r = plane_norms(gpu, only)
    assert (r.n_cells, r.n_nonfinite, r.max_abs, r.sum, r.sum_abs, r.sum_sq) == (15, 15, NEG_INF, 0.0, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------------- determinism
def test_the_same_call_gives_the_same_bytes(gpu):
    from stencilstream_amd import capi, update as U

    rng = np.random.default_rng(41)
    cells = aos_cells(rng, (67, 1100), U.HOTSPOT_CELL)
    plane = wide(rng, (1030, 2050))
    dc, dp = on_device(gpu, cells), on_device(gpu, plane)
    fields = [capi.norm_field(dp.data_ptr(), "<f4", 4, 1030, 2050),
              capi.norm_field(dc.data_ptr(), "<f4", 8, 67, 1100),
              capi.norm_field(dc.data_ptr() + 4, "<f4", 8, 67, 1100)]
    runs = [bytes(capi.grid_norms(fields)) for _ in range(3)]
    assert len(runs[0]) == 3 * 48 and runs[0] == runs[1] == runs[2]


# ---------------------------------------------------------------------------------------------------- with a sweep
def test_distance_after_a_sweep(gpu):
    """jacobi5general, 0.2 x 5, 96 x 160, the centred square, 16 generations: the distance of the result and its
    source, both still on the device, equals numpy's on the two downloaded grids."""
    from stencilstream_amd import update as U

    H, W = 96, 160
    r, c = np.mgrid[0:H, 0:W]
    start = ((r >= H * 0.25) & (r < H * 0.75) & (c >= W * 0.25) & (c < W * 0.75)).astype("<f4")
    source = U.Grid.from_numpy(start, gpu)
    update = U.StencilUpdate(U.Params(U.jacobi("Jacobi5General", [0.2] * 5), halo_value=np.float32(0.0), n_iterations=16))
    result = update(source)  # not blocking: the norms are ordered behind the sweep
    got = result.norms(other=source)[None]
    after, before = result.to_numpy(), source.to_numpy()
    assert np.array_equal(before, start)
    want = reference(after, before)
    assert want["max_abs"] > 0.0 and got.max_abs == want["max_abs"]
    expect("after - before", got, want)
    expect("after", result.norms()[None], reference(after))

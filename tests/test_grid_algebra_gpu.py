"""ststhip_grid_combine / ststhip_grid_resample on the device against numpy, operation by operation in the element's
dtype: `np.float32(c0) * x0`, then `+ np.float32(c1) * x1` ...; the restrict and prolong formulas of ststhip.h verbatim.

The comparison is special_values.assert_same_cells: NaNs in exactly the same cells, every other cell equal AS BITS
(+-0, +-inf and subnormals included); there is no tolerance anywhere.  Every device buffer has GUARD bytes in front of
and behind the grid and holds a byte pattern everywhere but in the float members the test computes with; the host
keeps a model of all of it, and after every call the WHOLE buffer is compared with the model: cells outside the
rectangle, other members of the cells inside it, the pitch padding and both guards hold their former bytes."""
import numpy as np
import pytest
import torch

import special_values as SV

pytestmark = pytest.mark.gpu

GUARD = 4096
F32, F64 = np.dtype("<f4"), np.dtype("<f8")
RESTRICT, PROLONG = 0, 1
WIDTHS = [1, 3, 1023, 1024, 1025, 4097]  # around a strided segment (1024 cells) and a dense one (16 KiB)


class Buffer:
    """height x pitch cells of `stride` bytes in HBM between two guards, `shift` bytes behind the front guard, and the
    host's model of all of it.  `fields`: {byte offset in the cell: dtype} of the float members; they start out as
    values in (-1, 1), everything else as a byte pattern."""

    def __init__(self, device, height, pitch, stride, seed, fields, width=None, shift=0, values=None):
        self.height, self.pitch, self.stride, self.shift = height, pitch, stride, shift
        self.width = pitch if width is None else width
        self.n = height * pitch * stride
        rng = np.random.default_rng(seed)
        self.model = rng.integers(0, 256, size=GUARD + shift + self.n + GUARD, dtype=np.uint8)
        for offset, dtype in fields.items():
            made = (2.0 * rng.random((height, pitch)) - 1.0) if values is None else values((height, pitch), seed + offset, dtype)
            self.field(offset, dtype)[...] = made.astype(dtype)
        self.device = torch.from_numpy(self.model.copy()).to(device)
        self.base = self.device.data_ptr() + GUARD + shift

    def field(self, offset, dtype, of=None):
        """The member at `offset` of every cell as a height x pitch array: a view of the model (or of `of`)."""
        whole = self.model if of is None else of
        return np.ndarray((self.height, self.pitch), dtype=dtype, buffer=whole, offset=GUARD + self.shift + offset,
                          strides=(self.pitch * self.stride, self.stride))

    def view(self, offset=0):
        from stencilstream_amd import capi

        return capi.grid_view(self.base + offset, self.stride, self.height, self.width, self.pitch)

    def settle(self, offset, dtype, rows, cols, want, what):
        """The rectangle rows x cols of the member holds `want` by the rule of special_values, and every other byte of
        the buffer is the model's.  The model takes over what the device wrote."""
        torch.cuda.synchronize()
        got = self.device.cpu().numpy()
        there = self.field(offset, dtype, of=got)[rows[0]:rows[1], cols[0]:cols[1]]
        assert there.shape == want.shape, (there.shape, want.shape)
        SV.assert_same_cells(there, want, what)
        self.field(offset, dtype)[rows[0]:rows[1], cols[0]:cols[1]] = there  # (a NaN's payload is the device's)
        if not np.array_equal(got, self.model):
            wrong = np.flatnonzero(got != self.model) - GUARD - self.shift
            cell, byte = np.divmod(wrong, self.stride)
            row, col = np.divmod(cell, self.pitch)
            raise AssertionError(f"{what}: {wrong.size} bytes outside the rectangle changed, the first at row {row[0]}, "
                                 f"column {col[0]}, byte {byte[0]} of the cell")

    def unchanged(self, what):
        torch.cuda.synchronize()
        assert np.array_equal(self.device.cpu().numpy(), self.model), f"{what}: a source changed"


# ------------------------------------------------------------------ the models, operation by operation
def combine_model(dtype, coefs, xs):
    T = dtype.type
    with np.errstate(all="ignore"):
        acc = T(coefs[0]) * xs[0]
        for coef, x in zip(coefs[1:], xs[1:]):
            acc = acc + T(coef) * x
    assert acc.dtype == dtype
    return acc


def restrict_model(dtype, s):
    """s: the 2n x 2m source rectangle."""
    T = dtype.type
    with np.errstate(all="ignore"):
        out = ((s[0::2, 0::2] + s[0::2, 1::2]) + (s[1::2, 0::2] + s[1::2, 1::2])) * T(0.25)
    assert out.dtype == dtype
    return out


def prolong_model(dtype, view, at, n_rows, n_cols, halo):
    """view: the whole source view (height x width); the rectangle of n_rows x n_cols coarse cells begins at `at`."""
    T = dtype.type
    padded = np.full((view.shape[0] + 2, view.shape[1] + 2), T(halo), dtype=dtype)
    padded[1:-1, 1:-1] = view
    r, q = at[0] + 1, at[1] + 1  # the rectangle in `padded`

    def c(row_shift, col_shift):
        return padded[r + row_shift:r + row_shift + n_rows, q + col_shift:q + col_shift + n_cols]

    out = np.empty((2 * n_rows, 2 * n_cols), dtype=dtype)
    with np.errstate(all="ignore"):
        for b, j_far in ((0, -1), (1, +1)):
            h = {i: T(0.75) * c(i, 0) + T(0.25) * c(i, j_far) for i in (-1, 0, +1)}
            for a, i_far in ((0, -1), (1, +1)):
                out[a::2, b::2] = T(0.75) * h[0] + T(0.25) * h[i_far]
    return out


def huge_coef(dtype):
    return float(np.finfo(dtype).max) / 2


# ------------------------------------------------------------------ calls with their models
def combine(dst, dst_offset, dtype, terms, n_rows, n_cols, dst_at=(0, 0)):
    """terms: (coef, buffer, offset, (row, col)).  Returns (description, what the rectangle must hold)."""
    from stencilstream_amd import capi

    xs = [buf.field(off, dtype)[:buf.height, :buf.width][r:r + n_rows, c:c + n_cols].copy() for _, buf, off, (r, c) in terms]
    assert all(x.shape == (n_rows, n_cols) for x in xs), "a term's rectangle leaves its view"
    want = combine_model(dtype, [t[0] for t in terms], xs)
    desc = capi.grid_combine_desc(dst.view(dst_offset), dtype.str, [(coef, buf.view(off), at) for coef, buf, off, at in terms],
                                  n_rows, n_cols, dst_at)
    return desc, want


def run_combine(dst, dst_offset, dtype, terms, n_rows, n_cols, dst_at=(0, 0), what="combine"):
    from stencilstream_amd import capi

    desc, want = combine(dst, dst_offset, dtype, terms, n_rows, n_cols, dst_at)
    capi.grid_combine([desc])
    dst.settle(dst_offset, dtype, (dst_at[0], dst_at[0] + n_rows), (dst_at[1], dst_at[1] + n_cols), want, what)


def resample(mode, dst, dst_offset, src, src_offset, dtype, n_rows, n_cols, dst_at=(0, 0), src_at=(0, 0), halo=0.0):
    """Returns (description, the destination rectangle (rows, cols), what it must hold)."""
    from stencilstream_amd import capi

    s = src.field(src_offset, dtype)[:src.height, :src.width]
    if mode == RESTRICT:
        want = restrict_model(dtype, s[src_at[0]:src_at[0] + 2 * n_rows, src_at[1]:src_at[1] + 2 * n_cols].copy())
    else:
        want = prolong_model(dtype, s, src_at, n_rows, n_cols, halo)
    desc = capi.grid_resample_desc(dst.view(dst_offset), src.view(src_offset), dtype.str, mode, n_rows, n_cols, dst_at,
                                   src_at, halo)
    return desc, ((dst_at[0], dst_at[0] + want.shape[0]), (dst_at[1], dst_at[1] + want.shape[1])), want


def run_resample(mode, dst, dst_offset, src, src_offset, dtype, n_rows, n_cols, dst_at=(0, 0), src_at=(0, 0), halo=0.0,
                 what="resample"):
    from stencilstream_amd import capi

    desc, (rows, cols), want = resample(mode, dst, dst_offset, src, src_offset, dtype, n_rows, n_cols, dst_at, src_at, halo)
    capi.grid_resample([desc])
    dst.settle(dst_offset, dtype, rows, cols, want, what)


# the cells: name -> (stride, dtype, offsets of the members the tests compute with)
CELLS = {
    "hotspot": (8, F32, (0, 4)),                # update.HOTSPOT_CELL: temp, power
    "hotspot f64": (16, F64, (0, 8)),           # update.HOTSPOT_CELL_F64
    "fdtd": (32, F32, (8, 12, 28)),             # update.FDTD_CELL: hz, hz_sum, db
    "fdtd f64": (32, F64, (0, 16, 24)),         # four doubles
}


def cell_buffer(device, cell, height, pitch, seed, width=None, shift=0, values=None):
    stride, dtype, offsets = CELLS[cell]
    return Buffer(device, height, pitch, stride, seed, {o: dtype for o in offsets}, width, shift, values)


def plane(device, dtype, height, pitch, seed, width=None, shift=0, values=None):
    return Buffer(device, height, pitch, dtype.itemsize, seed, {0: dtype}, width, shift * dtype.itemsize, values)


# ------------------------------------------------------------------ combine
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_combine_planes_at_every_alignment(gpu, dtype, width):
    """1 to 4 terms over three rows of planes whose bases are shifted by 0..3 elements against each other, from
    column offsets 0..3: every access width, heads and tails of every length; coefficients 0, -1, 0.1 and a huge one;
    every other call has the destination among its terms (in place)."""
    pitch = width + 7
    dst = plane(gpu, dtype, 4, pitch, seed=10 * width + 1, width=width + 3, shift=1)
    srcs = [plane(gpu, dtype, 4, pitch + k, seed=10 * width + 2 + k, width=width + 3, shift=k) for k in range(4)]
    coefs = [0.1, -1.0, 0.0, huge_coef(dtype), 1.0]
    n_calls = 0
    for d in range(4):
        for rel in range(4):
            n_terms = 1 + (d + rel) % 4
            cols = [(d + rel * (k + 1)) % 4 for k in range(n_terms)]
            terms = [(coefs[(k + rel) % 5], srcs[(k + d) % 4], 0, (k % 2, cols[k])) for k in range(n_terms)]
            if (d + rel) % 2 == 1:
                terms[-1] = (coefs[(d + 2) % 5], dst, 0, (1, d))  # the destination's own rectangle
            run_combine(dst, 0, dtype, terms, 3, width, dst_at=(1, d),
                        what=f"{n_terms} terms, width {width}, destination column {d}, terms' columns {cols}")
            n_calls += 1
    assert n_calls == 16
    for s in srcs:
        s.unchanged("combine of planes")


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("cell", sorted(CELLS))
def test_combine_members_of_cells(gpu, cell, width):
    """A member of AoS cells from members of the same cells (in place, member to member), of other cells of the same
    type and of a plane; the other members of the destination's cells keep their bytes."""
    stride, dtype, offsets = CELLS[cell]
    a = cell_buffer(gpu, cell, 5, width + 2, seed=7 * width + 1, width=width + 1)
    b = cell_buffer(gpu, cell, 4, width + 4, seed=7 * width + 2)
    p = plane(gpu, dtype, 3, width + 1, seed=7 * width + 3, shift=1)
    m0, m1 = offsets[0], offsets[1]
    # member to member of the same cells, then in place, then everything at once
    run_combine(a, m0, dtype, [(0.1, a, m1, (1, 1))], 3, width, (1, 1), what=f"{cell}: member to member")
    run_combine(a, m1, dtype, [(-1.0, a, m1, (0, 0)), (0.1, b, offsets[-1], (0, 3))], 4, width, what=f"{cell}: in place")
    run_combine(a, m0, dtype, [(0.5, a, m0, (2, 1)), (0.0, a, m1, (2, 1)), (huge_coef(dtype), p, 0, (0, 0)), (0.1, b, m0, (0, 4))],
                3, width, (2, 1), what=f"{cell}: four terms")
    # a plane from members, and a member from a plane alone
    run_combine(p, 0, dtype, [(2.0, a, m1, (0, 1)), (-1.0, b, m0, (1, 0))], 3, width, (0, 1), what=f"{cell}: members into a plane")
    run_combine(b, offsets[-1], dtype, [(0.1, p, 0, (1, 0))], 2, width, (2, 2), what=f"{cell}: a plane into a member")


def test_more_rows_than_row_workgroups(gpu):
    """2051 x 3: more rows than the launch has workgroups, so a workgroup walks several rows."""
    for dtype in (F32, F64):
        x, y = plane(gpu, dtype, 2051, 5, seed=21, width=4), plane(gpu, dtype, 2051, 3, seed=22)
        run_combine(x, 0, dtype, [(0.1, x, 0, (0, 1)), (-1.0, y, 0, (0, 0))], 2051, 3, (0, 1), what="2051 x 3 planes")
    cells = cell_buffer(gpu, "fdtd", 2051, 3, seed=23)
    run_combine(cells, 8, F32, [(1.0, cells, 8, (0, 0)), (0.1, cells, 28, (0, 0))], 2051, 3, what="2051 x 3 members")
    fine = plane(gpu, F32, 4102, 6, seed=24)
    coarse = plane(gpu, F32, 2051, 3, seed=25)
    run_resample(RESTRICT, coarse, 0, fine, 0, F32, 2051, 3, what="restrict to 2051 x 3")
    run_resample(PROLONG, fine, 0, coarse, 0, F32, 2051, 3, halo=1.5, what="prolong from 2051 x 3")


def test_coefficients_are_rounded_once_on_the_host(gpu):
    """0.1 is no float: the model multiplies by np.float32(0.1), and by 0.1 for doubles."""
    for dtype in (F32, F64):
        x = plane(gpu, dtype, 3, 70, seed=3)
        y = plane(gpu, dtype, 3, 70, seed=4)
        for coef in (0.1, 1.0 / 3.0, -0.7, 1e-40, 0.0, -0.0):
            run_combine(y, 0, dtype, [(coef, x, 0, (0, 0))], 3, 70, what=f"coefficient {coef!r}")


# ------------------------------------------------------------------ restrict and prolong
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_restrict_planes(gpu, dtype, width):
    """`width` coarse columns from planes whose bases are shifted by 0..3 elements, from even and odd source rows and
    columns: the 16-byte path, its odd tail and the element path."""
    n_calls = 0
    for shift in range(4):
        fine = plane(gpu, dtype, 7, 2 * width + 3 + shift, seed=100 * width + shift, shift=shift)
        coarse = plane(gpu, dtype, 4, width + 2, seed=100 * width + 10 + shift, shift=(3 * shift) % 4)
        for src_at, dst_at in (((0, 0), (0, 0)), ((1, 0), (1, 2)), ((0, 1), (1, 1)), ((1, 3), (0, 2)), ((0, 2), (1, 0))):
            run_resample(RESTRICT, coarse, 0, fine, 0, dtype, 3, width, dst_at, src_at,
                         what=f"restrict to width {width}, shift {shift}, from {src_at} to {dst_at}")
            n_calls += 1
        fine.unchanged("restrict")
    assert n_calls == 20


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_prolong_planes(gpu, dtype, width):
    """Whole grids (all four borders read the halo: 0, a non-zero value and NaN) and inner rectangles whose neighbours
    come from the view, into planes whose bases are shifted by 0..3 elements (paired and single stores)."""
    n_calls = 0
    for shift, halo in ((0, 0.0), (1, -2.5), (2, float("nan")), (3, 0.1)):
        coarse = plane(gpu, dtype, 3, width + 2 + shift, seed=200 * width + shift, width=width, shift=(shift * 3) % 4)
        fine = plane(gpu, dtype, 7, 2 * width + 2, seed=200 * width + 10 + shift, shift=shift)
        run_resample(PROLONG, fine, 0, coarse, 0, dtype, 3, width, (1, shift % 3), (0, 0), halo,
                     what=f"prolong a whole {3} x {width} grid, halo {halo}")
        n_calls += 1
        if width >= 3:  # an inner rectangle: every neighbour is a cell of the view
            run_resample(PROLONG, fine, 0, coarse, 0, dtype, 1, width - 2, (0, 1), (1, 1), halo,
                         what=f"prolong the inside of a 3 x {width} grid, halo {halo}")
            n_calls += 1
        coarse.unchanged("prolong")
    assert n_calls == (8 if width >= 3 else 4)


@pytest.mark.parametrize("halo", [0.0, 3.25, float("nan")], ids=["zero", "value", "nan"])
def test_prolong_rectangles_at_each_border(gpu, halo):
    """Rectangles of a 9 x 11 coarse grid that touch one border each, two, or none: outside the view the halo, outside
    the rectangle the view."""
    for dtype in (F32, F64):
        coarse = plane(gpu, dtype, 9, 13, seed=31, width=11)
        fine = plane(gpu, dtype, 18, 22, seed=32)
        rects = {"top": (0, 3, 4, 7), "bottom": (6, 9, 4, 7), "left": (3, 6, 0, 3), "right": (3, 6, 8, 11),
                 "top left": (0, 2, 0, 2), "bottom right": (7, 9, 9, 11), "inside": (2, 7, 3, 8), "whole": (0, 9, 0, 11),
                 "one cell inside": (4, 5, 5, 6), "a corner cell": (8, 9, 0, 1)}
        for name, (r0, r1, c0, c1) in rects.items():
            run_resample(PROLONG, fine, 0, coarse, 0, dtype, r1 - r0, c1 - c0, (2 * r0, 2 * c0), (r0, c0), halo,
                         what=f"prolong the {name} of a 9 x 11 grid, halo {halo}")


def test_one_by_one_coarse_grid(gpu):
    for dtype in (F32, F64):
        for halo in (0.0, -1.5, float("nan")):
            coarse = plane(gpu, dtype, 1, 1, seed=41)
            fine = plane(gpu, dtype, 2, 2, seed=42)
            run_resample(PROLONG, fine, 0, coarse, 0, dtype, 1, 1, halo=halo, what=f"prolong a 1 x 1 grid, halo {halo}")
            run_resample(RESTRICT, coarse, 0, fine, 0, dtype, 1, 1, what="restrict to a 1 x 1 grid")


@pytest.mark.parametrize("cell", sorted(CELLS))
def test_transfers_between_members_of_cells(gpu, cell):
    """Restrict and prolong between members of AoS cells and planes, whole grids and inner rectangles from odd rows and
    columns; the other members keep their bytes."""
    stride, dtype, offsets = CELLS[cell]
    h, w = 5, 1025  # coarse
    fine = cell_buffer(gpu, cell, 2 * h, 2 * w + 1, seed=51, width=2 * w)
    coarse = cell_buffer(gpu, cell, h, w, seed=52)
    p = plane(gpu, dtype, 2 * h, 2 * w, seed=53)
    run_resample(RESTRICT, coarse, offsets[0], fine, offsets[1], dtype, h, w, what=f"{cell}: restrict member to member")
    run_resample(RESTRICT, coarse, offsets[-1], fine, offsets[0], dtype, 2, w - 2, (1, 1), (3, 1), what=f"{cell}: restrict a rectangle")
    run_resample(RESTRICT, coarse, offsets[1], p, 0, dtype, h, w, what=f"{cell}: restrict a plane into a member")
    run_resample(PROLONG, fine, offsets[-1], coarse, offsets[0], dtype, h, w, halo=0.5, what=f"{cell}: prolong member to member")
    run_resample(PROLONG, fine, offsets[0], coarse, offsets[1], dtype, 2, w - 3, (2, 4), (1, 2), halo=float("nan"),
                 what=f"{cell}: prolong a rectangle")
    run_resample(PROLONG, p, 0, coarse, offsets[-1], dtype, h - 1, w, (2, 0), (1, 0), halo=-1.0, what=f"{cell}: prolong a member into a plane")


# ------------------------------------------------------------------ special values
@pytest.mark.parametrize("kind", ["planted", "tiny", "huge"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_special_values(gpu, dtype, kind):
    """Subnormal, non-finite and signed-zero inputs: products that underflow to subnormals and zeros of either sign,
    sums that overflow, inf - inf; subnormal results are kept."""
    make = {"planted": lambda shape, seed, dt: SV.planted(shape, seed, dtype=dt),
            "tiny": lambda shape, seed, dt: SV.tiny(shape, seed, dtype=dt),
            "huge": lambda shape, seed, dt: SV.huge(shape, seed, dtype=dt)}[kind]
    h, w = 12, 134  # fine: even, wider than 128 so that `planted` has its seam
    x, y, z = (plane(gpu, dtype, h, w, seed=60 + k, values=make) for k in range(3))
    if kind != "huge":
        sub = SV.classify(x.field(0, dtype))["subnormal"]
        assert sub > 0, "the inputs hold no subnormal"
    out = plane(gpu, dtype, h, w, seed=70)
    run_combine(out, 0, dtype, [(1.0, x, 0, (0, 0)), (-1.0, y, 0, (0, 0))], h, w, what=f"{kind}: x - y")
    run_combine(out, 0, dtype, [(0.5, x, 0, (0, 0)), (0.25, y, 0, (0, 0)), (2.0, z, 0, (0, 0)), (-0.0, out, 0, (0, 0))],
                h, w, what=f"{kind}: four terms")
    run_combine(out, 0, dtype, [(0.1, x, 0, (0, 0))], h, w, what=f"{kind}: 0.1 x")
    if kind == "tiny":  # a result below the smallest normal stays what it is
        assert SV.classify(out.field(0, dtype))["subnormal"] > 0.1
    coarse = plane(gpu, dtype, h // 2, w // 2, seed=71)
    run_resample(RESTRICT, coarse, 0, x, 0, dtype, h // 2, w // 2, what=f"{kind}: restrict")
    for halo in (0.0, float("inf"), float("nan"), float(np.finfo(dtype).smallest_subnormal)):
        small = plane(gpu, dtype, h // 2, w // 2, seed=72, values=make)
        run_resample(PROLONG, out, 0, small, 0, dtype, h // 2, w // 2, halo=halo, what=f"{kind}: prolong, halo {halo}")
    # members of cells take the same path as far as the arithmetic goes; once through the strided kernels
    cells = cell_buffer(gpu, "fdtd" if dtype == F32 else "fdtd f64", h, w, seed=73, values=make)
    offsets = CELLS["fdtd" if dtype == F32 else "fdtd f64"][2]
    run_combine(cells, offsets[0], dtype, [(1.0, cells, offsets[0], (0, 0)), (-1.0, cells, offsets[1], (0, 0)), (0.1, cells, offsets[2], (0, 0))],
                h, w, what=f"{kind}: members")


# ------------------------------------------------------------------ several entries
def test_eight_entries_in_one_call(gpu):
    from stencilstream_amd import capi

    outs = [plane(gpu, F32 if k % 2 == 0 else F64, 6, 40 + k, seed=80 + k) for k in range(8)]
    ins = [plane(gpu, F32 if k % 2 == 0 else F64, 6, 40 + k, seed=90 + k) for k in range(8)]
    made = [combine(outs[k], 0, F32 if k % 2 == 0 else F64, [(0.1 * (k + 1), ins[k], 0, (0, 0)), (1.0, outs[k], 0, (k % 3, k % 5))][:1 + k % 2],
                    6 - k % 3, 40 + k - k % 5, (k % 3, k % 5)) for k in range(8)]
    capi.grid_combine([desc for desc, _ in made])
    for k, (_, want) in enumerate(made):
        dt = F32 if k % 2 == 0 else F64
        outs[k].settle(0, dt, (k % 3, 6), (k % 5, 40 + k), want, f"entry {k} of eight combines")

    fines = [plane(gpu, F32 if k % 2 == 0 else F64, 8, 20 + 2 * k, seed=110 + k) for k in range(8)]
    coarses = [plane(gpu, F32 if k % 2 == 0 else F64, 4, 10 + k, seed=120 + k) for k in range(8)]
    made = []
    for k in range(8):
        dt = F32 if k % 2 == 0 else F64
        if k < 4:
            made.append((coarses[k], dt) + resample(RESTRICT, coarses[k], 0, fines[k], 0, dt, 4, 10 + k))
        else:
            made.append((fines[k], dt) + resample(PROLONG, fines[k], 0, coarses[k], 0, dt, 4, 10 + k, halo=float(k)))
    capi.grid_resample([m[2] for m in made])
    for k, (buf, dt, _, (rows, cols), want) in enumerate(made):
        buf.settle(0, dt, rows, cols, want, f"entry {k} of eight transfers")


# ------------------------------------------------------------------ update.Grid
def test_a_two_grid_chain_through_update_grid(gpu):
    """64 x 96 fine: restrict -> combine -> prolong -> combine through update.Grid equals the same chain in numpy;
    members of HotSpot cells on the fine side, planes on the coarse side."""
    from stencilstream_amd import update as U

    rng = np.random.default_rng(0xA16)
    fine_host = np.zeros((64, 96), dtype=U.HOTSPOT_CELL)
    fine_host["temp"] = rng.random((64, 96), dtype=np.float32) - 0.5
    fine_host["power"] = rng.random((64, 96), dtype=np.float32)
    guess_host = (rng.random((32, 48), dtype=np.float32) - 0.5).astype("<f4")
    fine, guess = U.Grid.from_numpy(fine_host, device=gpu), U.Grid.from_numpy(guess_host, device=gpu)
    coarse = U.Grid(32, 48, "<f4", device=gpu)
    correction = U.Grid(64, 96, "<f4", device=gpu)

    coarse.restrict_from(fine, src_field="power")                          # r = R(power)
    coarse.combine([(0.1, coarse), (-1.0, guess)])                         # e = 0.1 r - guess
    correction.prolong_from(coarse, halo=0.25)                             # P(e)
    fine.combine([(1.0, fine, "temp"), (0.7, correction)], field="temp", rows=(1, 63), cols=(2, 96))

    r = restrict_model(F32, fine_host["power"].copy())
    e = combine_model(F32, [0.1, -1.0], [r, guess_host])
    p = prolong_model(F32, e, (0, 0), 32, 48, 0.25)
    want = fine_host.copy()
    want["temp"][1:63, 2:96] = combine_model(F32, [1.0, 0.7], [fine_host["temp"][1:63, 2:96], p[1:63, 2:96]])
    SV.assert_same_cells(coarse.to_numpy(), e, "the coarse grid")
    SV.assert_same_cells(correction.to_numpy(), p, "the prolonged correction")
    got = fine.to_numpy()
    SV.assert_same_cells(got["temp"], want["temp"], "temp")
    assert np.array_equal(got["power"].view(np.uint32), fine_host["power"].view(np.uint32)), "power changed"
    # the same through read(): a queued call is ordered in front of it
    SV.assert_same_cells(fine.read(rows=(0, 3), field="temp"), want["temp"][0:3], "temp through read()")


def test_update_grid_doubles_and_empty_ranges(gpu):
    from stencilstream_amd import update as U

    rng = np.random.default_rng(5)
    host = np.zeros((6, 10), dtype=U.HOTSPOT_CELL_F64)
    host["temp"], host["power"] = rng.random((6, 10)), rng.random((6, 10))
    grid = U.Grid.from_numpy(host, device=gpu)
    grid.combine([(2.0, grid, "power")], field="temp", rows=(2, 2))  # nothing
    grid.combine([(1.0 / 3.0, grid, "temp"), (-0.1, grid, "power")], field="temp")
    want = combine_model(F64, [1.0 / 3.0, -0.1], [host["temp"], host["power"]])
    SV.assert_same_cells(grid.to_numpy()["temp"], want, "doubles in place")
    coarse = U.Grid(3, 5, "<f8", device=gpu)
    coarse.restrict_from(grid, src_field="temp")
    SV.assert_same_cells(coarse.to_numpy(), restrict_model(F64, want), "restricted doubles")
    grid.prolong_from(coarse, halo=float("nan"), field="power")
    SV.assert_same_cells(grid.to_numpy()["power"], prolong_model(F64, restrict_model(F64, want), (0, 0), 3, 5, float("nan")),
                         "prolonged doubles")

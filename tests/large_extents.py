"""Grids whose rows lie gigabytes apart, rectangles far into a row, rows of more segments than a launch has workgroups
and the longest row ststhip.h admits: the case table of tests/test_large_extents_gpu.py and what it builds them from.
A plain module (imported by name from the tests beside it), no fixtures.  The table and everything tests/
test_large_extents_cpu.py asks of it is Python integers; torch is imported only where a buffer is made.

A CASE is one GPU test: a few buffers, and the operations that run on them one after the other.

  * A `View` is ststhip_grid_view in bytes: the `elem` bytes at `offset` of the cells of buffer `buf`, cells `stride`
    bytes apart within a row and `pitch` cells from row to row.  A huge pitch puts a few rows gigabytes apart; a
    `Rect` of it touches a few thousand cells per row, so the buffers are large and the work is tiny.
  * The data: cell (r, c) of operand k holds ((131 r + 7 c + 17 k) mod 251) - 125 (`coded`): neighbours differ, and a
    row or a column read from the wrong place reads another value.  With small dyadic weights every product and every
    sum of the operations is exact in fp32, so any correct order of evaluation gives the same bits, and sums of values,
    of squares and of products are integers far below 2^53.
  * An `Arena` is one buffer on the device: FRONT_GUARD = 2^31 + 4096 bytes in front of the cells, so that a row offset
    cut to 32 bits (which lands lower) and one sign-extended from 32 bits (which lands at most 2^31 lower) still land
    inside the allocation: a kernel with such a defect returns wrong values, it does not fault.  All of it holds a
    sentinel (a NaN with a payload; 0xA5 bytes for the Game of Life) but the rectangles an operation is given; after
    the call the result is copied out, the sentinel is put back over the rectangles through torch views and the WHOLE
    buffer, guards included, must be the sentinel again.  A stray read of a reduction reads a NaN and shows in
    n_nonfinite."""
import os
import re
from dataclasses import dataclass, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stencilstream_amd", "csrc")

GiB = 1 << 30
FRONT_GUARD = (1 << 31) + 4096
BACK_GUARD = 4096
MAX_NEED = 40 * GiB     # no test may need more
HEADROOM = 4 * GiB      # a test skips unless need + HEADROOM bytes are free (never on an MI355X: 288 GB)
SENTINEL_F32 = 0x7FC00BAD
SENTINEL_F64 = 0x7FF8000000000BAD
SENTINEL_BYTES = 0xA5A5A5A5 - (1 << 32)  # four bytes 0xA5 as a signed 32-bit word


# ------------------------------------------------------------------------------------------ the kernels' constants
def kernel_constants(file_name):
    """Every `constexpr unsigned NAME = <product of integers and earlier names>;` of a file under csrc/."""
    out = {}
    with open(os.path.join(CSRC, file_name)) as f:
        for name, expr in re.findall(r"constexpr unsigned (\w+) = ([\w *]+);", f.read()):
            value = 1
            for factor in expr.split("*"):
                factor = factor.strip()
                if factor.isdigit():
                    value *= int(factor)
                elif factor in out:
                    value *= out[factor]
                else:
                    value = None
                    break
            if value is not None:
                out[name] = value
    return out


def segments_of(family):
    """{layout: (cells of an f32 row per workgroup, cap of workgroups per launch)} of a family of kernels."""
    if family == "regions":
        k = kernel_constants("regions.hip")
        return {"dense": (k["region_segment_bytes"] // 4, k["region_block_cap"]),
                "strided": (k["region_segment_cells"], k["region_block_cap"])}
    if family == "algebra":
        k = kernel_constants("algebra.hip")
        return {"dense": (k["algebra_segment_bytes"] // 4, k["algebra_block_cap"]),
                "strided": (k["algebra_segment_cells"], k["algebra_block_cap"])}
    if family == "stencil":  # (the dense kernel has no segments: a workgroup takes stencil_threads units of a row)
        k = kernel_constants("stencil.hip")
        return {"dense": (k["stencil_segment_cells"], k["stencil_block_cap"]),
                "strided": (k["stencil_segment_cells"], k["stencil_block_cap"])}
    if family == "norms":
        k = kernel_constants("norms.hip")
        return {"dense": (k["norm_segment_bytes"] // 4, k["norm_block_cap"]),
                "strided": (k["norm_segment_cells"], k["norm_block_cap"])}
    if family == "dot":
        k = kernel_constants("dot.hip")
        return {"dense": (k["dot_segment_bytes"] // 4, k["dot_block_cap"]),
                "strided": (k["dot_segment_cells"], k["dot_block_cap"])}
    raise KeyError(family)


# ------------------------------------------------------------------------------------------ views and rectangles
@dataclass(frozen=True)
class View:
    buf: str        # the buffer its cells lie in
    k: int          # the operand number its values are coded with
    elem: int       # bytes of an element
    stride: int     # bytes between neighbouring cells of a row
    pitch: int      # cells between neighbouring rows
    height: int
    width: int
    offset: int = 0  # of the member inside the cell

    @property
    def row_bytes(self):
        return self.pitch * self.stride

    @property
    def dense(self):
        return self.stride == self.elem

    def extent(self):
        """Bytes from cell (0, 0) to the end of the last cell."""
        return ((self.height - 1) * self.pitch + self.width) * self.stride

    def at(self, r, c):
        """Byte offset of element (r, c) from cell (0, 0) of the buffer."""
        return (r * self.pitch + c) * self.stride + self.offset


@dataclass(frozen=True)
class Rect:
    view: View
    row: int
    col: int
    n_rows: int
    n_cols: int
    row_step: int = 1
    col_step: int = 1

    def rows(self):
        return [self.row + i * self.row_step for i in range(self.n_rows)]

    def first(self):
        return self.view.at(self.row, self.col)

    def last_byte(self):
        v = self.view
        return v.at(self.row + (self.n_rows - 1) * self.row_step, self.col + (self.n_cols - 1) * self.col_step) + v.elem - 1

    def row_distance(self):
        return self.view.row_bytes * self.row_step

    def row_extent(self):
        """n_cols * step * stride, the quantity ststhip.h limits to below 2^31."""
        return self.n_cols * self.col_step * self.view.stride

    def widened(self):
        """The rectangle with the neighbours a stencil or a prolongation reads, where they lie inside the view."""
        assert self.row_step == 1 and self.col_step == 1
        r0, c0 = max(self.row - 1, 0), max(self.col - 1, 0)
        r1, c1 = min(self.row + self.n_rows + 1, self.view.height), min(self.col + self.n_cols + 1, self.view.width)
        return Rect(self.view, r0, c0, r1 - r0, c1 - c0)

    def admitted(self):
        """The documented limits of ststhip.h: extents below 2^31, a row of the rectangle below 2^31 bytes, the view
        below 2^63 bytes, the rectangle inside the view."""
        v = self.view
        return (self.n_rows < 1 << 31 and self.n_cols < 1 << 31 and self.row_extent() < 1 << 31
                and v.pitch >= v.width and v.row_bytes * (v.height + 1) < 1 << 63
                and self.row + (self.n_rows - 1) * self.row_step < v.height
                and self.col + (self.n_cols - 1) * self.col_step < v.width)


def code_of(k, r, c):
    """What cell (r, c) of operand k holds.  r, c: Python integers, numpy or torch integer arrays that broadcast."""
    return (131 * r + 7 * c + 17 * k) % 251 - 125


# two models of a defective kernel: the byte offset of a rectangle's row i, i * row distance, formed in 32 bits
def kept_to_32_bits(offset):
    return offset & 0xFFFFFFFF


def sign_extended_from_32_bits(offset):
    low = offset & 0xFFFFFFFF
    return low - (1 << 32) if low >> 31 else low


def value_at_byte(rect, byte):
    """What the element-sized load at `byte` (from cell (0, 0) of the buffer) returns while `rect` holds its coded
    values and everything else the sentinel: the coded value, or None for sentinel bytes and for the guards."""
    v = rect.view
    if byte < 0:
        return None
    cell, inner = divmod(byte, v.stride)
    r, c = divmod(cell, v.pitch)
    if inner != v.offset:
        return None
    dr, dc = r - rect.row, c - rect.col
    if dr % rect.row_step or dc % rect.col_step or not (0 <= dr // rect.row_step < rect.n_rows) \
            or not (0 <= dc // rect.col_step < rect.n_cols):
        return None
    return code_of(v.k, r, c)


# ------------------------------------------------------------------------------------------ operations and cases
@dataclass(frozen=True)
class Op:
    name: str
    kind: str                # copy, fill, download, upload, combine, restrict, prolong, stencil, norms, distance, dot, max_abs
    dst: object = None       # a Rect, or None for reductions
    srcs: tuple = ()         # the Rects it reads
    par: dict = field(default_factory=dict)

    def rects(self):
        return tuple(r for r in (self.dst,) + tuple(self.srcs) if r is not None)


@dataclass(frozen=True)
class Case:
    id: str
    family: str
    geometry: str            # G1 ... G5, "G1xG2", "sweep"
    crosses: tuple           # what it is named for: "2^31", "2^32", "segments", "row"
    ops: tuple
    extra: int = 16 << 20    # bytes of device memory beside the buffers: results copied out, references

    def views(self):
        """One view per buffer (the widest cells decide the size)."""
        out = {}
        for op in self.ops:
            for r in op.rects():
                v = r.view
                if v.buf is None:  # (host memory)
                    continue
                if v.buf not in out or v.extent() > out[v.buf].extent():
                    out[v.buf] = v
        return out

    def need(self):
        """Bytes of device memory the test asks for."""
        return sum(arena_bytes(v) for v in self.views().values()) + self.extra


def arena_bytes(view):
    return -(-(FRONT_GUARD + view.extent() + BACK_GUARD) // 16) * 16


P29, P30 = 1 << 29, 1 << 30
HALO = 1000.5                                   # no cell holds it
BOX = (0.5, -2.0, 0.25, 1.0, -0.5, 2.0, -0.25, 0.125, -1.0)
CROSS = (0.0, -2.0, 0.0, 1.0, -0.5, 2.0, 0.0, 0.125, 0.0)
BOX9, CROSS5 = 1, 0


def plane(buf, k, pitch, height, width, elem=4):
    return View(buf, k, elem, elem, pitch, height, width)


def hotspot(buf, k, member, pitch, height, width):
    """HotSpot cells: 8 bytes, temp at 0 and power at 4."""
    return View(buf, k, 4, 8, pitch, height, width, {"temp": 0, "power": 4}[member])


def fdtd(buf, k, offset, pitch, height, width):
    """FDTD cells: 32 bytes, eight floats (hz at 8, hz_sum at 12)."""
    return View(buf, k, 4, 32, pitch, height, width, offset)


def whole(view, rows=None, cols=(5, 8205)):
    rows = (0, view.height) if rows is None else rows
    return Rect(view, rows[0], cols[0], rows[1] - rows[0], cols[1] - cols[0])


def geometry_views(g):
    """The operands of a geometry: planes P and Q, and cells whose rows lie as far apart."""
    if g == "G1":    # rows 2^31 + 12 bytes apart (cells: 2^31 + 24), four of them
        return dict(P=plane("P", 0, P29 + 3, 4, 9000), Q=plane("Q", 1, P29 + 3, 4, 9000),
                    temp=hotspot("C", 2, "temp", (1 << 28) + 3, 4, 9000), power=hotspot("C", 3, "power", (1 << 28) + 3, 4, 9000))
    if g == "G1f64":  # the f64 twin: rows 2^31 + 24 bytes apart
        return dict(P=plane("P", 0, (1 << 28) + 3, 4, 9000, 8), Q=plane("Q", 1, (1 << 28) + 3, 4, 9000, 8))
    if g == "G2":    # rows 2^32 + 16 bytes apart (FDTD cells: 2^32 + 32), three of them
        return dict(P=plane("P", 0, P30 + 4, 3, 9000), Q=plane("Q", 1, P30 + 4, 3, 9000),
                    temp=hotspot("C", 2, "temp", P29 + 2, 3, 9000), power=hotspot("C", 3, "power", P29 + 2, 3, 9000),
                    hz=fdtd("F", 4, 8, (1 << 27) + 1, 3, 9000), hz_sum=fdtd("F", 5, 12, (1 << 27) + 1, 3, 9000))
    if g == "G3":    # two rows of 6 GiB
        return dict(P=plane("P", 0, 3 * P29, 2, 3 * P29), Q=plane("Q", 1, 3 * P29, 2, 3 * P29))
    if g == "G5":    # rows of 2^31 - 4 bytes
        return dict(P=plane("P", 0, P29 + 1, 2, P29 - 1), Q=plane("Q", 1, P29 + 1, 2, P29 - 1),
                    R=plane("R", 2, P29 + 1, 2, P29 - 1))
    raise KeyError(g)


FAR_A, FAR_B = P29 + 1, P30 + 7   # G3: byte 2^31 + 4 and byte 2^32 + 28 of a row
G5_CELLS = 2 * (P29 - 1)


def g3(view, col, n_cols=3000):
    return Rect(view, 0, col, 2, n_cols)


def host(k, n_rows, n_cols):
    """A small pinned host array as a view (no Arena: buf None)."""
    return Rect(View(None, k, 4, 4, n_cols + 3, n_rows, n_cols), 0, 0, n_rows, n_cols)


def region_cases():
    out = []
    v = geometry_views("G1")
    P, Q = whole(v["P"]), whole(v["Q"])
    out.append(Case("regions-G1", "regions", "G1", ("2^31", "2^32"), (
        Op("plane to plane (dense)", "copy", Q, (P,)),
        Op("member to plane", "copy", Q, (whole(v["temp"]),)),
        Op("plane to member", "copy", whole(v["power"]), (P,)),
        Op("every second source row", "copy", whole(v["Q"], (2, 4)), (Rect(v["P"], 1, 5, 2, 8200, row_step=2),)),
        Op("fill", "fill", Q, (), {"value": -77.0}),
        Op("download", "download", host(0, 4, 8200), (P,)),
        Op("upload", "upload", Q, (host(6, 4, 8200),)),
    )))
    v = geometry_views("G2")
    P, Q = whole(v["P"]), whole(v["Q"])
    out.append(Case("regions-G2-hotspot", "regions", "G2", ("2^31", "2^32"), (
        Op("plane to plane (dense)", "copy", Q, (P,)),
        Op("member to plane", "copy", Q, (whole(v["temp"]),)),
        Op("plane to member", "copy", whole(v["power"]), (P,)),
        Op("fill", "fill", whole(v["power"]), (), {"value": -77.0}),
        Op("download", "download", host(2, 3, 8200), (whole(v["temp"]),)),
        Op("upload", "upload", Q, (host(6, 3, 8200),)),
    )))
    out.append(Case("regions-G2-fdtd", "regions", "G2", ("2^31", "2^32"), (
        Op("member to plane", "copy", P, (whole(v["hz"]),)),
        Op("plane to member", "copy", whole(v["hz_sum"]), (P,)),
        Op("member to member of the same cells", "copy", whole(v["hz_sum"]), (whole(v["hz"]),)),
        Op("fill", "fill", whole(v["hz"]), (), {"value": -77.0}),
        Op("upload", "upload", whole(v["hz"]), (host(6, 3, 8200),)),
    )))
    v = geometry_views("G3")
    out.append(Case("regions-G3", "regions", "G3", ("2^31", "2^32"), (
        Op("plane to plane (dense), from 2^32 + 28 to 2^31 + 4", "copy", g3(v["Q"], FAR_A), (g3(v["P"], FAR_B),)),
        Op("plane to plane (dense), from 2^31 + 4 to 2^32 + 28", "copy", g3(v["Q"], FAR_B), (g3(v["P"], FAR_A),)),
        Op("every second source column (strided)", "copy", g3(v["Q"], FAR_B), (Rect(v["P"], 0, FAR_B, 2, 3000, col_step=2),)),
        Op("fill", "fill", g3(v["Q"], FAR_B), (), {"value": -77.0}),
        Op("download", "download", host(0, 2, 3000), (g3(v["P"], FAR_B),)),
        Op("upload", "upload", g3(v["Q"], FAR_B), (host(6, 2, 3000),)),
    )))
    v = geometry_views("G5")
    P, Q = Rect(v["P"], 0, 0, 2, P29 - 1), Rect(v["Q"], 0, 0, 2, P29 - 1)
    out.append(Case("regions-G5", "regions", "G5", ("row",), (
        Op("plane to plane (dense)", "copy", Q, (P,)),
        Op("fill", "fill", Q, (), {"value": -77.0}),
    ), extra=6 * GiB))
    return out


def coarse(k, n_rows, n_cols):
    """A small coarse plane: one row and one column more than the rectangle on the far sides, so that a prolongation
    reads the halo at the top and on the left and cells of the view at the bottom and on the right."""
    return Rect(plane("S", k, n_cols + 4, n_rows + 1, n_cols + 1), 0, 0, n_rows, n_cols)


def algebra_cases():
    out = []
    for g, dist in (("G1", "2^31 + 12"), ("G2", "2^32 + 16")):
        v = geometry_views(g)
        h = v["P"].height
        P, Q = whole(v["P"]), whole(v["Q"])
        S = coarse(7, h // 2, 4100)
        fine_rows = (h - 2 * (h // 2), h)   # the last 2 * (h // 2) rows: the farthest
        out.append(Case(f"algebra-{g}-planes", "algebra", g, ("2^31", "2^32"), (
            Op(f"two terms of one plane, rows {dist} apart (dense)", "combine", whole(v["Q"], (1, h)),
               (whole(v["P"], (0, h - 1)), whole(v["P"], (1, h))), {"coefs": (0.5, -2.0)}),
            Op("in place (dense)", "combine", Q, (Q, P), {"coefs": (0.25, -2.0)}),
            Op("restrict_mean from the far rows", "restrict", S, (whole(v["P"], fine_rows, (5, 8205)),)),
            Op("prolong_bilinear into the far rows", "prolong", whole(v["Q"], fine_rows, (5, 8205)), (S,), {"halo": HALO}),
        )))
    v = geometry_views("G1")
    out.append(Case("algebra-G1-members", "algebra", "G1", ("2^31", "2^32"), (
        Op("a member of the same cells and a plane", "combine", whole(v["power"]), (whole(v["temp"]), whole(v["P"])),
           {"coefs": (0.25, -2.0)}),
        Op("in place on a member", "combine", whole(v["temp"]), (whole(v["temp"]), whole(v["P"])), {"coefs": (0.5, 0.25)}),
    )))
    v = geometry_views("G2")
    out.append(Case("algebra-G2-members", "algebra", "G2", ("2^31", "2^32"), (
        Op("members of two kinds of cells", "combine", whole(v["power"]), (whole(v["temp"]), whole(v["hz"])),
           {"coefs": (0.25, -2.0)}),
        Op("in place on a member", "combine", whole(v["hz_sum"]), (whole(v["hz_sum"]), whole(v["temp"])), {"coefs": (0.5, 0.25)}),
    )))
    v = geometry_views("G1f64")
    P, Q = whole(v["P"]), whole(v["Q"])
    out.append(Case("algebra-G1-f64", "algebra", "G1", ("2^31", "2^32"), (
        Op("two terms of one plane (dense)", "combine", whole(v["Q"], (1, 4)), (whole(v["P"], (0, 3)), whole(v["P"], (1, 4))),
           {"coefs": (0.5, -2.0)}),
        Op("in place (dense)", "combine", Q, (Q, P), {"coefs": (0.25, -2.0)}),
    )))
    v = geometry_views("G3")
    out.append(Case("algebra-G3", "algebra", "G3", ("2^31", "2^32"), (
        Op("two far rectangles of one plane (dense)", "combine", g3(v["Q"], FAR_B), (g3(v["P"], FAR_A), g3(v["P"], FAR_B)),
           {"coefs": (0.5, -2.0)}),
        Op("in place (dense)", "combine", g3(v["Q"], FAR_B), (g3(v["Q"], FAR_B), g3(v["P"], FAR_B)), {"coefs": (0.25, -2.0)}),
    )))
    v = geometry_views("G5")
    n = P29 - 1
    P, Q, R = (Rect(v[x], 0, 0, 2, n) for x in "PQR")
    out.append(Case("algebra-G5-combine", "algebra", "G5", ("row",), (
        Op("two terms (dense)", "combine", R, (P, Q), {"coefs": (0.5, -2.0)}),), extra=10 * GiB))
    small = Rect(plane("S", 7, (1 << 28) + 1, 1, (1 << 28) - 1), 0, 0, 1, (1 << 28) - 1)
    out.append(Case("algebra-G5-transfers", "algebra", "G5", ("row",), (
        Op("restrict_mean", "restrict", small, (Rect(v["P"], 0, 0, 2, n - 1),)),
        Op("prolong_bilinear", "prolong", Rect(v["Q"], 0, 0, 2, n - 1), (small,), {"halo": HALO}),
    ), extra=14 * GiB))
    return out


def stencil_cases():
    out = []

    def ops(dst, src, rhs, member_dst=None, member_src=None):
        made = [
            Op("BOX9 (dense)", "stencil", dst, (src,), {"shape": BOX9, "weights": BOX, "halo": HALO}),
            Op("BOX9 with the destination as right-hand side (dense)", "stencil", dst, (src, rhs),
               {"shape": BOX9, "weights": BOX, "halo": HALO, "rhs_coef": 0.25}),
            Op("BOX9 (general)", "stencil", dst, (src,), {"shape": BOX9, "weights": BOX, "halo": HALO, "general": True}),
            Op("BOX9 with a right-hand side (general)", "stencil", dst, (src, rhs),
               {"shape": BOX9, "weights": BOX, "halo": HALO, "rhs_coef": 0.25, "general": True}),
            Op("CROSS5", "stencil", dst, (src,), {"shape": CROSS5, "weights": CROSS, "halo": HALO}),
        ]
        if member_dst is not None:
            made += [Op("BOX9 on members", "stencil", member_dst, (member_src,), {"shape": BOX9, "weights": BOX, "halo": HALO}),
                     Op("CROSS5 on members", "stencil", member_dst, (member_src,), {"shape": CROSS5, "weights": CROSS, "halo": HALO})]
        return tuple(made)

    # G1: rows 1 to 3 of four (the view ends below, row 3 begins beyond 3 * 2^31), and rows 0 to 2 (it ends above)
    v = geometry_views("G1")
    Q = whole(v["Q"], (1, 4))
    upper = (Op("BOX9 (dense), rows 0 to 2", "stencil", whole(v["Q"], (0, 3)), (whole(v["P"], (0, 3)),),
                {"shape": BOX9, "weights": BOX, "halo": HALO}),)
    out.append(Case("stencil-G1", "stencil", "G1", ("2^31", "2^32"),
                    ops(Q, whole(v["P"], (1, 4)), Q, whole(v["power"], (1, 4)), whole(v["temp"], (1, 4))) + upper))
    v = geometry_views("G2")  # rows 1 and 2 of three: the view ends below; 16-byte units with a head of three elements
    Q = whole(v["Q"], (1, 3))
    upper = (Op("BOX9 (dense), rows 0 and 1", "stencil", whole(v["Q"], (0, 2)), (whole(v["P"], (0, 2)),),
                {"shape": BOX9, "weights": BOX, "halo": HALO}),)
    out.append(Case("stencil-G2", "stencil", "G2", ("2^31", "2^32"),
                    ops(Q, whole(v["P"], (1, 3)), Q, whole(v["power"], (1, 3)), whole(v["temp"], (1, 3))) + upper))
    v = geometry_views("G3")  # the source rectangle begins at byte 2^32 of a row: its west neighbour lies across the mark
    # (the destination at byte 2^31 + 16: 16-byte units, and 3001 columns leave a tail)
    Q = g3(v["Q"], P29 + 4, 3001)
    out.append(Case("stencil-G3", "stencil", "G3", ("2^31", "2^32"), ops(Q, g3(v["P"], P30, 3001), Q)))
    v = geometry_views("G5")
    n = P29 - 1
    out.append(Case("stencil-G5", "stencil", "G5", ("row",), (
        Op("BOX9 (dense)", "stencil", Rect(v["Q"], 0, 0, 2, n), (Rect(v["P"], 0, 0, 2, n),),
           {"shape": BOX9, "weights": BOX, "halo": HALO}),), extra=10 * GiB))
    return out


def reduction_cases():
    out = []
    v = geometry_views("G1")
    P, Q, temp, power = whole(v["P"]), whole(v["Q"]), whole(v["temp"]), whole(v["power"])
    out.append(Case("reductions-G1", "reductions", "G1", ("2^31", "2^32"), (
        Op("norms of a plane and two members in one call", "norms", None, (P, temp, power)),
        Op("distance of two planes and of two members", "distance", None, (P, Q, temp, power)),
        Op("dot of two planes", "dot", None, (P, Q)),
        Op("dot of two members", "dot", None, (temp, power)),
        Op("dot of a plane and a member", "dot", None, (Q, temp)),
        Op("max_abs of a plane", "max_abs", None, (P,)),
        Op("max_abs of a member", "max_abs", None, (power,)),
    )))
    v = geometry_views("G2")
    P, temp, power, hz = whole(v["P"]), whole(v["temp"]), whole(v["power"]), whole(v["hz"])
    out.append(Case("reductions-G2", "reductions", "G2", ("2^31", "2^32"), (
        Op("norms of a plane and members of two kinds of cells", "norms", None, (P, power, hz)),
        Op("distance of two members", "distance", None, (temp, power)),
        Op("dot of two members", "dot", None, (temp, hz)),
        Op("dot of a plane and a member", "dot", None, (P, hz)),
        Op("max_abs of a plane", "max_abs", None, (P,)),
        Op("max_abs of a member", "max_abs", None, (hz,)),
    )))
    g1, g2 = geometry_views("G1"), geometry_views("G2")
    out.append(Case("dot-G1xG2", "reductions", "G1xG2", ("2^31", "2^32"), (
        Op("a plane in G1 against a member in G2", "dot", None, (Rect(g1["P"], 0, 5, 3, 8200), whole(g2["hz"]))),
        Op("the member against the plane", "dot", None, (whole(g2["hz"]), Rect(g1["P"], 1, 5, 3, 8200))),
    )))
    v = geometry_views("G3")
    out.append(Case("reductions-G3", "reductions", "G3", ("2^31", "2^32"), (
        Op("norms at byte 2^31 + 4 and at byte 2^32 + 28", "norms", None, (g3(v["P"], FAR_A), g3(v["Q"], FAR_B))),
        Op("distance", "distance", None, (g3(v["P"], FAR_B), g3(v["Q"], FAR_B))),
        Op("dot of two far rectangles", "dot", None, (g3(v["P"], FAR_A), g3(v["Q"], FAR_B))),
        Op("max_abs", "max_abs", None, (g3(v["P"], FAR_B),)),
    )))
    v = geometry_views("G5")
    n = P29 - 1
    P, Q = Rect(v["P"], 0, 0, 2, n), Rect(v["Q"], 0, 0, 2, n)
    out.append(Case("reductions-G5", "reductions", "G5", ("row",), (
        Op("norms of a plane", "norms", None, (P,)),
        Op("dot of two planes", "dot", None, (P, Q)),
    ), extra=14 * GiB))
    return out


# G4: rows of more segments than a launch has workgroups; small enough for the families' own random-float models
G4_DENSE = 2049 * 4096 + 5
G4_STRIDED = 2049 * 1024 + 5
G4 = {  # id -> (family, layout, columns)
    "regions-G4-dense": ("regions", "dense", G4_DENSE), "regions-G4-strided": ("regions", "strided", G4_STRIDED),
    "algebra-G4-dense": ("algebra", "dense", G4_DENSE), "algebra-G4-strided": ("algebra", "strided", G4_STRIDED),
    "stencil-G4-dense": ("stencil", "dense", G4_DENSE), "stencil-G4-strided": ("stencil", "strided", G4_STRIDED),
    "norms-G4-dense": ("norms", "dense", G4_DENSE), "norms-G4-strided": ("norms", "strided", G4_STRIDED),
    "dot-G4-dense": ("dot", "dense", G4_DENSE), "dot-G4-strided": ("dot", "strided", G4_STRIDED),
}
G4_NEED = 2 * GiB  # a handful of buffers of 3 x (G4_DENSE + 3) floats, 101 MB each


def g4_segments(case_id):
    """(segments of a row, cap of workgroups) of a G4 case."""
    family, layout, n_cols = G4[case_id]
    segment, cap = segments_of(family)[layout]
    return -(-n_cols // segment), cap


# scatter / gather: an AoS buffer that ends behind 4 GiB
AOS_CELLS, AOS_CELL_BYTES, AOS_FIELDS = (1 << 27) + 3, 32, 8
AOS_NEED = FRONT_GUARD + AOS_CELLS * AOS_CELL_BYTES + AOS_FIELDS * (AOS_CELLS * 4 + 2 * BACK_GUARD) + 3 * GiB

# one sweep launch: rows 2^28 + 44 bytes apart, or the next multiple of the cell's size
SWEEP_ROW_DISTANCE = (1 << 28) + 44
SWEEP_ROWS = 20
SWEEP_APPS = {  # registered name -> columns in the function's own cells
    "jacobi5general": 701, "jacobi5uniform_only": 701, "hotspot": 701, "hotspot_aos": 701, "fdtd_coef_aos": 701,
    "conway": 701, "conway_packed": 700 // 4,
}


def sweep_pitch(elem_size):
    """Elements between two rows: SWEEP_ROW_DISTANCE bytes, rounded up to whole elements."""
    return -(-SWEEP_ROW_DISTANCE // elem_size)


def sweep_need(plane_sizes):
    """Source and destination planes of a sweep case: one row more than the grid's, so that whole rows follow the last."""
    return 2 * sum(arena_bytes(plane("x", 0, sweep_pitch(s), SWEEP_ROWS + 1, 701, s)) for s in plane_sizes) + (16 << 20)


def f64_cases():
    """The f64 twin of G1 (rows 2^31 + 24 bytes apart) for the families besides the algebra."""
    v = geometry_views("G1f64")
    P, Q = whole(v["P"]), whole(v["Q"])
    lower, source = whole(v["Q"], (1, 4)), whole(v["P"], (1, 4))
    return [
        Case("regions-G1-f64", "regions", "G1", ("2^31", "2^32"), (
            Op("plane to plane (dense)", "copy", Q, (P,)),
            Op("every second source row and column (strided)", "copy", whole(v["Q"], (2, 4), (5, 4105)),
               (Rect(v["P"], 1, 5, 2, 4100, row_step=2, col_step=2),)),
            Op("fill", "fill", Q, (), {"value": -77.0}),
        )),
        Case("stencil-G1-f64", "stencil", "G1", ("2^31", "2^32"), (
            Op("BOX9 (dense)", "stencil", lower, (source,), {"shape": BOX9, "weights": BOX, "halo": HALO}),
            Op("BOX9 with the destination as right-hand side (general)", "stencil", lower, (source, lower),
               {"shape": BOX9, "weights": BOX, "halo": HALO, "rhs_coef": 0.25, "general": True}),
            Op("CROSS5", "stencil", lower, (source,), {"shape": CROSS5, "weights": CROSS, "halo": HALO}),
        )),
        Case("reductions-G1-f64", "reductions", "G1", ("2^31", "2^32"), (
            Op("norms of two planes in one call", "norms", None, (P, Q)),
            Op("distance of two planes", "distance", None, (P, Q)),
            Op("dot of two planes", "dot", None, (P, Q)),
        )),
    ]


CASES = region_cases() + algebra_cases() + stencil_cases() + reduction_cases() + f64_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def ids(family):
    return [c.id for c in CASES if c.family == family]


# ------------------------------------------------------------------------------------------ buffers on the device
def require(need):
    """Skip unless need + HEADROOM bytes are free (a condition, not an escape: an MI355X has 288 GB)."""
    import pytest
    import torch

    assert need <= MAX_NEED, f"a test may need {MAX_NEED} bytes at the most, not {need}"
    free, _ = torch.cuda.mem_get_info()
    if free < need + HEADROOM:
        pytest.skip(f"needs {need} bytes of device memory (+ {HEADROOM} headroom), {free} are free")
    torch.cuda.reset_peak_memory_stats()


def release(what=""):
    """Give everything back: torch's cache and the library's pool.  Prints the peak the test reached."""
    import torch

    from stencilstream_amd import capi

    torch.cuda.synchronize()
    print(f"\n[large extents] {what}: peak {torch.cuda.max_memory_allocated()} bytes")
    torch.cuda.empty_cache()
    capi.load().ststhip_pool_trim()


class Arena:
    """The cells of one buffer behind FRONT_GUARD bytes, all of it the sentinel."""

    CHUNK = 1 << 28  # words per reduction when the whole buffer is checked

    def __init__(self, device, view, sentinel=None):
        import torch

        self.view = view
        self.nbytes = arena_bytes(view)
        self.raw = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        if sentinel is None:
            sentinel = SENTINEL_F64 if view.elem == 8 else SENTINEL_F32
        self.sentinel = sentinel
        self.words = self.raw.view(torch.int64 if sentinel == SENTINEL_F64 else torch.int32)
        self.words.fill_(sentinel)
        self.base = self.raw.data_ptr() + FRONT_GUARD
        assert self.base % 16 == 0

    def capi_view(self, view):
        from stencilstream_amd import capi

        assert view.buf == self.view.buf and view.stride == self.view.stride and view.pitch == self.view.pitch
        return capi.grid_view(self.base + view.offset, view.stride, view.height, view.width, view.pitch)

    def _strided(self, rect, typed):
        import torch

        v, size = rect.view, typed.element_size()
        assert v.elem % size == 0 and v.stride % size == 0 and v.offset % size == 0 and rect.last_byte() < v.extent()
        per = v.elem // size  # (the 0xA5 words of byte cells: never more than one per element here)
        assert per == 1
        return torch.as_strided(typed, (rect.n_rows, rect.n_cols),
                                (rect.row_distance() // size, rect.col_step * v.stride // size),
                                (FRONT_GUARD + rect.first()) // size)

    def cells(self, rect):
        """The rectangle as a strided torch view of floats."""
        import torch

        return self._strided(rect, self.raw.view(torch.float64 if rect.view.elem == 8 else torch.float32))

    def put_coded(self, rect):
        """Coded values into the rectangle, in slices of 2^25 columns."""
        import torch

        target, v = self.cells(rect), rect.view
        rows = torch.tensor(rect.rows(), dtype=torch.int64, device=self.raw.device)[:, None]
        for begin in range(0, rect.n_cols, 1 << 25):
            end = min(begin + (1 << 25), rect.n_cols)
            cols = (rect.col + rect.col_step * torch.arange(begin, end, dtype=torch.int64, device=self.raw.device))[None, :]
            target[:, begin:end] = code_of(v.k, rows, cols).to(target.dtype)

    def clear(self, rect):
        self._strided(rect, self.words).fill_(self.sentinel)

    def assert_clean(self, what):
        """Every word of the buffer, guards included, is the sentinel."""
        import torch

        lows, highs = [], []
        for begin in range(0, self.words.numel(), self.CHUNK):
            low, high = torch.aminmax(self.words[begin:begin + self.CHUNK])
            lows.append(low)
            highs.append(high)
        low, high = int(torch.stack(lows).min()), int(torch.stack(highs).max())
        if low == self.sentinel and high == self.sentinel:
            return
        for begin in range(0, self.words.numel(), self.CHUNK):
            wrong = torch.nonzero(self.words[begin:begin + self.CHUNK] != self.sentinel)
            if wrong.numel():
                byte = (begin + int(wrong[0])) * self.words.element_size() - FRONT_GUARD
                raise AssertionError(f"{what}: buffer {self.view.buf} changed outside the rectangles: {wrong.numel()} words "
                                     f"of one gigabyte, the first at byte {byte} from the cells' base "
                                     f"({'the front guard' if byte < 0 else f'row {byte // self.view.row_bytes}'})")

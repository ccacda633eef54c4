"""The grid extensions (regions, algebra, stencil, norms / distance, dot), ststhip_reduce_max_abs and
ststhip_scatter_fields / _gather_fields behind byte offsets of 2^31 and 2^32 and more, on rows of more segments than a
launch has workgroups and on the longest row ststhip.h admits; and one sweep launch on rows 2^28 + 44 bytes apart.

The cases, their buffers and their data are tests/large_extents.py (read its docstring first): views with a huge pitch,
coded small integers, a front guard of 2^31 + 4096 bytes, a sentinel everywhere else.  What is compared:

  * G1 (rows 2^31 + 12 bytes apart), G2 (2^32 + 16), G3 (rectangles 2^31 + 4 and 2^32 + 28 bytes into rows of 6 GiB): the
    result rectangle, copied out, against the operation's formula in float64 numpy on the coded values -- every product
    and sum is exact, the float64 result is representable in the element's type (asserted) and the bits must be equal.
    Sums, sums of squares and dot products are integers below 2^53: the doubles are compared as bits, counts as integers.
  * G5 (rows of 2^31 - 4 bytes, 2^30 - 2 cells): the same formulas with torch's element-wise kernels on the device, one
    torch.mul and one torch.add per operation; sums in float64 (integers: exact in any order).
  * G4 (2049 segments of a row): the families' own random-float models (tests/test_grid_*_gpu.py), so that the rounding
    order is exercised at that shape too.  The segment sizes and the cap of 2048 workgroups are read from the .hip files
    and `width > cap * segment` is asserted.

After every call the sentinel is put back over the rectangles and every buffer, guards included, must be all sentinel:
nothing outside the rectangle was written, no source changed.

Every test states its need in bytes, skips (with that number) unless need + 4 GiB are free -- never on an MI355X -- and
gives its buffers back before it returns.  FDTD on eight planes at these row distances would need about 80 GiB (sixteen
planes of 5 GiB): it is left out on purpose; FDTD runs as AoS cells."""
import os

import numpy as np
import pytest
import torch

import large_extents as LE
from large_extents import BY_ID, Arena

pytestmark = pytest.mark.gpu

BIG = 1 << 24  # cells of a rectangle from which on the reference is computed on the device
DTYPE = {4: (np.dtype("<f4"), torch.float32, torch.int32), 8: (np.dtype("<f8"), torch.float64, torch.int64)}


# ------------------------------------------------------------------------------------------ coded values and formulas
def coded(rect):
    """The coded values of a rectangle's cells, float64 on the host."""
    rows = np.array(rect.rows(), dtype=np.int64)[:, None]
    cols = (rect.col + rect.col_step * np.arange(rect.n_cols, dtype=np.int64))[None, :]
    return LE.code_of(rect.view.k, rows, cols).astype(np.float64)


def combine_formula(coefs, xs):
    acc = xs[0] * coefs[0]
    for coef, x in zip(coefs[1:], xs[1:]):
        acc = acc + x * coef
    return acc


def restrict_formula(s):
    return ((s[0::2, 0::2] + s[0::2, 1::2]) + (s[1::2, 0::2] + s[1::2, 1::2])) * 0.25


def window(rect):
    """The part of the view a stencil or a prolongation of `rect` reads, as the models of the families' own tests take
    a view: where the window ends the view ends, so the models' halo is the view's.  Returns (values, rect's place)."""
    w = rect.widened()
    return coded(w), (rect.row - w.row, rect.col - w.col)


def expected(op):
    from test_grid_algebra_gpu import prolong_model
    from test_grid_stencil_gpu import stencil_model

    f8 = np.dtype("<f8")
    if op.kind in ("copy", "upload", "download"):
        return coded(op.srcs[0])
    if op.kind == "fill":
        return np.full((op.dst.n_rows, op.dst.n_cols), op.par["value"])
    if op.kind == "combine":
        return combine_formula(op.par["coefs"], [coded(s) for s in op.srcs])
    if op.kind == "restrict":
        return restrict_formula(coded(op.srcs[0]))
    if op.kind == "prolong":
        view, at = window(op.srcs[0])
        return prolong_model(f8, view, at, op.srcs[0].n_rows, op.srcs[0].n_cols, op.par["halo"])
    if op.kind == "stencil":
        view, at = window(op.srcs[0])
        rhs = coded(op.srcs[1]) if len(op.srcs) > 1 else None
        return stencil_model(f8, op.par["shape"], list(op.par["weights"]), view, at, op.dst.n_rows, op.dst.n_cols,
                             op.par["halo"], rhs, op.par.get("rhs_coef", 1.0))
    raise KeyError(op.kind)


def same_bits(got, want64, elem, what):
    """`got` (a device tensor copied out) holds the float64 values `want64`, which the element's type represents."""
    np_type = DTYPE[elem][0]
    want = want64.astype(np_type)
    assert np.array_equal(want.astype(np.float64), want64), f"{what}: the expected values are not exact in the element's type"
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    int_type = "<u4" if elem == 4 else "<u8"
    if not np.array_equal(got.view(int_type), want.view(int_type)):
        bad = np.argwhere(got.view(int_type) != want.view(int_type))
        r, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} cells differ in rows {sorted(set(bad[:, 0].tolist()))} of the "
                             f"rectangle, the first at ({r}, {c}): got {got[r, c]!r}, expected {want[r, c]!r}")


# ------------------------------------------------------------------------------------------ running a case
class Bench:
    """The arenas of a case."""

    def __init__(self, device, case):
        LE.require(case.need())
        self.case, self.device = case, device
        self.arenas = {name: Arena(device, view) for name, view in case.views().items()}
        torch.cuda.synchronize()

    def of(self, rect):
        return self.arenas[rect.view.buf]

    def view(self, rect):
        return self.of(rect).capi_view(rect.view)

    def settle(self, patches, what):
        for p in patches:
            self.of(p).clear(p)
        for arena in self.arenas.values():
            arena.assert_clean(what)

    def close(self):
        self.arenas.clear()


def patches_of(op):
    """What an operation reads, on the device: its sources, the first one widened where neighbours are read."""
    out = []
    for i, s in enumerate(op.srcs):
        if s.view.buf is None:
            continue
        out.append(s.widened() if i == 0 and op.kind in ("stencil", "prolong") else s)
    return out


def pinned(rect, fill):
    """Host memory for the host side of a download or an upload: rows of n_cols + 3 floats, `fill` everywhere."""
    return torch.full((rect.n_rows, rect.view.pitch), fill, dtype=torch.float32).pin_memory()


def call_of(bench, op, host=None):
    """The library call of an operation, as a function without arguments."""
    from stencilstream_amd import capi

    dtype = None if op.dst is None else DTYPE[op.dst.view.elem][0].str
    if op.kind in ("copy", "download", "upload"):
        src, dst = op.srcs[0], op.dst
        sv = capi.grid_view(host.data_ptr(), 4, src.n_rows, src.n_cols, src.view.pitch) if op.kind == "upload" else bench.view(src)
        dv = capi.grid_view(host.data_ptr(), 4, dst.n_rows, dst.n_cols, dst.view.pitch) if op.kind == "download" else bench.view(dst)
        desc = capi.grid_copy_desc(dv, sv, src.view.elem, dst.n_rows, dst.n_cols, (dst.row, dst.col), (src.row, src.col),
                                   (src.row_step, src.col_step))
        return lambda: getattr(capi, "grid_" + op.kind)([desc])
    if op.kind == "fill":
        value = np.array([op.par["value"]], dtype=DTYPE[op.dst.view.elem][0]).tobytes()
        desc = capi.grid_fill_desc(bench.view(op.dst), value, op.dst.n_rows, op.dst.n_cols, (op.dst.row, op.dst.col))
        return lambda: capi.grid_fill([desc])
    if op.kind == "combine":
        terms = [(coef, bench.view(s), (s.row, s.col)) for coef, s in zip(op.par["coefs"], op.srcs)]
        desc = capi.grid_combine_desc(bench.view(op.dst), dtype, terms, op.dst.n_rows, op.dst.n_cols, (op.dst.row, op.dst.col))
        return lambda: capi.grid_combine([desc])
    if op.kind in ("restrict", "prolong"):
        src, dst = op.srcs[0], op.dst
        coarse = dst if op.kind == "restrict" else src
        desc = capi.grid_resample_desc(bench.view(dst), bench.view(src), dtype,
                                       capi.RESTRICT_MEAN if op.kind == "restrict" else capi.PROLONG_BILINEAR,
                                       coarse.n_rows, coarse.n_cols, (dst.row, dst.col), (src.row, src.col),
                                       op.par.get("halo", 0.0))
        return lambda: capi.grid_resample([desc])
    if op.kind == "stencil":
        src, dst = op.srcs[0], op.dst
        rhs = op.srcs[1] if len(op.srcs) > 1 else None
        desc = capi.grid_stencil_desc(bench.view(dst), bench.view(src), dtype, op.par["shape"], list(op.par["weights"]),
                                      dst.n_rows, dst.n_cols, (dst.row, dst.col), (src.row, src.col), op.par["halo"],
                                      None if rhs is None else bench.view(rhs), op.par.get("rhs_coef", 1.0),
                                      (0, 0) if rhs is None else (rhs.row, rhs.col))

        def call():
            # (read at every call: planes take the general kernel too)
            if op.par.get("general"):
                os.environ["STSTHIP_STENCIL_GENERAL"] = "1"
            try:
                capi.grid_stencil([desc])
            finally:
                os.environ.pop("STSTHIP_STENCIL_GENERAL", None)
        return call
    raise KeyError(op.kind)


def run_small(bench, op):
    """An operation on rectangles of a few thousand cells per row: the reference on the host."""
    what = f"{bench.case.id}: {op.name}"
    patches = patches_of(op)
    for p in patches:
        bench.of(p).put_coded(p)
    host = None
    if op.kind == "upload":
        host = pinned(op.srcs[0], float("nan"))
        host[:, :op.srcs[0].n_cols] = torch.from_numpy(coded(op.srcs[0]).astype("<f4"))
    if op.kind == "download":
        host = pinned(op.dst, float("nan"))
    call = call_of(bench, op, host)
    torch.cuda.synchronize()
    call()
    torch.cuda.synchronize()
    if op.kind == "download":
        got = host[:, :op.dst.n_cols].clone()
        assert bool(torch.isnan(host[:, op.dst.n_cols:]).all()), f"{what}: the host rows' padding was written"
    else:
        got = bench.of(op.dst).cells(op.dst).clone()
    for p in patches:  # a source that is not the destination holds what it held
        if p != op.dst:
            same_bits(bench.of(p).cells(p).clone(), coded(p), p.view.elem, f"{what}: a source")
    bench.settle(patches + ([] if op.kind == "download" else [op.dst]), what)
    same_bits(got, expected(op), 4 if op.kind == "download" else op.dst.view.elem, what)


def equal_on_device(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    ints = torch.int32 if got.element_size() == 4 else torch.int64
    if not torch.equal(got.view(ints), want.view(ints)):
        bad = torch.nonzero(got.view(ints) != want.view(ints))
        r, c = (int(x) for x in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} cells differ, the first at ({r}, {c}): got {float(got[r, c])!r}, "
                             f"expected {float(want[r, c])!r}")


def shifted(src, a, b, halo):
    """src(i + a, j + b) over a whole view on the device, `halo` outside."""
    n_rows, n_cols = src.shape
    out = torch.full((n_rows, n_cols), halo, dtype=src.dtype, device=src.device)
    r0, r1, c0, c1 = max(0, -a), min(n_rows, n_rows - a), max(0, -b), min(n_cols, n_cols - b)
    if r0 < r1 and c0 < c1:
        out[r0:r1, c0:c1] = src[r0 + a:r1 + a, c0 + b:c1 + b]
    return out


def expected_on_device(bench, op):
    """G5: the formula with torch's element-wise kernels, one torch.mul and one torch.add per operation.  The rectangles
    are whole views."""
    xs = [bench.of(s).cells(s) for s in op.srcs]
    if op.kind == "copy":
        return xs[0]
    if op.kind == "fill":
        return torch.full((op.dst.n_rows, op.dst.n_cols), op.par["value"], dtype=torch.float32, device=bench.device)
    if op.kind == "combine":
        acc = torch.mul(xs[0], op.par["coefs"][0])
        for coef, x in zip(op.par["coefs"][1:], xs[1:]):
            term = torch.mul(x, coef)
            torch.add(acc, term, out=acc)
            del term
        return acc
    if op.kind == "restrict":
        s = xs[0]
        top = torch.add(s[0::2, 0::2], s[0::2, 1::2])
        bottom = torch.add(s[1::2, 0::2], s[1::2, 1::2])
        torch.add(top, bottom, out=top)
        del bottom
        return torch.mul(top, 0.25, out=top)
    if op.kind == "prolong":
        s, halo = xs[0], op.par["halo"]
        assert op.srcs[0].widened() == op.srcs[0]  # the whole view: the halo on every side
        out = torch.empty((2 * s.shape[0], 2 * s.shape[1]), dtype=s.dtype, device=s.device)
        for b, j_far in ((0, -1), (1, +1)):
            h = {}
            for i in (-1, 0, +1):
                h[i] = torch.mul(shifted(s, i, 0, halo), 0.75)
                far = torch.mul(shifted(s, i, j_far, halo), 0.25)
                torch.add(h[i], far, out=h[i])
                del far
            for a, i_far in ((0, -1), (1, +1)):
                v = torch.mul(h[0], 0.75)
                far = torch.mul(h[i_far], 0.25)
                out[a::2, b::2] = torch.add(v, far, out=v)
                del v, far
        return out
    if op.kind == "stencil":
        from test_grid_stencil_gpu import TAPS

        s = xs[0]
        assert op.srcs[0].widened() == op.srcs[0] and len(xs) == 1
        acc = None
        for a, b in TAPS[op.par["shape"]]:
            term = shifted(s, a, b, op.par["halo"])
            torch.mul(term, op.par["weights"][3 * (a + 1) + (b + 1)], out=term)
            acc = term if acc is None else torch.add(acc, term, out=acc)
            del term
        return acc
    raise KeyError(op.kind)


def run_big(bench, op):
    """An operation on whole rows of 2^31 - 4 bytes: the reference on the device, the result compared in place."""
    what = f"{bench.case.id}: {op.name}"
    patches = patches_of(op)
    for p in patches:
        bench.of(p).put_coded(p)
    want = expected_on_device(bench, op)
    call = call_of(bench, op)
    torch.cuda.synchronize()
    call()
    torch.cuda.synchronize()
    equal_on_device(bench.of(op.dst).cells(op.dst), want, what)
    del want
    bench.settle(patches + [op.dst], what)


def run_case(gpu, case_id, run_op=None):
    case = BY_ID[case_id]
    bench = Bench(gpu, case)
    try:
        for op in case.ops:
            cells = max(r.n_rows * r.n_cols for r in op.rects())
            (run_op or (run_big if cells > BIG else run_small))(bench, op)
    finally:
        bench.close()
        del bench
        LE.release(f"{case_id}, need {case.need()}")


@pytest.mark.parametrize("case_id", LE.ids("regions"))
def test_regions(gpu, case_id):
    """Copies plane to plane (the dense kernel), member to plane and plane to member (the strided kernels), one with
    src_row_step = 2 and one with src_col_step = 2, fills, downloads to and uploads from a small pinned host array; on G5
    a dense copy and a fill of two rows of 2^31 - 4 bytes."""
    run_case(gpu, case_id)


@pytest.mark.parametrize("case_id", LE.ids("algebra"))
def test_algebra(gpu, case_id):
    """Combines of two terms on planes, on members and in place; restrict_mean and prolong_bilinear with the fine side in
    G1 and G2 (halo 1000.5, which no cell holds: at the top and on the left of the coarse rectangle, cells of the view at
    the bottom and on the right); on G5 a combine of two terms over 2^30 - 2 cells and both transfers with 2^28 - 1
    coarse columns."""
    run_case(gpu, case_id)


@pytest.mark.parametrize("case_id", LE.ids("stencil"))
def test_stencil(gpu, case_id):
    """BOX9 on planes with and without a right-hand side (the destination itself) through the dense kernel -- in G2 in
    16-byte units with a head of three elements, in G1 in units of one element -- and through the general kernel
    (STSTHIP_STENCIL_GENERAL), CROSS5 on planes, BOX9 and CROSS5 from one member of HotSpot cells to the other.  The
    views have neighbours on all four sides but where a view of three or four rows ends (rows 1 .. and rows 0 .. run
    both); in G3 the west neighbour of the first column lies across the 2^32 byte mark.  On G5 BOX9 dense."""
    run_case(gpu, case_id)


# ------------------------------------------------------------------------------------------ reductions
def as_bits(value):
    return np.float64(value).tobytes()


def exact_norms(v):
    """v: integers as float64."""
    return {"n_cells": v.size, "n_nonfinite": 0, "max_abs": float(np.abs(v).max()), "sum": float(v.sum()),
            "sum_abs": float(np.abs(v).sum()), "sum_sq": float((v * v).sum())}


def assert_norms(got, want, what):
    print(f"{what}: got {got.as_dict()}, expected {want}")
    assert (got.n_cells, got.n_nonfinite) == (want["n_cells"], want["n_nonfinite"]), what
    for name in ("max_abs", "sum", "sum_abs", "sum_sq"):
        assert as_bits(getattr(got, name)) == as_bits(want[name]), (what, name, getattr(got, name), want[name])


def assert_dot(got, want, what):
    print(f"{what}: got n_cells {got.n_cells}, n_nonfinite {got.n_nonfinite}, dot {got.dot!r}, sum_aa {got.sum_aa!r}, "
          f"sum_bb {got.sum_bb!r}; expected {want}")
    assert (got.n_cells, got.n_nonfinite) == (want["n_cells"], 0), what
    for name in ("dot", "sum_aa", "sum_bb"):
        assert as_bits(getattr(got, name)) == as_bits(want[name]), (what, name, getattr(got, name), want[name])


def norm_field(bench, r):
    from stencilstream_amd import capi

    v = r.view
    return capi.norm_field(bench.of(r).base + v.offset, DTYPE[v.elem][0].str, v.stride, v.height, v.width, v.pitch,
                           (r.row, r.row + r.n_rows), (r.col, r.col + r.n_cols))


def values_of(bench, r, big):
    """The rectangle's values: float64 on the host, or the float32 cells on the device."""
    return bench.of(r).cells(r) if big else coded(r)


def sums(x, big):
    """Integers: exact in double in any order."""
    if big:
        return {"n_cells": x.numel(), "n_nonfinite": 0, "max_abs": float(x.abs().max()), "sum": float(x.sum(dtype=torch.float64)),
                "sum_abs": float(x.abs().sum(dtype=torch.float64)), "sum_sq": float(torch.mul(x, x).sum(dtype=torch.float64))}
    return exact_norms(x)


def product_sum(x, y, big):
    return float(torch.mul(x, y).sum(dtype=torch.float64)) if big else float((x * y).sum())


def run_reduction(bench, op):
    from stencilstream_amd import capi

    what = f"{bench.case.id}: {op.name}"
    big = max(r.n_rows * r.n_cols for r in op.srcs) > BIG
    for s in op.srcs:
        bench.of(s).put_coded(s)
    torch.cuda.synchronize()
    if op.kind == "norms":
        got = capi.grid_norms([norm_field(bench, s) for s in op.srcs])
        for i, s in enumerate(op.srcs):
            assert_norms(got[i], sums(values_of(bench, s, big), big), f"{what}, field {i}")
    elif op.kind == "distance":
        pairs = list(zip(op.srcs[0::2], op.srcs[1::2]))
        for a, b in pairs:  # the second grid has the layout of the first
            assert (a.view.stride, a.view.pitch, a.row, a.col) == (b.view.stride, b.view.pitch, b.row, b.col)
        got = capi.grid_norms([norm_field(bench, a) for a, _ in pairs], [bench.of(b).base + b.view.offset for _, b in pairs])
        for i, (a, b) in enumerate(pairs):
            assert_norms(got[i], exact_norms(coded(a) - coded(b)), f"{what}, pair {i}")
    elif op.kind == "dot":
        a, b = op.srcs
        desc = capi.grid_dot_desc(bench.view(a), bench.view(b), DTYPE[a.view.elem][0].str, a.n_rows, a.n_cols, (a.row, a.col),
                                  (b.row, b.col))
        got = capi.grid_dot([desc])[0]
        x, y = values_of(bench, a, big), values_of(bench, b, big)
        assert_dot(got, {"n_cells": a.n_rows * a.n_cols, "dot": product_sum(x, y, big), "sum_aa": product_sum(x, x, big),
                         "sum_bb": product_sum(y, y, big)}, what)
    elif op.kind == "max_abs":
        # NaNs do not count in a maximum, so a row read from the wrong place would go unseen: row i gets a peak of
        # 1000 + i in its column n_cols - 1 - i, and the rows up to i must have the maximum 1000 + i
        (s,) = op.srcs
        v, cells = s.view, bench.of(s).cells(s)
        for i in range(s.n_rows):
            cells[i, s.n_cols - 1 - i] = 1000.0 + i
        torch.cuda.synchronize()
        first = bench.of(s).base + (s.row * v.pitch + s.col) * v.stride
        for i in range(s.n_rows):
            got = capi.reduce_max_abs(first, v.stride, s.n_rows, s.n_cols, [(v.offset, "f4", i + 1, s.n_cols)], pitch=v.pitch)
            assert got == [1000.0 + i], (what, i, got)
        got = capi.reduce_max_abs(first, v.stride, s.n_rows, s.n_cols, [(v.offset, "f4", s.n_rows, s.n_cols - s.n_rows)],
                                  pitch=v.pitch)
        assert got == [float(np.abs(coded(s)[:, :s.n_cols - s.n_rows]).max())], (what, got)
    else:
        raise KeyError(op.kind)
    bench.settle(list(op.srcs), what)


@pytest.mark.parametrize("case_id", LE.ids("reductions"))
def test_reductions(gpu, case_id):
    """ststhip_grid_norms, _distance and _dot of planes and of members, and ststhip_reduce_max_abs: everything outside the
    rectangles is NaN, so a stray read shows in n_nonfinite (which must be 0) and in the sums.  The two sides of one dot
    lie in different geometries: a plane in G1 against a member of FDTD cells in G2.  On G5 n_cells is 2^30 - 2."""
    if case_id == "reductions-G5":
        assert LE.G5_CELLS == (1 << 30) - 2
    run_case(gpu, case_id, run_reduction)


# ------------------------------------------------------------------------------------------ G4: more segments than workgroups
@pytest.mark.parametrize("case_id", sorted(LE.G4))
def test_more_segments_than_workgroups(gpu, case_id, monkeypatch):
    """Three rows of 2049 * 4096 + 5 floats (dense) or of 2049 * 1024 + 5 HotSpot cells (strided), pitch = width + 3: a
    row has more segments than the cap of 2048 workgroups, so plan_blocks puts one workgroup on every segment
    (gridDim.x > cap) and every workgroup walks down all three rows.  The segment sizes and the cap come from the .hip
    files; the models are the families' own (random floats, numpy in the element's type, whole buffers compared)."""
    family, layout, W = LE.G4[case_id]
    segment, cap = LE.segments_of(family)[layout]
    assert W > cap * segment and LE.g4_segments(case_id)[0] > cap
    LE.require(LE.G4_NEED)
    from stencilstream_amd import capi
    from stencilstream_amd import update as U

    F32 = np.dtype("<f4")
    try:
        if family == "regions":
            from test_grid_regions_gpu import Buffer, copy

            if layout == "dense":
                src, dst = Buffer(gpu, 3, W + 3, 4, seed=41, width=W), Buffer(gpu, 3, W + 3, 4, seed=42, width=W)
                capi.grid_copy([copy(dst, src, 4, 3, W - 1, dst_at=(0, 1))])
                dst.check("plane to plane")
                dst.bytes()[:, 2:W, :] = np.frombuffer(np.float32(-77.0).tobytes(), dtype=np.uint8)
                capi.grid_fill([capi.grid_fill_desc(dst.view(), np.float32(-77.0).tobytes(), 3, W - 2, dst_at=(0, 2))])
                dst.check("fill")
                back = np.zeros((3, W), dtype="<f4")
                capi.grid_download([capi.grid_copy_desc(capi.grid_view(back.ctypes.data, 4, 3, W), src.view(), 4, 3, W)])
                assert np.array_equal(back.view(np.uint8).reshape(3, W, 4), src.bytes()[:, :W, :])
                capi.grid_upload([capi.grid_copy_desc(dst.view(), capi.grid_view(back.ctypes.data, 4, 3, W), 4, 3, W)])
                dst.bytes()[:, :W, :] = src.bytes()[:, :W, :]
                dst.check("upload")
                src.check("the source")
            else:
                cells, flat = Buffer(gpu, 3, W + 3, 8, seed=43, width=W), Buffer(gpu, 3, W + 3, 4, seed=44, width=W)
                capi.grid_copy([copy(flat, cells, 4, 3, W, src_offset=4)])
                flat.check("member to plane")
                capi.grid_copy([copy(cells, flat, 4, 3, W - 1, dst_at=(0, 1), dst_offset=0)])
                cells.check("plane to member")
                cells.bytes()[:, :W, 4:8] = np.frombuffer(np.float32(-77.0).tobytes(), dtype=np.uint8)
                capi.grid_fill([capi.grid_fill_desc(cells.view(4), np.float32(-77.0).tobytes(), 3, W)])
                cells.check("fill of a member")
                flat.check("the plane")
        elif family == "algebra":
            from test_grid_algebra_gpu import PROLONG, RESTRICT, cell_buffer, plane, run_combine, run_resample

            if layout == "dense":
                dst, a = plane(gpu, F32, 3, W + 3, 51, width=W), plane(gpu, F32, 3, W + 3, 52, width=W)
                run_combine(dst, 0, F32, [(0.5, a, 0, (0, 0)), (-2.0, a, 0, (0, 1))], 3, W - 1, what="two terms of one plane")
                run_combine(dst, 0, F32, [(0.3, dst, 0, (0, 1)), (0.1, a, 0, (0, 0))], 3, W - 1, dst_at=(0, 1), what="in place")
                a.unchanged("the source")
            else:
                cells, flat = cell_buffer(gpu, "hotspot", 3, W + 3, 53, width=W), plane(gpu, F32, 3, W + 3, 54, width=W)
                run_combine(cells, 4, F32, [(0.5, cells, 0, (0, 0)), (-2.0, flat, 0, (0, 0))], 3, W, what="a member and a plane")
                run_combine(cells, 0, F32, [(0.3, cells, 0, (0, 0)), (0.1, flat, 0, (0, 0))], 3, W, what="in place on a member")
                flat.unchanged("the plane")
                # the transfers count coarse columns: W coarse cells of one row, two fine rows of 2 W
                coarse, fine = plane(gpu, F32, 2, W + 3, 55, width=W), plane(gpu, F32, 2, 2 * W + 3, 56, width=2 * W)
                run_resample(RESTRICT, coarse, 0, fine, 0, F32, 1, W, what="restrict")
                run_resample(PROLONG, fine, 0, coarse, 0, F32, 1, W, halo=0.7, what="prolong")
        elif family == "stencil":
            from test_grid_algebra_gpu import cell_buffer, plane
            from test_grid_stencil_gpu import BOX9, CROSS5, WEIGHTS, run

            if layout == "dense":
                dst, src = plane(gpu, F32, 3, W + 3, 61, width=W), plane(gpu, F32, 3, W + 3, 62, width=W)
                run(dst, 0, src, 0, F32, BOX9, WEIGHTS[BOX9], 3, W, halo=1.5, what="BOX9 (dense)")
                monkeypatch.setenv("STSTHIP_STENCIL_GENERAL", "1")
                run(dst, 0, src, 0, F32, BOX9, WEIGHTS[BOX9], 3, W, halo=1.5, rhs=(dst, 0, (0, 0)), rhs_coef=0.25,
                    what="BOX9 with a right-hand side (general)")
                monkeypatch.delenv("STSTHIP_STENCIL_GENERAL")
            else:
                dst, src = cell_buffer(gpu, "hotspot", 3, W + 3, 63, width=W), cell_buffer(gpu, "hotspot", 3, W + 3, 64, width=W)
                run(dst, 4, src, 0, F32, BOX9, WEIGHTS[BOX9], 3, W, halo=1.5, what="BOX9 on members")
                run(dst, 0, src, 4, F32, CROSS5, WEIGHTS[CROSS5], 3, W, halo=-2.5, what="CROSS5 on members")
            src.unchanged("the source")
        elif family == "norms":
            from test_grid_norms_gpu import aos_cells, expect, grid_of, plane_norms, reference, wide

            rng = np.random.default_rng(71)
            if layout == "dense":
                a = wide(rng, (3, W + 3))
                expect("3 rows of 2049 * 4096 + 5 floats", plane_norms(gpu, a, width=W), reference(a[:, :W]))
            else:
                a, b = aos_cells(rng, (3, W), U.HOTSPOT_CELL), aos_cells(rng, (3, W), U.HOTSPOT_CELL)
                ga = grid_of(gpu, a)
                expect("power", ga.norms(fields=["power"])["power"], reference(a["power"]))
                expect("temp distance", ga.norms(other=grid_of(gpu, b), fields=["temp"])["temp"], reference(a["temp"], b["temp"]))
        else:
            from test_grid_dot_gpu import Planes, dot_of, expect, reference
            from test_grid_norms_gpu import aos_cells, grid_of, wide

            rng = np.random.default_rng(81)
            if layout == "dense":
                p = Planes(gpu, wide(rng, (3, W + 3)), wide(rng, (3, W + 3)))
                expect("3 rows of 2049 * 4096 + 5 floats", dot_of(p.desc(3, W, width=W)), p.want(3, W))
            else:
                a = aos_cells(rng, (3, W), U.HOTSPOT_CELL)
                expect("temp . power", grid_of(gpu, a).dot(field="temp", other_field="power"), reference(a["temp"], a["power"]))
    finally:
        dst = src = cells = flat = a = b = p = ga = coarse = fine = None
        LE.release(f"{case_id}, need {LE.G4_NEED}")


# ------------------------------------------------------------------------------------------ scatter and gather
def test_scatter_and_gather_behind_4_gib(gpu):
    """2^27 + 3 FDTD cells of 32 bytes, an AoS buffer of 4 GiB + 96 bytes behind the front guard, and eight planes of
    floats, in both directions.  Field f of cell i holds the code of operand f at (0, i).  Every plane is compared with
    the AoS member as a whole on the device, and the last 1024 cells and every 4099th cell with the coded values.  (The
    planes are 512 MiB: no offset into them reaches 2^31, so they have guards of 4096 bytes.)"""
    from stencilstream_amd import capi

    LE.require(LE.AOS_NEED)
    n, fields = LE.AOS_CELLS, LE.AOS_FIELDS
    try:
        arena = Arena(gpu, LE.View("A", 0, 4, LE.AOS_CELL_BYTES, n, 1, n))
        cells = torch.as_strided(arena.raw.view(torch.float32), (n, fields), (fields, 1), LE.FRONT_GUARD // 4)
        member = torch.arange(fields, dtype=torch.int64, device=gpu)[None, :]

        def write_cells():
            for begin in range(0, n, 1 << 24):
                index = torch.arange(begin, min(begin + (1 << 24), n), dtype=torch.int64, device=gpu)[:, None]
                cells[begin:begin + (1 << 24)] = LE.code_of(member, 0, index).to(torch.float32)

        write_cells()
        pad = LE.BACK_GUARD // 4
        planes = [torch.full((n + 2 * pad,), LE.SENTINEL_F32, dtype=torch.int32, device=gpu) for _ in range(fields)]
        data = [p[pad:pad + n].view(torch.float32) for p in planes]
        sample = torch.cat([torch.arange(0, n, 4099, device=gpu), torch.arange(n - 1024, n, device=gpu)])
        offsets, sizes = [4 * f for f in range(fields)], [4] * fields

        def check(what):
            for f in range(fields):
                assert bool((planes[f][:pad] == LE.SENTINEL_F32).all()) and bool((planes[f][pad + n:] == LE.SENTINEL_F32).all()), \
                    f"{what}: the guards of plane {f} were written"
                assert torch.equal(data[f].view(torch.int32), cells[:, f].view(torch.int32)), f"{what}: plane {f} is not member {f}"
                want = LE.code_of(f, 0, sample).to(torch.float32)
                assert torch.equal(data[f][sample], want), f"{what}: plane {f} against the coded values"
                assert torch.equal(cells[sample, f], want), f"{what}: member {f} against the coded values"

        torch.cuda.synchronize()
        capi.scatter_fields(arena.base, LE.AOS_CELL_BYTES, n, offsets, sizes, [d.data_ptr() for d in data])
        torch.cuda.synchronize()
        check("scatter")
        whole = LE.Rect(arena.view, 0, 0, 1, n)
        arena.words[LE.FRONT_GUARD // 4:LE.FRONT_GUARD // 4 + n * fields].fill_(LE.SENTINEL_F32)
        arena.assert_clean("scatter")  # (with the cells cleared: the guards of the AoS buffer)
        torch.cuda.synchronize()
        capi.gather_fields(arena.base, LE.AOS_CELL_BYTES, n, offsets, sizes, [d.data_ptr() for d in data])
        torch.cuda.synchronize()
        check("gather")
        arena.words[LE.FRONT_GUARD // 4:LE.FRONT_GUARD // 4 + n * fields].fill_(LE.SENTINEL_F32)
        arena.assert_clean("gather")
        assert whole.last_byte() >= 1 << 32
    finally:
        arena = cells = planes = data = None
        LE.release(f"scatter and gather, need {LE.AOS_NEED}")


# ------------------------------------------------------------------------------------------ one sweep launch
@pytest.mark.parametrize("app", sorted(LE.SWEEP_APPS))
def test_a_sweep_launch_on_rows_256_mib_apart(gpu, oracle, app):
    """One ststhip_app_sweep launch at the deepest compiled depth on 20 x 701 cells (20 x 700 for the packed Game of
    Life) in buffers whose rows lie 2^28 + 44 bytes apart -- for cells of 8 and 32 bytes the next multiple of the cell's
    size, 2^28 + 48 and 2^28 + 64 --: rows 8 and above begin beyond 2^31, rows 16 and above beyond 2^32, and the pitch in
    elements stays below 2^31.  jacobi5general with general coefficients, jacobi5uniform_only (five equal coefficients),
    hotspot on planes and as AoS, fdtd as AoS, conway and conway_packed; the workloads are LaunchWorkload's, the result is
    the oracle's bits, every other byte of the destination and every byte around the source rows stays the sentinel.
    FDTD on eight planes would need about 80 GiB and is left out on purpose."""
    from mesh_threads import split_planes
    from stencilstream_amd import capi
    from sweep_workloads import SENTINEL_LIFE, LaunchWorkload

    H, W = LE.SWEEP_ROWS, LE.SWEEP_APPS[app]
    w = LaunchWorkload(oracle, app, (H, W))
    info = w.info
    sizes = [info.plane_elem_size[p] for p in range(info.n_planes)]
    need = LE.sweep_need(sizes)
    LE.require(need)
    word = LE.SENTINEL_BYTES if w.sentinel is SENTINEL_LIFE else LE.SENTINEL_F32
    pitch = LE.sweep_pitch(sizes[0])
    assert all(LE.sweep_pitch(s) == pitch for s in sizes) and pitch < 1 << 31
    assert 8 * pitch * sizes[0] >= 1 << 31 and 16 * pitch * sizes[0] >= 1 << 32
    try:
        views = [LE.plane(f"plane {p}", 0, pitch, H + 1, W, size) for p, size in enumerate(sizes)]  # (a whole row of padding behind the last)
        src, dst = [Arena(gpu, v, word) for v in views], [Arena(gpu, v, word) for v in views]

        def rows_of(arena, size):
            return torch.as_strided(arena.raw, (H, W * size), (pitch * size, 1), LE.FRONT_GUARD)

        blank = [torch.from_numpy(np.resize(w.sentinel, H * W * size).reshape(H, W * size).copy()).to(gpu) for size in sizes]
        start = [torch.from_numpy(p).to(gpu) for p in split_planes(info, w.cells)]
        for arena, size, rows in zip(src, sizes, start):
            rows_of(arena, size).copy_(rows)
        depth = info.max_generations
        want = split_planes(info, w.want(depth))
        torch.cuda.synchronize()
        capi.app_sweep(app, w.params, w.halo, capi.Domain(H, W, 0, H, pitch), [a.base for a in src], [a.base for a in dst],
                       0, H, w.offset, depth)
        torch.cuda.synchronize()
        got = [rows_of(arena, size).cpu().numpy() for arena, size in zip(dst, sizes)]
        kept = [rows_of(arena, size).cpu().numpy() for arena, size in zip(src, sizes)]
        for p, (a, b, size) in enumerate(zip(src, dst, sizes)):
            rows_of(a, size).copy_(blank[p])
            rows_of(b, size).copy_(blank[p])
            a.assert_clean(f"{app}: source plane {p}")
            b.assert_clean(f"{app}: destination plane {p}")
        for p in range(info.n_planes):
            assert np.array_equal(kept[p], split_planes(info, w.cells)[p]), f"{app}: source plane {p} changed"
            if not np.array_equal(got[p], want[p]):
                bad = np.argwhere(got[p] != want[p])
                raise AssertionError(f"{app} depth {depth}, plane {p}: {len(bad)} bytes differ from the oracle in rows "
                                     f"{sorted(set(bad[:, 0].tolist()))}, the first at row {bad[0][0]}, element {bad[0][1] // sizes[p]}")
    finally:
        src = dst = blank = start = None
        LE.release(f"sweep {app}, need {need}")

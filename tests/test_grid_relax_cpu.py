"""ststhip_grid_relax without a GPU: the header declares it and the library exports it, the ctypes mirror has the layout
of the C struct, every bad argument is refused before anything touches the device (status 2, "grid relax ..."), empty
rectangles need no device, the overlap rule accepts another member of the cells and nothing else, and update.Grid.relax
raises ValueError for bad input.

The model of the GPU tests lives here too (tests/test_grid_relax_gpu.py imports it): numpy in the element's dtype,
colour masks over an array padded with the halo, operation by operation as ststhip.h states it.  It is checked on a
3 x 3 case worked by hand, and its own properties on a 48 x 40 Poisson problem: red-black Gauss-Seidel needs fewer sweeps
than the Jacobi relaxation of INTEGRATION.md, and evaluating the product-sums fused changes result bits of the f32 test
data, so a kernel that fuses cannot pass the GPU tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INVALID = 2  # STSTHIP_ERR_INVALID
BASE, OTHER = 0x100000, 0x900000  # made-up addresses: nothing here reaches a device
F32, F64 = "<f4", "<f8"
FIVE = [0.2, 0.4, 0.5, 0.6, 0.8]
NAME = "ststhip_grid_relax"
INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------ the model, operation by operation
def cross_model(dtype, cross, view, halo, rhs=None, rhs_coef=1.0, fused=False):
    """The CROSS5 formula of ststhip.h for EVERY cell of `view` (height x width), out of place: acc = T(w_n) * N, then
    acc = acc + T(w_k) * s_k for W, C, E, S, then acc = acc + T(rhs_coef) * rhs.  fused: every `acc + w * s` rounded
    once, as a fused multiply-add would (f32 only: through float64, where the product is exact)."""
    dtype = np.dtype(dtype)
    T = dtype.type
    padded = np.full((view.shape[0] + 2, view.shape[1] + 2), T(halo), dtype=dtype)
    padded[1:-1, 1:-1] = view
    n, w, c, e, s = padded[0:-2, 1:-1], padded[1:-1, 0:-2], padded[1:-1, 1:-1], padded[1:-1, 2:], padded[2:, 1:-1]

    def add(acc, weight, x):
        if fused:
            assert dtype == np.dtype(F32)
            return (acc.astype(np.float64) + np.float64(T(weight)) * x.astype(np.float64)).astype(dtype)
        return acc + T(weight) * x

    with np.errstate(all="ignore"):
        acc = T(cross[0]) * n
        acc = add(acc, cross[1], w)
        acc = add(acc, cross[2], c)
        acc = add(acc, cross[3], e)
        acc = add(acc, cross[4], s)
        if rhs is not None:
            acc = add(acc, rhs_coef, rhs)
    assert acc.dtype == dtype and acc.shape == view.shape
    return acc


def relax_model(dtype, cross, view, at, n_rows, n_cols, halo, first_colour=0, half_sweeps=2, parity=0, rhs=None,
                rhs_coef=1.0, fused=False):
    """The whole view (height x width) after the half-sweeps over the n_rows x n_cols rectangle at `at`; rhs: the
    rectangle's n_rows x n_cols values.  A half-sweep computes every cell from the view as the previous one left it and
    keeps the cells of its colour inside the rectangle: their neighbours have the other colour."""
    dtype = np.dtype(dtype)
    u = np.array(view, dtype=dtype)
    rows, cols = np.indices(u.shape)
    rect = (rows >= at[0]) & (rows < at[0] + n_rows) & (cols >= at[1]) & (cols < at[1] + n_cols)
    f = None
    if rhs is not None:
        f = np.zeros(u.shape, dtype=dtype)
        f[at[0]:at[0] + n_rows, at[1]:at[1] + n_cols] = rhs
    for k in range(half_sweeps):
        active = rect & (((rows + cols + parity) & 1) == ((first_colour + k) & 1))
        u[active] = cross_model(dtype, cross, u, halo, f, rhs_coef, fused)[active]
    return u


def test_the_model_on_a_case_worked_by_hand():
    """3 x 3 view 1 .. 9, weights n, w, c, e, s = 1 .. 5, halo 10."""
    view = np.arange(1, 10, dtype=F32).reshape(3, 3)
    w = [1, 2, 3, 4, 5]
    red = relax_model(F32, w, view, (0, 0), 3, 3, 10.0, half_sweeps=1)
    assert red[1, 1] == 1 * 2 + 2 * 4 + 3 * 5 + 4 * 6 + 5 * 8 == 89
    assert red[0, 0] == 1 * 10 + 2 * 10 + 3 * 1 + 4 * 2 + 5 * 4 == 61  # north and west are halo
    assert red[0, 2] == 1 * 10 + 2 * 2 + 3 * 3 + 4 * 10 + 5 * 6 == 93
    assert (red[0, 1], red[1, 0], red[1, 2], red[2, 1]) == (2, 4, 6, 8)  # the other colour keeps its values
    # the second half-sweep reads what the first left: (0, 1) sees the new (0, 0), (0, 2) and (1, 1)
    both = relax_model(F32, w, view, (0, 0), 3, 3, 10.0, half_sweeps=2)
    assert both[0, 1] == 1 * 10 + 2 * 61 + 3 * 2 + 4 * 93 + 5 * 89 == 955
    assert both[1, 1] == 89
    # the other colour first, parity, a right-hand side, and a rectangle whose neighbours are cells of the view
    assert relax_model(F32, w, view, (0, 0), 3, 3, 10.0, 1, 1)[0, 1] == 1 * 10 + 2 * 1 + 3 * 2 + 4 * 3 + 5 * 5
    shifted = relax_model(F32, w, view, (0, 0), 3, 3, 10.0, 0, 1, 1)  # parity 1: colour 0 is where r + q is odd
    assert shifted[0, 1] == 55 and shifted[1, 1] == 5
    inner = relax_model(F32, w, view, (1, 1), 1, 1, 10.0, 0, 2, 0, np.full((1, 1), 2, F32), 0.5)
    assert inner[1, 1] == 89 + 1 and np.array_equal(np.delete(inner.reshape(-1), 4), np.delete(view.reshape(-1), 4))


# ------------------------------------------------------------------ the model's own properties: a Poisson problem
PH, PW = 48, 40
H2 = 1.0 / 2304.0  # h = 1 / 48
MINUS_A = (1.0 / H2, 1.0 / H2, -4.0 / H2, 1.0 / H2, 1.0 / H2)  # A u = (4 u - N - W - E - S) / h^2
JACOBI = (0.25, 0.25, 0.0, 0.25, 0.25)
MAX_SWEEPS = 4000


def sor(omega):
    return (omega / 4, omega / 4, 1 - omega, omega / 4, omega / 4)


def poisson_f():
    rng = np.random.default_rng(0x50150)
    return (200.0 * (rng.random((PH, PW), dtype=np.float32) - 0.5)).astype(F32)


def poisson_tolerance(f):
    """A twentieth of the first residual (u = 0: the residual is f), as a float."""
    return float(np.abs(f).max()) / 20.0


def residual_max(u, f):
    return float(np.abs(cross_model(F32, MINUS_A, u, 0.0, f, 1.0)).max())  # |f - A u|


def solve(f, sweep):
    """(sweeps, u): u <- sweep(u) from zero until the residual's largest element is within the tolerance."""
    u, tolerance = np.zeros((PH, PW), dtype=F32), poisson_tolerance(f)
    for count in range(1, MAX_SWEEPS + 1):
        u = sweep(u)
        if residual_max(u, f) <= tolerance:
            return count, u
    raise AssertionError(f"no convergence in {MAX_SWEEPS} sweeps")


def red_black(f, omega):
    return solve(f, lambda u: relax_model(F32, sor(omega), u, (0, 0), PH, PW, 0.0, rhs=f, rhs_coef=omega * H2 / 4))


def test_red_black_converges_faster_than_jacobi():
    f = poisson_f()
    jacobi, _ = solve(f, lambda u: cross_model(F32, JACOBI, u, 0.0, f, H2 / 4))
    gauss_seidel, _ = red_black(f, 1.0)
    over_relaxed, _ = red_black(f, 1.5)
    assert over_relaxed < gauss_seidel < jacobi, (over_relaxed, gauss_seidel, jacobi)
    assert 3 * gauss_seidel < 2 * jacobi, (gauss_seidel, jacobi)  # about twice as fast per sweep


def test_a_fused_evaluation_changes_bits():
    """The data of the GPU tests: random planes in (-1, 1) with distinct weights, and the Poisson problem."""
    rng = np.random.default_rng(7)
    u = (2.0 * rng.random((12, 70)) - 1.0).astype(F32)
    f = (2.0 * rng.random((12, 70)) - 1.0).astype(F32)
    weights = [-0.23, 0.41, -0.53, 0.67, -0.83]
    for rhs in (None, f):
        plain = relax_model(F32, weights, u, (0, 0), 12, 70, 0.5, rhs=rhs, rhs_coef=-0.3)
        fused = relax_model(F32, weights, u, (0, 0), 12, 70, 0.5, rhs=rhs, rhs_coef=-0.3, fused=True)
        differ = plain.view(np.uint32) != fused.view(np.uint32)
        assert differ.mean() > 0.1, differ.mean()
    g = poisson_f()
    zero = np.zeros((PH, PW), dtype=F32)
    plain = relax_model(F32, sor(1.5), zero, (0, 0), PH, PW, 0.0, half_sweeps=4, rhs=g, rhs_coef=1.5 * H2 / 4)
    fused = relax_model(F32, sor(1.5), zero, (0, 0), PH, PW, 0.0, half_sweeps=4, rhs=g, rhs_coef=1.5 * H2 / 4, fused=True)
    assert (plain.view(np.uint32) != fused.view(np.uint32)).any()


# ------------------------------------------------------------------ the library without a device
def test_header_binding_and_symbols(built_lib):
    from stencilstream_amd import capi

    assert hasattr(capi, "grid_relax"), "stencilstream_amd.capi has no grid_relax"
    header = open(os.path.join(ROOT, "include", "ststhip.h")).read()
    for name in ("ststhip_grid_relax(", "ststhip_grid_relax_desc"):
        assert name in header, name
    for name in ("grid_relax", "grid_relax_desc"):
        assert callable(getattr(capi, name))
    raw = C.CDLL(os.path.join(ROOT, "stencilstream_amd", "libststhip.so"))
    assert hasattr(raw, NAME), f"libststhip.so lacks {NAME}"
    assert built_lib.ststhip_abi_version() == 6  # additive


def test_ctypes_struct_mirrors_the_c_struct(built_lib, tmp_path):
    from stencilstream_amd import capi

    c_name, mirror = "ststhip_grid_relax_desc", capi.GridRelaxDesc
    lines = ["#include <cstdio>", "#include <cstddef>", '#include "ststhip.h"', "int main() {",
             f'    std::printf("{c_name} %zu\\n", sizeof({c_name}));']
    for member, _ in mirror._fields_:
        lines.append(f'    std::printf("{c_name}.{member} %zu\\n", offsetof({c_name}, {member}));')
    lines.append("}")
    source = tmp_path / "layout.cpp"
    source.write_text("\n".join(lines) + "\n")
    program = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(source), "-o", str(program)], check=True)
    out = subprocess.run([str(program)], check=True, capture_output=True, text=True).stdout.splitlines()
    want = {key: int(value) for key, value in (line.split() for line in out)}
    got = {c_name: C.sizeof(mirror)}
    for member, _ in mirror._fields_:
        got[f"{c_name}.{member}"] = getattr(mirror, member).offset
    assert got == want
    assert len(want) == 1 + len(mirror._fields_)
    assert mirror.weight.size == 5 * 8


def view(base=BASE, stride=4, height=8, width=8, pitch=None):
    from stencilstream_amd import capi

    return capi.grid_view(base, stride, height, width, pitch)


def cells(offset=0, base=BASE, stride=32):
    """A member of the 32-byte cells of an 8 x 8 grid."""
    return view(base + offset, stride=stride)


def relax(u=None, dtype=F32, weights=None, n_rows=4, n_cols=4, rhs=None, **kw):
    """A valid relaxation of a 4 x 4 rectangle of an 8 x 8 plane; the arguments break it."""
    from stencilstream_amd import capi

    changes = {k: kw.pop(k) for k in list(kw) if k in ("type", "reserved", "has_rhs")}
    d = capi.grid_relax_desc(view() if u is None else u, dtype, FIVE if weights is None else weights, n_rows, n_cols,
                             rhs=rhs, **kw)
    for name, value in changes.items():
        setattr(d, name, value)
    return d


def with_weight(k, value, **kw):
    weights = list(FIVE)
    weights[k] = value
    return relax(weights=weights, **kw)


BAD = {
    "no entry": lambda: [],
    "nine entries": lambda: [relax()] * 9,
    "unknown type": lambda: [relax(type=2)],
    "first_colour 2": lambda: [relax(first_colour=2)],
    "parity 2": lambda: [relax(parity=2)],
    "no half-sweep": lambda: [relax(half_sweeps=0)],
    "1025 half-sweeps": lambda: [relax(half_sweeps=1025)],
    "reserved set": lambda: [relax(reserved=1)],
    "stride 0": lambda: [relax(view(stride=0))],
    "right-hand side stride 0": lambda: [relax(rhs=view(OTHER, stride=0))],
    "pitch below the width": lambda: [relax(view(pitch=7))],
    "right-hand side pitch below the width": lambda: [relax(rhs=view(OTHER, pitch=7))],
    "null base": lambda: [relax(view(0))],
    "null right-hand side": lambda: [relax(rhs=view(0))],
    "has_rhs without a view": lambda: [relax(has_rhs=1)],
    "base off by two bytes": lambda: [relax(view(BASE + 2))],
    "f64 base off by four bytes": lambda: [relax(view(BASE + 4, stride=8), F64)],
    "f64 right-hand side base off by four bytes": lambda: [relax(view(stride=8), F64, rhs=view(OTHER + 4, stride=8))],
    "stride no multiple of the element": lambda: [relax(view(stride=6))],
    "f64 in twelve-byte cells": lambda: [relax(view(stride=12), F64)],
    "extents past 2^63 bytes": lambda: [relax(view(height=2 ** 62, pitch=2 ** 20))],
    "right-hand side extents past 2^63 bytes": lambda: [relax(rhs=view(OTHER, height=2 ** 62, pitch=2 ** 20))],
    "rows past the view": lambda: [relax(u_at=(5, 0))],
    "columns past the view": lambda: [relax(u_at=(0, 5))],
    "row past 2^64": lambda: [relax(u_at=(2 ** 64 - 2, 0))],
    "right-hand side rows past the view": lambda: [relax(rhs=view(OTHER), rhs_at=(5, 0))],
    "right-hand side columns past the view": lambda: [relax(rhs=view(OTHER), rhs_at=(0, 5))],
    "2^31 rows": lambda: [relax(view(height=2 ** 32), n_rows=2 ** 31)],
    "2^31 columns": lambda: [relax(view(width=2 ** 32), n_cols=2 ** 31)],
    "2^31 rows of no columns": lambda: [relax(n_rows=2 ** 31, n_cols=0)],
    "a row of 2^31 bytes": lambda: [relax(view(stride=2 ** 29))],
    "a right-hand side row of 2^31 bytes": lambda: [relax(rhs=view(OTHER + 2 ** 40, stride=2 ** 29))],
    "an infinite weight": lambda: [with_weight(2, INF)],
    "a NaN weight": lambda: [with_weight(0, NAN)],
    "a NaN south weight": lambda: [with_weight(4, NAN)],
    "an infinite rhs_coef": lambda: [relax(rhs=view(OTHER), rhs_coef=-INF)],
    "a NaN rhs_coef": lambda: [relax(rhs=view(OTHER), rhs_coef=NAN)],
    "overlap: the right-hand side is u": lambda: [relax(rhs=view())],
    "overlap: the right-hand side is u, on a member": lambda: [relax(cells(8), rhs=cells(8))],
    "overlap: the right-hand side shifted by one element": lambda: [relax(rhs=view(), rhs_at=(0, 1))],
    "overlap: the right-hand side shifted by one row": lambda: [relax(rhs=view(), rhs_at=(1, 0))],
    # the rectangles are disjoint, but column 4 of u is read as the neighbour of column 3
    "overlap: the right-hand side is a neighbour that is read": lambda: [relax(n_rows=8, rhs=view(), rhs_at=(0, 4))],
    "overlap: the right-hand side is the row below": lambda: [relax(n_cols=8, rhs=view(), rhs_at=(4, 0))],
    # rhs begins where row 4 of the view of u does: outside the 4 x 8 rectangle, but read as its neighbour
    "overlap: onto the row below the rectangle": lambda: [relax(n_cols=8, rhs=view(BASE + 4 * 8 * 4, height=4))],
    "overlap: u with another pitch": lambda: [relax(rhs=view(BASE, 4, 4, 8, 16))],
    "overlap: a member running into the next cell": lambda: [relax(cells(0, stride=8), rhs=cells(8, stride=8))],
    "overlap: an f64 member running into the next cell": lambda: [relax(cells(0, stride=16), F64, rhs=cells(16, stride=16))],
    "overlap: a member of other cells": lambda: [relax(cells(8), rhs=cells(16), rhs_at=(0, 1))],
    "overlap: member to member with another pitch": lambda: [relax(cells(16), rhs=view(BASE + 8, 32, 4, 8, 16))],
    "second entry bad": lambda: [relax(), relax(u_at=(5, 0))],
}


def call(built_lib, entries):
    from stencilstream_amd import capi

    table = (capi.GridRelaxDesc * max(len(entries), 1))(*entries)
    return getattr(built_lib, NAME)(len(entries), table, None)


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_are_refused_before_the_device(built_lib, case):
    """STSTHIP_ERR_INVALID, not "no GPU" (4), on a machine without one: validation comes first."""
    from stencilstream_amd import capi

    status = call(built_lib, BAD[case]())
    assert status == INVALID, (status, capi.last_error())
    assert capi.last_error().startswith("grid relax"), capi.last_error()


def test_null_table_is_refused(built_lib):
    from stencilstream_amd import capi

    assert getattr(built_lib, NAME)(1, None, None) == INVALID
    assert capi.last_error().startswith("grid relax")


def test_the_wrappers_raise(built_lib):
    from stencilstream_amd import capi

    with pytest.raises(capi.StsthipError) as e:
        capi.grid_relax([relax(u_at=(5, 0))])
    assert e.value.status == INVALID
    with pytest.raises(ValueError):
        capi.grid_relax_desc(view(), "<i4", FIVE, 4, 4)
    with pytest.raises(ValueError):
        capi.grid_relax_desc(view(), F32, FIVE[:4], 4, 4)
    made = capi.grid_relax_desc(view(), F32, FIVE, 4, 4)
    assert list(made.weight) == FIVE and (made.has_rhs, made.reserved, made.first_colour, made.n_half_sweeps, made.parity) == (0, 0, 0, 2, 0)


def test_empty_rectangles_need_no_device(built_lib):
    """Nothing to compute: success on the host, also for null bases."""
    from stencilstream_amd import capi

    null = view(0)
    capi.grid_relax([relax(null, n_rows=0), relax(n_cols=0), relax(null, rhs=null, n_rows=0, n_cols=0),
                     relax(view(0, stride=8), F64, n_cols=0, half_sweeps=1024)])
    capi.grid_relax([relax(n_rows=0, u_at=(100, 100))])  # an empty rectangle may start anywhere
    capi.grid_relax([relax(rhs=view(), n_rows=0)])  # ... and overlaps nothing


ACCEPTED = {
    "plain": lambda: [relax()],
    "doubles": lambda: [relax(view(stride=8), F64)],
    "every colour, parity and count": lambda: [relax(first_colour=1, parity=1, half_sweeps=1024), relax(half_sweeps=1)],
    "up to the last cell": lambda: [relax(u_at=(4, 4))],
    "a non-finite halo": lambda: [relax(halo=NAN), relax(halo=-INF)],
    "with a right-hand side": lambda: [relax(rhs=view(OTHER), rhs_coef=0.25)],
    "a non-finite rhs_coef that is not used": lambda: [relax(rhs_coef=NAN)],
    "the right-hand side another member of the cells": lambda: [relax(cells(8), rhs=cells(16))],
    "the member in front of it": lambda: [relax(cells(28), rhs=cells(0))],
    "an f64 member beside it": lambda: [relax(cells(0, stride=16), F64, rhs=cells(8, stride=16))],
    "another member, on an inner rectangle": lambda: [relax(cells(8), u_at=(2, 3), rhs=cells(12), rhs_at=(2, 3))],
    # rows 0..2 relaxed, row 3 read; the right-hand side begins in row 4
    "apart by the one row that is read": lambda: [relax(n_rows=3, n_cols=8, rhs=view(), rhs_at=(4, 0))],
    # the same addresses as the refused case, but the view of u ends with the rectangle: row 4 is halo and is not read
    "beside what it does not read": lambda: [relax(view(height=4), n_cols=8, rhs=view(BASE + 4 * 8 * 4, height=4))],
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_a_valid_call_gets_as_far_as_the_device(built_lib, case):
    """Without a GPU a valid, non-empty call fails for want of a device: neither success nor a bad argument."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the made-up addresses must not reach it")
    assert call(built_lib, ACCEPTED[case]()) not in (0, INVALID)


def test_grid_method_refuses_bad_input(built_lib):
    from stencilstream_amd import update as U

    grid = U.Grid(6, 8, U.HOTSPOT_CELL, device="cpu")  # (no call below gets as far as the cells)
    same = U.Grid(6, 8, U.FDTD_CELL, device="cpu")
    plane = U.Grid(6, 8, "<f4", device="cpu")
    other = U.Grid(6, 8, "<f4", device="cpu")
    doubles = U.Grid(6, 8, U.HOTSPOT_CELL_F64, device="cpu")
    small = U.Grid(3, 4, "<f4", device="cpu")
    ints = U.Grid(6, 8, U.SELFCHECK_CELL, device="cpu")
    cross = (0.25, 0.25, 0.0, 0.25, 0.25)
    bad = [
        lambda: plane.relax(cross=(1, 2, 3, 4)),  # not five weights
        lambda: plane.relax(cross=[[1, 2, 3], [4, 5, 6], [7, 8, 9]]),
        lambda: plane.relax(cross=(1, 2, float("nan"), 4, 5)),
        lambda: plane.relax(cross=(1, 2, 3, 4, float("inf"))),
        lambda: plane.relax(cross=cross, rhs=other, rhs_coef=float("inf")),
        lambda: plane.relax(cross=cross, rhs=plane),  # the relaxed element itself
        lambda: grid.relax(cross=cross, field="temp", rhs=grid, rhs_field="temp"),
        lambda: grid.relax(cross=cross),  # no field of a structured cell
        lambda: grid.relax(cross=cross, field="pressure"),
        lambda: grid.relax(cross=cross, field="temp", rhs=same),  # the right-hand side names no field
        lambda: grid.relax(cross=cross, field="temp", rhs=same, rhs_field="pressure"),
        lambda: grid.relax(cross=cross, field="temp", rhs=doubles, rhs_field="power"),  # another dtype
        lambda: grid.relax(cross=cross, field="temp", rhs_field="power"),  # no right-hand side to name a field of
        lambda: plane.relax(cross=cross, rhs=small),  # another extent
        lambda: plane.relax(cross=cross, rows=(0, 7)),
        lambda: plane.relax(cross=cross, cols=(5, 4)),
        lambda: ints.relax(cross=cross, field="status"),  # not a float
        lambda: plane.relax(cross=cross, field="temp"),  # plain cells have no fields
        lambda: plane.relax(cross=cross, first_colour=2),
        lambda: plane.relax(cross=cross, first_colour=-1),
        lambda: plane.relax(cross=cross, parity=2),
        lambda: plane.relax(cross=cross, parity=0.5),
        lambda: plane.relax(cross=cross, half_sweeps=0),
        lambda: plane.relax(cross=cross, half_sweeps=1025),
        lambda: plane.relax(cross=cross, half_sweeps=2.0),
    ]
    for number, attempt in enumerate(bad):
        with pytest.raises(ValueError):
            attempt()
            pytest.fail(f"attempt {number} was accepted")
    with pytest.raises(TypeError):
        plane.relax(cross)  # the weights are a keyword argument
    # an empty range is nothing, and needs no device
    plane.relax(cross=cross, rows=(2, 2))
    plane.relax(cross=cross, rhs=other, cols=(8, 8), half_sweeps=1024, first_colour=1, parity=1)
    grid.relax(cross=cross, field="temp", rhs=grid, rhs_field="power", rows=(3, 3))

"""ststhip_grid_diffusion without a GPU: the header declares it and the library exports it, the ctypes mirror has the
layout of the C struct, every bad argument is refused before anything touches the device (status 2, "grid diffusion
..."), empty rectangles need no device, the overlap rules accept another member of the cells (and the right-hand side in
place) and nothing else, and update.Grid.diffusion raises ValueError for bad input.

The model of the GPU tests lives here too (tests/test_grid_diffusion_gpu.py imports it): numpy in the element's dtype
over arrays padded with the halo (u) and with k_halo (kx, ky, each by its own extents), operation by operation as
ststhip.h states it.  It is checked on a 3 x 3 case worked by hand, and its own properties: constants give exactly zero
under insulated outer faces, the operator is symmetric, a fused evaluation changes result bits of the f32 test data (so a
kernel that fuses cannot pass the GPU tests), and on a 48 x 40 problem whose coefficients span three decades
Jacobi-preconditioned conjugate gradients need fewer than a quarter of the plain method's iterations."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INVALID = 2  # STSTHIP_ERR_INVALID
# made-up addresses: nothing here reaches a device
BASE, U_AT, KX_AT, KY_AT, OTHER = 0x100000, 0x300000, 0x500000, 0x700000, 0x900000
F32, F64 = "<f4", "<f8"
NAME = "ststhip_grid_diffusion"
INF, NAN = float("inf"), float("nan")
APPLY, JACOBI, SOLVE_DIAG = 0, 1, 2


# ------------------------------------------------------------------ the model, operation by operation
def _padded(view, value, dtype):
    padded = np.full((view.shape[0] + 2, view.shape[1] + 2), dtype.type(value), dtype=dtype)
    padded[1:-1, 1:-1] = view
    return padded


def diffusion_model(dtype, mode, u, kx, ky, n_rows, n_cols, u_at=(0, 0), kx_at=(0, 0), ky_at=(0, 0), halo=0.0, k_halo=0.0,
                    sigma=0.0, scale=1.0, omega=1.0, rhs=None, rhs_coef=1.0, fused=False):
    """The formula of ststhip.h for the n_rows x n_cols rectangle.  u, kx, ky: the WHOLE views (u may be None in
    SOLVE_DIAG); the rectangle begins at u_at, kx_at, ky_at in them; rhs: the rectangle's values.  fused: every
    `acc + k * (c - x)` and `y + scale * acc` rounded once, as a fused multiply-add would (f32 only: through float64,
    where the product is exact)."""
    dtype = np.dtype(dtype)
    T = dtype.type

    def window(padded, at, a, b):
        r, q = at[0] + 1 + a, at[1] + 1 + b
        return padded[r:r + n_rows, q:q + n_cols]

    def add(acc, factor, x):
        if fused:
            assert dtype == np.dtype(F32)
            return (acc.astype(np.float64) + np.asarray(factor, dtype).astype(np.float64) * x.astype(np.float64)).astype(dtype)
        return acc + factor * x

    east, south = _padded(kx, k_halo, dtype), _padded(ky, k_halo, dtype)
    ke, kw = window(east, kx_at, 0, 0), window(east, kx_at, 0, -1)
    ks, kn = window(south, ky_at, 0, 0), window(south, ky_at, -1, 0)
    with np.errstate(all="ignore"):
        if mode != SOLVE_DIAG:
            centre = _padded(u, halo, dtype)
            c, n, w = window(centre, u_at, 0, 0), window(centre, u_at, -1, 0), window(centre, u_at, 0, -1)
            e, s = window(centre, u_at, 0, 1), window(centre, u_at, 1, 0)
            acc = kn * (c - n)
            acc = add(acc, kw, c - w)
            acc = add(acc, ke, c - e)
            acc = add(acc, ks, c - s)
        if mode != APPLY:
            d = kn + kw
            d = d + ke
            d = d + ks
            d = T(scale) * d
            d = T(sigma) + d
        if mode == APPLY:
            y = T(sigma) * c
            y = add(y, T(scale), acc)
            if rhs is not None:
                y = add(y, T(rhs_coef), rhs)
        elif mode == JACOBI:
            t = T(sigma) * c
            t = add(t, T(scale), acc)
            r = T(rhs_coef) * rhs
            r = r - t
            y = c + T(omega) * (r / d)
        else:
            y = (T(rhs_coef) * rhs) / d
    assert y.dtype == dtype and y.shape == (n_rows, n_cols)
    return y


def whole(dtype, mode, u, kx, ky, **kw):
    """The model on whole views of one extent."""
    return diffusion_model(dtype, mode, u, kx, ky, kx.shape[0], kx.shape[1], **kw)


def test_the_model_on_a_case_worked_by_hand():
    """3 x 3 views: u = 1 .. 9, kx = 10 .. 90, ky = 100 .. 900; halo 20, k_halo 7."""
    u = np.arange(1, 10, dtype=F32).reshape(3, 3)
    kx = 10 * np.arange(1, 10, dtype=F32).reshape(3, 3)
    ky = 100 * np.arange(1, 10, dtype=F32).reshape(3, 3)
    f = np.full((3, 3), 8, dtype=F32)
    common = dict(halo=20.0, k_halo=7.0, sigma=2.0, scale=0.5)
    # the centre: c = 5, n = 2, w = 4, e = 6, s = 8; kn = ky(0,1) = 200, kw = kx(1,0) = 40, ke = 50, ks = 500
    acc = 200 * (5 - 2) + 40 * (5 - 4) + 50 * (5 - 6) + 500 * (5 - 8)
    d = 2 + 0.5 * (200 + 40 + 50 + 500)
    assert acc == -910 and d == 397
    assert whole(F32, APPLY, u, kx, ky, **common)[1, 1] == 2 * 5 + 0.5 * acc == -445
    assert whole(F32, APPLY, u, kx, ky, rhs=f, rhs_coef=0.25, **common)[1, 1] == -443
    assert whole(F32, JACOBI, u, kx, ky, rhs=f, rhs_coef=0.25, omega=397.0, **common)[1, 1] == 5 + (2 - -445) == 452
    assert whole(F32, SOLVE_DIAG, None, kx, ky, rhs=f, rhs_coef=397.0 / 8, **common)[1, 1] == 1
    # the corner (0, 0): n and w are the halo, kn and kw are k_halo; ke = 10, ks = 100, e = 2, s = 4
    acc = 7 * (1 - 20) + 7 * (1 - 20) + 10 * (1 - 2) + 100 * (1 - 4)
    d = 2 + 0.5 * (7 + 7 + 10 + 100)
    assert acc == -576 and d == 64
    assert whole(F32, APPLY, u, kx, ky, **common)[0, 0] == 2 + 0.5 * acc == -286
    assert whole(F32, JACOBI, u, kx, ky, rhs=f, rhs_coef=0.25, omega=32.0, **common)[0, 0] == 1 + 32 * ((2 + 286) / 64) == 145
    assert whole(F32, SOLVE_DIAG, None, kx, ky, rhs=f, rhs_coef=16.0, **common)[0, 0] == 2
    # the corner (2, 2): e and s are the halo, but ke and ks are this cell's own faces, 90 and 900
    acc = 600 * (9 - 6) + 80 * (9 - 8) + 90 * (9 - 20) + 900 * (9 - 20)
    assert whole(F32, APPLY, u, kx, ky, **common)[2, 2] == 2 * 9 + 0.5 * acc
    # a rectangle inside larger views of other extents: cell (1, 1) again, seen from three different origins
    big_u, big_kx, big_ky = np.zeros((5, 6), F32), np.zeros((4, 4), F32), np.zeros((6, 3), F32)
    big_u[2:5, 1:4], big_kx[0:3, 1:4], big_ky[3:6, 0:3] = u, kx, ky
    one = diffusion_model(F32, APPLY, big_u, big_kx, big_ky, 1, 1, (3, 2), (1, 2), (4, 1), **common)
    assert one[0, 0] == -445
    # ... and (0, 0) of the small views from there: every view goes on to the north and to the west (zeros), so neither
    # the halo nor k_halo is read
    edge = diffusion_model(F32, APPLY, big_u, big_kx, big_ky, 1, 1, (2, 1), (0, 1), (3, 0), **common)
    assert edge[0, 0] == 2 + 0.5 * (0 * (1 - 0) + 0 * (1 - 0) + 10 * (1 - 2) + 100 * (1 - 4))
    # the same cell where ky's view begins with the rectangle's row: kn alone is k_halo, judged by ky's own extents
    top = diffusion_model(F32, APPLY, big_u, big_kx, big_ky[3:], 1, 1, (2, 1), (0, 1), (0, 0), **common)
    assert top[0, 0] == 2 + 0.5 * (7 * (1 - 0) + 0 * (1 - 0) + 10 * (1 - 2) + 100 * (1 - 4))


def random_faces(rng, shape, dtype):
    """Face coefficients of two materials, 1 and 1000, times a factor in (0.5, 1.5)."""
    return (np.where(rng.random(shape) < 0.5, 1.0, 1000.0) * rng.uniform(0.5, 1.5, shape)).astype(dtype)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_constants_give_exactly_zero_under_insulated_faces(dtype):
    rng = np.random.default_rng(5)
    kx, ky = random_faces(rng, (48, 70), dtype), random_faces(rng, (48, 70), dtype)
    kx[:, -1] = 0
    ky[-1, :] = 0
    u = np.full((48, 70), 3.7, dtype=dtype)
    y = whole(dtype, APPLY, u, kx, ky, halo=123.0, k_halo=0.0, scale=2.5)
    assert np.all(y == 0) and not np.signbit(y).any()
    # a ring of zero faces cuts a cell out: its row of the operator is sigma alone
    kx[20, 30] = kx[20, 29] = ky[20, 30] = ky[19, 30] = 0
    u = rng.standard_normal((48, 70)).astype(dtype)
    y = whole(dtype, APPLY, u, kx, ky, sigma=0.5)
    assert y[20, 30] == np.dtype(dtype).type(0.5) * u[20, 30]


def test_the_operator_is_symmetric():
    rng = np.random.default_rng(6)
    kx, ky = random_faces(rng, (48, 70), F64), random_faces(rng, (48, 70), F64)
    u, v = rng.standard_normal((48, 70)), rng.standard_normal((48, 70))
    a = np.sum(v * whole(F64, APPLY, u, kx, ky, k_halo=1.0, sigma=0.1))
    b = np.sum(u * whole(F64, APPLY, v, kx, ky, k_halo=1.0, sigma=0.1))
    assert abs(a - b) <= 1e-12 * abs(a), (a, b)


def test_a_fused_evaluation_changes_bits():
    """The data of the GPU tests: random planes in (-1, 1)."""
    rng = np.random.default_rng(7)
    u, kx, ky, f = ((2.0 * rng.random((12, 70)) - 1.0).astype(F32) for _ in range(4))
    common = dict(halo=0.5, k_halo=1.0, sigma=0.3, scale=0.7)
    for mode, more in ((APPLY, {}), (APPLY, dict(rhs=f, rhs_coef=-0.3)), (JACOBI, dict(rhs=f, rhs_coef=-0.3, omega=0.8))):
        plain = whole(F32, mode, u, kx, ky, **common, **more)
        fused = whole(F32, mode, u, kx, ky, fused=True, **common, **more)
        differ = plain.view(np.uint32) != fused.view(np.uint32)
        assert differ.mean() > 0.1, differ.mean()


# ------------------------------------------------------------------ preconditioned conjugate gradients
PH, PW = 48, 40
MAX_ITERATIONS = 5000
TOLERANCE = {F64: 1e-10, F32: 1e-5}


def pcg_problem(dtype):
    """(kx, ky, f): coefficients that grow by three decades from the first row to the last."""
    r, q = np.indices((PH, PW)).astype(np.float64)
    kx = 10.0 ** (3.0 * r / 47.0) * (1.0 + 0.5 * np.sin(0.7 * q + 0.3 * r))
    ky = 10.0 ** (3.0 * r / 47.0) * (1.0 + 0.5 * np.cos(0.4 * q - 0.9 * r))
    f = np.random.default_rng(11).standard_normal((PH, PW))
    return kx.astype(dtype), ky.astype(dtype), f.astype(dtype)


def dot_numpy(a, b):
    return float(np.dot(a.astype(np.float64).reshape(-1), b.astype(np.float64).reshape(-1)))


def dot_fsum(a, b):
    return math.fsum((a.astype(np.float64) * b.astype(np.float64)).reshape(-1).tolist())


def dot_reversed(a, b):
    return float(np.sum((a.astype(np.float64) * b.astype(np.float64)).reshape(-1)[::-1]))


def pcg_model(kx, ky, f, tolerance, preconditioned=True, dot=dot_numpy):
    """A x = f with halo 0, k_halo 1, sigma 0, scale 1, until |r| / |f| <= tolerance: the loop of the GPU test in numpy,
    the same combines in f's dtype, the dots in float64.  Returns (x, iterations)."""
    dtype = f.dtype
    T = dtype.type

    def solve(r):
        return whole(dtype, SOLVE_DIAG, None, kx, ky, k_halo=1.0, rhs=r) if preconditioned else r.copy()

    x, r = np.zeros_like(f), f.copy()
    z = solve(r)
    p = z.copy()
    ff, rz = dot(r, r), dot(r, z)
    for iteration in range(1, MAX_ITERATIONS + 1):
        ap = whole(dtype, APPLY, p, kx, ky, halo=0.0, k_halo=1.0)
        alpha = rz / dot(p, ap)
        x = T(1.0) * x + T(alpha) * p
        r = T(1.0) * r + T(-alpha) * ap
        if math.sqrt(dot(r, r) / ff) <= tolerance:
            return x, iteration
        z = solve(r)
        rz_next = dot(r, z)
        p = T(1.0) * z + T(rz_next / rz) * p
        rz = rz_next
    raise AssertionError("the model has not converged")


@pytest.mark.parametrize("dtype", [F64, F32])
def test_the_preconditioner_does_something(dtype):
    kx, ky, f = pcg_problem(dtype)
    _, with_it = pcg_model(kx, ky, f, TOLERANCE[dtype])
    _, without = pcg_model(kx, ky, f, TOLERANCE[dtype], preconditioned=False)
    print(f"{dtype}: {with_it} iterations with the Jacobi preconditioner, {without} without")
    assert 4 * with_it < without, (with_it, without)
    # the order in which a dot is summed does not move the count
    for dot in (dot_fsum, dot_reversed):
        assert pcg_model(kx, ky, f, TOLERANCE[dtype], dot=dot)[1] == with_it, dot.__name__


# ------------------------------------------------------------------ the library without a device
def test_header_binding_and_symbols(built_lib):
    from stencilstream_amd import capi

    header = open(os.path.join(ROOT, "include", "ststhip.h")).read()
    for name in ("ststhip_grid_diffusion(", "ststhip_grid_diffusion_desc", "STSTHIP_DIFFUSION_APPLY 0u",
                 "STSTHIP_DIFFUSION_JACOBI 1u", "STSTHIP_DIFFUSION_SOLVE_DIAG 2u"):
        assert name in header, name
    for name in ("grid_diffusion", "grid_diffusion_desc"):
        assert callable(getattr(capi, name))
    assert (capi.DIFFUSION_APPLY, capi.DIFFUSION_JACOBI, capi.DIFFUSION_SOLVE_DIAG) == (APPLY, JACOBI, SOLVE_DIAG)
    raw = C.CDLL(os.path.join(ROOT, "stencilstream_amd", "libststhip.so"))
    assert hasattr(raw, NAME), f"libststhip.so lacks {NAME}"
    assert built_lib.ststhip_abi_version() == 6  # additive


def test_ctypes_struct_mirrors_the_c_struct(built_lib, tmp_path):
    from stencilstream_amd import capi

    c_name, mirror = "ststhip_grid_diffusion_desc", capi.GridDiffusionDesc
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
    assert len(want) == 1 + len(mirror._fields_) == 28


def view(base=BASE, stride=4, height=8, width=8, pitch=None):
    from stencilstream_amd import capi

    return capi.grid_view(base, stride, height, width, pitch)


def cells(offset=0, base=BASE, stride=32):
    """A member of the 32-byte cells of an 8 x 8 grid."""
    return view(base + offset, stride=stride)


SIDES = ("dst", "u", "kx", "ky", "rhs")
HOME = {"dst": BASE, "u": U_AT, "kx": KX_AT, "ky": KY_AT, "rhs": OTHER}


def entry(dtype=F32, mode=APPLY, n_rows=4, n_cols=4, **kw):
    """A valid operation on a 4 x 4 rectangle of 8 x 8 planes, each side a plane of its own; the arguments break it.
    dst=, u=, kx=, ky=, rhs= replace a view (rhs=True: a plane of its own); JACOBI and SOLVE_DIAG get a right-hand
    side unless rhs=None says otherwise."""
    from stencilstream_amd import capi

    changes = {k: kw.pop(k) for k in list(kw) if k in ("type", "reserved", "has_rhs")}
    stride = 4 if dtype == F32 else 8
    views = {side: kw.pop(side, view(HOME[side], stride)) for side in SIDES[:4]}
    rhs = kw.pop("rhs", mode != APPLY)
    if rhs is True:
        rhs = view(OTHER, stride)
    elif rhs is False:
        rhs = None
    d = capi.grid_diffusion_desc(views["dst"], views["u"], views["kx"], views["ky"], dtype, mode, n_rows, n_cols, rhs=rhs, **kw)
    for name, value in changes.items():
        setattr(d, name, value)
    return d


def per_side(what, make, sides=SIDES):
    """One case per side: make(side) -> keyword arguments of entry()."""
    return {f"{what}: {side}": (lambda side=side: [entry(**make(side))]) for side in sides}


def at(side, where):
    return {f"{side}_at": where, **({"rhs": True} if side == "rhs" else {})}


BAD = {
    "no entry": lambda: [],
    "nine entries": lambda: [entry()] * 9,
    "unknown type": lambda: [entry(type=2)],
    "unknown mode": lambda: [entry(mode=3, rhs=True)],
    "reserved set": lambda: [entry(reserved=1)],
    "a Jacobi step without a right-hand side": lambda: [entry(mode=JACOBI, rhs=None)],
    "a diagonal solve without a right-hand side": lambda: [entry(mode=SOLVE_DIAG, rhs=None)],
    "has_rhs without a view": lambda: [entry(has_rhs=1)],
    **per_side("stride 0", lambda s: {s: view(HOME[s], stride=0)}),
    **per_side("pitch below the width", lambda s: {s: view(HOME[s], pitch=7)}),
    **per_side("null base", lambda s: {s: view(0)}),
    **per_side("base off by two bytes", lambda s: {s: view(HOME[s] + 2)}),
    **per_side("f64 base off by four bytes", lambda s: {s: view(HOME[s] + 4, stride=8), "dtype": F64}),
    **per_side("stride no multiple of the element", lambda s: {s: view(HOME[s], stride=6)}),
    **per_side("f64 in twelve-byte cells", lambda s: {s: view(HOME[s], stride=12), "dtype": F64}),
    **per_side("extents past 2^63 bytes", lambda s: {s: view(HOME[s], height=2 ** 62, pitch=2 ** 20)}),
    **per_side("rows past the view", lambda s: at(s, (5, 0))),
    **per_side("columns past the view", lambda s: at(s, (0, 5))),
    **per_side("row past 2^64", lambda s: at(s, (2 ** 64 - 2, 0))),
    **per_side("a row of 2^31 bytes", lambda s: {s: view(HOME[s] + 2 ** 40 * SIDES.index(s), stride=2 ** 29)}),
    "2^31 rows": lambda: [entry(n_rows=2 ** 31, **{s: view(HOME[s] + 2 ** 50 * k, height=2 ** 32) for k, s in enumerate(SIDES[:4])})],
    "2^31 columns": lambda: [entry(n_cols=2 ** 31, **{s: view(HOME[s] + 2 ** 50 * k, width=2 ** 32) for k, s in enumerate(SIDES[:4])})],
    "2^31 rows of no columns": lambda: [entry(n_rows=2 ** 31, n_cols=0)],
    "an infinite sigma": lambda: [entry(sigma=INF)],
    "a NaN sigma in a diagonal solve": lambda: [entry(mode=SOLVE_DIAG, sigma=NAN)],
    "a NaN scale": lambda: [entry(scale=NAN)],
    "an infinite scale in a Jacobi step": lambda: [entry(mode=JACOBI, scale=-INF)],
    "an infinite rhs_coef": lambda: [entry(rhs=True, rhs_coef=-INF)],
    "a NaN rhs_coef in a diagonal solve": lambda: [entry(mode=SOLVE_DIAG, rhs_coef=NAN)],
    "a NaN omega in a Jacobi step": lambda: [entry(mode=JACOBI, omega=NAN)],
    "an infinite omega in a Jacobi step": lambda: [entry(mode=JACOBI, omega=INF)],
    **per_side("overlap: the destination itself", lambda s: {s: view()}, SIDES[1:4]),
    **per_side("overlap: the destination itself, on a member", lambda s: {"dst": cells(8), s: cells(8)}, SIDES[1:4]),
    **per_side("overlap: shifted by one element", lambda s: {**at(s, (0, 1)), s: view()}, SIDES[1:]),
    **per_side("overlap: shifted by one row", lambda s: {**at(s, (1, 0)), s: view()}, SIDES[1:]),
    # whole rows: the side's rectangle is rows 4 .. 7 of the destination's plane, the destination rows 0 .. 3; u and
    # ky read row 3 as the neighbour of row 4
    **per_side("overlap: the row above is read", lambda s: {**at(s, (4, 0)), s: view(), "n_cols": 8}, ("u", "ky")),
    # ... the other way round: u reads row 4 as the neighbour of row 3
    "overlap: the row below is read: u": lambda: [entry(u=view(), n_cols=8, dst_at=(4, 0))],
    # u's view begins four rows in front of the destination: its rectangle (rows 0 .. 3) ends where the destination
    # begins, but row 4 of the view is read as the neighbour of row 3
    "overlap: onto the row below the rectangle: u": lambda: [entry(n_cols=8, u=view(BASE - 4 * 8 * 4, height=8))],
    # one row of the destination's plane: the destination is columns 0 .. 3, the side's rectangle columns 4 .. 7; u and
    # kx read column 3 (ky does not: ACCEPTED has that case)
    **per_side("overlap: the column to the west is read", lambda s: {**at(s, (0, 4)), s: view(), "n_rows": 1}, ("u", "kx")),
    "overlap: another pitch": lambda: [entry(u=view(BASE, 4, 4, 8, 16))],
    **per_side("overlap: a member running into the next cell",
               lambda s: {"dst": cells(0, stride=8), s: cells(8, stride=8)}, SIDES[1:]),
    **per_side("overlap: a member of other cells", lambda s: {**at(s, (0, 1)), "dst": cells(8), s: cells(16)}, SIDES[1:]),
    "second entry bad": lambda: [entry(), entry(u_at=(5, 0))],
}


def call(built_lib, entries):
    from stencilstream_amd import capi

    table = (capi.GridDiffusionDesc * max(len(entries), 1))(*entries)
    return getattr(built_lib, NAME)(len(entries), table, None)


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_are_refused_before_the_device(built_lib, case):
    """STSTHIP_ERR_INVALID, not "no GPU" (4), on a machine without one: validation comes first."""
    from stencilstream_amd import capi

    status = call(built_lib, BAD[case]())
    assert status == INVALID, (status, capi.last_error())
    assert capi.last_error().startswith("grid diffusion"), capi.last_error()


def test_null_table_is_refused(built_lib):
    from stencilstream_amd import capi

    assert getattr(built_lib, NAME)(1, None, None) == INVALID
    assert capi.last_error().startswith("grid diffusion")


def test_the_wrappers_raise(built_lib):
    from stencilstream_amd import capi

    with pytest.raises(capi.StsthipError) as e:
        capi.grid_diffusion([entry(u_at=(5, 0))])
    assert e.value.status == INVALID
    with pytest.raises(ValueError):
        capi.grid_diffusion_desc(view(), view(U_AT), view(KX_AT), view(KY_AT), "<i4", APPLY, 4, 4)
    made = capi.grid_diffusion_desc(view(), None, view(KX_AT), view(KY_AT), F32, SOLVE_DIAG, 4, 4, rhs=view(OTHER))
    assert (made.mode, made.has_rhs, made.reserved, made.u.base, made.u.stride) == (SOLVE_DIAG, 1, 0, None, 0)
    assert (made.sigma, made.scale, made.omega, made.rhs_coef, made.halo, made.k_halo) == (0.0, 1.0, 1.0, 1.0, 0.0, 0.0)


def test_empty_rectangles_need_no_device(built_lib):
    """Nothing to compute: success on the host, also for null bases."""
    from stencilstream_amd import capi

    null = view(0)
    capi.grid_diffusion([entry(dst=null, u=null, kx=null, ky=null, n_rows=0), entry(n_cols=0),
                         entry(mode=JACOBI, dst=null, rhs=null, n_rows=0, n_cols=0),
                         entry(F64, SOLVE_DIAG, dst=view(0, stride=8), n_cols=0)])
    capi.grid_diffusion([entry(n_rows=0, u_at=(100, 100), kx_at=(9, 9))])  # an empty rectangle may start anywhere
    capi.grid_diffusion([entry(u=view(), kx=view(), n_rows=0)])  # ... and overlaps nothing


ACCEPTED = {
    "plain": lambda: [entry()],
    "doubles": lambda: [entry(F64)],
    "with a right-hand side": lambda: [entry(rhs=True, rhs_coef=0.25)],
    "a Jacobi step": lambda: [entry(mode=JACOBI, omega=0.8, sigma=1.0, scale=0.5)],
    "a diagonal solve": lambda: [entry(mode=SOLVE_DIAG)],
    # u is neither read nor validated there
    "a diagonal solve without u": lambda: [entry(mode=SOLVE_DIAG, u=view(0, stride=0)), entry(mode=SOLVE_DIAG, u=view(2, 3, 1, 1)),
                                           entry(mode=SOLVE_DIAG, u=view(), u_at=(100, 100))],
    "up to the last cell": lambda: [entry(dst_at=(4, 4), u_at=(4, 4), kx_at=(4, 4), ky_at=(4, 4))],
    "non-finite halos": lambda: [entry(halo=NAN, k_halo=INF), entry(mode=JACOBI, halo=-INF, k_halo=NAN)],
    "a non-finite rhs_coef or omega that is not read": lambda: [entry(rhs_coef=NAN, omega=NAN), entry(mode=SOLVE_DIAG, omega=INF)],
    "views of other extents": lambda: [entry(u=view(U_AT, height=5, width=6), u_at=(1, 2), kx=view(KX_AT, height=4, width=4),
                                             ky=view(KY_AT, height=9, width=4, pitch=12), ky_at=(5, 0))],
    "five members of one cell": lambda: [entry(mode=JACOBI, dst=cells(0), u=cells(4), kx=cells(8), ky=cells(12), rhs=cells(16))],
    "the members in front of the destination": lambda: [entry(dst=cells(28), u=cells(0), kx=cells(4), ky=cells(8))],
    "f64 members beside it": lambda: [entry(F64, dst=cells(0), u=cells(8), kx=cells(16), ky=cells(24))],
    "the right-hand side is the destination": lambda: [entry(rhs=view()), entry(mode=JACOBI, dst=cells(8), rhs=cells(8))],
    "the sources are one plane": lambda: [entry(mode=JACOBI, u=view(OTHER), kx=view(OTHER), ky=view(OTHER), rhs=view(OTHER))],
    # whole rows: kx and ky read nothing below their rectangle, kx nothing above it
    "beside what the faces do not read": lambda: [entry(kx=view(), n_cols=8, dst_at=(4, 0)), entry(ky=view(), n_cols=8, dst_at=(4, 0)),
                                                  entry(kx=view(), n_cols=8, kx_at=(4, 0))],
    # the same addresses as the refused case, but the view of u ends with the rectangle: row 4 is halo and is not read
    "beside what u does not read": lambda: [entry(n_cols=8, u=view(BASE - 4 * 8 * 4, height=4))],
    # one row: ky's rectangle begins right behind the destination's and reads nothing to its west
    "beside the column that ky does not read": lambda: [entry(ky=view(), ky_at=(0, 4), n_rows=1)],
    "apart by the one row that is read": lambda: [entry(u=view(), n_rows=3, n_cols=8, dst_at=(4, 0))],
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_a_valid_call_gets_as_far_as_the_device(built_lib, case):
    """Without a GPU a valid, non-empty call fails for want of a device: neither success nor a bad argument."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the made-up addresses must not reach it")
    for one in ACCEPTED[case]():
        assert call(built_lib, [one]) not in (0, INVALID)


def test_grid_method_refuses_bad_input(built_lib):
    from stencilstream_amd import update as U

    grid = U.Grid(6, 8, U.FDTD_CELL, device="cpu")  # (no call below gets as far as the cells)
    plane, u, kx, ky, f = (U.Grid(6, 8, "<f4", device="cpu") for _ in range(5))
    doubles = U.Grid(6, 8, "<f8", device="cpu")
    small = U.Grid(3, 4, "<f4", device="cpu")
    ints = U.Grid(6, 8, U.SELFCHECK_CELL, device="cpu")
    bad = [
        lambda: plane.diffusion(u, kx, ky, mode="relax"),
        lambda: plane.diffusion(u, kx, ky, mode=0),
        lambda: plane.diffusion(u, kx, ky, mode="jacobi"),  # no right-hand side
        lambda: plane.diffusion(None, kx, ky, mode="solve_diag"),
        lambda: plane.diffusion(None, kx, ky),  # only solve_diag reads no source
        lambda: plane.diffusion(None, kx, ky, mode="jacobi", rhs=f),
        lambda: plane.diffusion(None, kx, ky, mode="solve_diag", rhs=f, src_field="hz"),
        lambda: plane.diffusion(u, kx, ky, sigma=float("nan")),
        lambda: plane.diffusion(u, kx, ky, scale=float("inf")),
        lambda: plane.diffusion(u, kx, ky, rhs=f, rhs_coef=float("inf")),
        lambda: plane.diffusion(u, kx, ky, mode="jacobi", rhs=f, omega=float("nan")),
        lambda: plane.diffusion(plane, kx, ky),  # the destination itself
        lambda: plane.diffusion(u, plane, ky),
        lambda: plane.diffusion(u, kx, plane),
        lambda: grid.diffusion(grid, kx, ky, field="hz", src_field="hz"),
        lambda: grid.diffusion(u, kx, ky),  # no field of a structured cell
        lambda: grid.diffusion(u, kx, ky, field="pressure"),
        lambda: plane.diffusion(grid, kx, ky),  # the source names no field
        lambda: plane.diffusion(u, grid, ky, kx_field="pressure"),
        lambda: plane.diffusion(u, kx, grid),
        lambda: plane.diffusion(u, kx, ky, rhs=grid),
        lambda: plane.diffusion(doubles, kx, ky),  # another dtype
        lambda: plane.diffusion(u, doubles, ky),
        lambda: plane.diffusion(u, kx, doubles),
        lambda: plane.diffusion(u, kx, ky, rhs=doubles),
        lambda: plane.diffusion(u, kx, ky, rhs_field="hz"),  # no right-hand side to name a field of
        lambda: plane.diffusion(small, kx, ky),  # another extent
        lambda: plane.diffusion(u, small, ky),
        lambda: plane.diffusion(u, kx, small),
        lambda: plane.diffusion(u, kx, ky, rhs=small),
        lambda: plane.diffusion(u, kx, ky, rows=(0, 7)),
        lambda: plane.diffusion(u, kx, ky, cols=(5, 4)),
        lambda: ints.diffusion(u, kx, ky, field="status"),  # not a float
        lambda: plane.diffusion(u, kx, ky, field="hz"),  # plain cells have no fields
    ]
    for number, attempt in enumerate(bad):
        with pytest.raises(ValueError):
            attempt()
            pytest.fail(f"attempt {number} was accepted")
    with pytest.raises(TypeError):
        plane.diffusion(u, kx, ky, "jacobi")  # the mode is a keyword argument
    # an empty range is nothing, and needs no device
    plane.diffusion(u, kx, ky, rows=(2, 2))
    plane.diffusion(None, kx, ky, mode="solve_diag", rhs=plane, cols=(8, 8))
    grid.diffusion(grid, grid, grid, mode="jacobi", field="hz", src_field="hz_sum", kx_field="ex", ky_field="ey", rhs=grid,
                   rhs_field="hz", rows=(3, 3))

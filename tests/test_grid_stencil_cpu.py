"""ststhip_grid_stencil without a GPU: the header declares it and the library exports it, the ctypes mirror has the
layout of the C struct, every bad argument is refused before anything touches the device (status 2, "grid stencil ..."),
empty rectangles need no device, the overlap rules accept what they promise and nothing else, and
update.Grid.apply_stencil raises ValueError for bad input."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

INVALID = 2  # STSTHIP_ERR_INVALID
BASE, OTHER, THIRD = 0x100000, 0x900000, 0x1100000  # made-up addresses: nothing here reaches a device
F32, F64 = "<f4", "<f8"
CROSS5, BOX9 = 0, 1
NINE = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]
CROSS = [0.0, 0.2, 0.0, 0.4, 0.5, 0.6, -0.0, 0.8, 0.0]
NAME = "ststhip_grid_stencil"


def test_header_binding_and_symbols(built_lib):
    from stencilstream_amd import capi

    assert hasattr(capi, "grid_stencil"), "stencilstream_amd.capi has no grid_stencil"
    header = open(os.path.join(ROOT, "include", "ststhip.h")).read()
    for name in ("ststhip_grid_stencil(", "ststhip_grid_stencil_desc", "STSTHIP_STENCIL_CROSS5", "STSTHIP_STENCIL_BOX9"):
        assert name in header, name
    for name in ("grid_stencil", "grid_stencil_desc"):
        assert callable(getattr(capi, name))
    raw = C.CDLL(os.path.join(ROOT, "stencilstream_amd", "libststhip.so"))
    assert hasattr(raw, NAME), f"libststhip.so lacks {NAME}"
    assert built_lib.ststhip_abi_version() == 6  # additive
    assert (capi.STENCIL_CROSS5, capi.STENCIL_BOX9) == (CROSS5, BOX9)


def test_ctypes_struct_mirrors_the_c_struct(built_lib, tmp_path):
    from stencilstream_amd import capi

    c_name, mirror = "ststhip_grid_stencil_desc", capi.GridStencilDesc
    lines = ["#include <cstdio>", "#include <cstddef>", '#include "ststhip.h"', "int main() {",
             '    std::printf("shapes %u %u\\n", STSTHIP_STENCIL_CROSS5, STSTHIP_STENCIL_BOX9);',
             f'    std::printf("{c_name} %zu\\n", sizeof({c_name}));']
    for member, _ in mirror._fields_:
        lines.append(f'    std::printf("{c_name}.{member} %zu\\n", offsetof({c_name}, {member}));')
    lines.append("}")
    source = tmp_path / "layout.cpp"
    source.write_text("\n".join(lines) + "\n")
    program = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(source), "-o", str(program)], check=True)
    out = subprocess.run([str(program)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == f"shapes {capi.STENCIL_CROSS5} {capi.STENCIL_BOX9}"
    want = {key: int(value) for key, value in (line.split() for line in out[1:])}
    got = {c_name: C.sizeof(mirror)}
    for member, _ in mirror._fields_:
        got[f"{c_name}.{member}"] = getattr(mirror, member).offset
    assert got == want
    assert len(want) == 1 + len(mirror._fields_)
    assert mirror.weight.size == 9 * 8


def view(base=BASE, stride=4, height=8, width=8, pitch=None):
    from stencilstream_amd import capi

    return capi.grid_view(base, stride, height, width, pitch)


def cells(offset=0, base=BASE, stride=32):
    """A member of the 32-byte cells of an 8 x 8 grid."""
    return view(base + offset, stride=stride)


def stencil(dst=None, src=None, dtype=F32, shape=BOX9, weights=None, n_rows=4, n_cols=4, rhs=None, **kw):
    """A valid BOX9 stencil from one 8 x 8 plane into another over a 4 x 4 rectangle; the arguments break it."""
    from stencilstream_amd import capi

    changes = {k: kw.pop(k) for k in list(kw) if k in ("type", "reserved", "has_rhs")}
    if weights is None:
        weights = NINE if shape != CROSS5 else CROSS
    d = capi.grid_stencil_desc(view() if dst is None else dst, view(OTHER) if src is None else src, dtype, shape, weights,
                               n_rows, n_cols, rhs=rhs, **kw)
    for name, value in changes.items():
        setattr(d, name, value)
    return d


def with_weight(k, value, shape=BOX9, **kw):
    weights = list(NINE if shape == BOX9 else CROSS)
    weights[k] = value
    return stencil(shape=shape, weights=weights, **kw)


INF, NAN = float("inf"), float("nan")

BAD = {
    "no entry": lambda: [],
    "nine entries": lambda: [stencil()] * 9,
    "unknown type": lambda: [stencil(type=2)],
    "unknown shape": lambda: [stencil(shape=2)],
    "reserved set": lambda: [stencil(reserved=1)],
    "destination stride 0": lambda: [stencil(view(stride=0))],
    "source stride 0": lambda: [stencil(src=view(OTHER, stride=0))],
    "right-hand side stride 0": lambda: [stencil(rhs=view(THIRD, stride=0))],
    "destination pitch below the width": lambda: [stencil(view(pitch=7))],
    "source pitch below the width": lambda: [stencil(src=view(OTHER, pitch=7))],
    "right-hand side pitch below the width": lambda: [stencil(rhs=view(THIRD, pitch=7))],
    "null destination": lambda: [stencil(view(0))],
    "null source": lambda: [stencil(src=view(0))],
    "null right-hand side": lambda: [stencil(rhs=view(0))],
    "has_rhs without a view": lambda: [stencil(has_rhs=1)],
    "destination base off by two bytes": lambda: [stencil(view(BASE + 2))],
    "f64 source base off by four bytes": lambda: [stencil(view(stride=8), view(OTHER + 4, stride=8), F64)],
    "f64 right-hand side base off by four bytes": lambda: [stencil(view(stride=8), view(OTHER, stride=8), F64, rhs=view(THIRD + 4, stride=8))],
    "stride no multiple of the element": lambda: [stencil(view(stride=6))],
    "f64 in twelve-byte cells": lambda: [stencil(view(stride=12), view(OTHER, stride=8), F64)],
    "extents past 2^63 bytes": lambda: [stencil(src=view(OTHER, height=2 ** 62, pitch=2 ** 20))],
    "destination rows past the view": lambda: [stencil(dst_at=(5, 0))],
    "destination columns past the view": lambda: [stencil(dst_at=(0, 5))],
    "destination row past 2^64": lambda: [stencil(dst_at=(2 ** 64 - 2, 0))],
    "source rows past the view": lambda: [stencil(src_at=(5, 0))],
    "source columns past the view": lambda: [stencil(src_at=(0, 5))],
    "right-hand side rows past the view": lambda: [stencil(rhs=view(THIRD), rhs_at=(5, 0))],
    "right-hand side columns past the view": lambda: [stencil(rhs=view(THIRD), rhs_at=(0, 5))],
    "2^31 rows": lambda: [stencil(view(height=2 ** 32), view(OTHER + 2 ** 40, height=2 ** 32), n_rows=2 ** 31)],
    "2^31 columns": lambda: [stencil(view(width=2 ** 32), view(OTHER + 2 ** 40, width=2 ** 32), n_cols=2 ** 31)],
    "2^31 rows of no columns": lambda: [stencil(n_rows=2 ** 31, n_cols=0)],
    "a destination row of 2^31 bytes": lambda: [stencil(view(stride=2 ** 29))],
    "a source row of 2^31 bytes": lambda: [stencil(src=view(OTHER + 2 ** 40, stride=2 ** 29))],
    "a right-hand side row of 2^31 bytes": lambda: [stencil(rhs=view(OTHER + 2 ** 40, stride=2 ** 29))],
    "an infinite weight": lambda: [with_weight(4, INF)],
    "a NaN corner weight": lambda: [with_weight(8, NAN)],
    "a NaN weight of a cross": lambda: [with_weight(1, NAN, CROSS5)],
    "an infinite rhs_coef": lambda: [stencil(rhs=view(THIRD), rhs_coef=-INF)],
    "a NaN rhs_coef": lambda: [stencil(rhs=view(THIRD), rhs_coef=NAN)],
    "cross with a north-west weight": lambda: [with_weight(0, 0.5, CROSS5)],
    "cross with a north-east weight": lambda: [with_weight(2, 1e-300, CROSS5)],
    "cross with a south-west weight": lambda: [with_weight(6, -0.5, CROSS5)],
    "cross with a south-east weight": lambda: [with_weight(8, 0.5, CROSS5)],
    "overlap: in place": lambda: [stencil(src=view())],
    "overlap: in place on a member": lambda: [stencil(cells(8), cells(8))],
    "overlap: the source a column further": lambda: [stencil(src=view(), src_at=(0, 4), n_cols=3)],
    # the rectangles are disjoint, but column 3 of the source is read as the neighbour of column 4
    "overlap: the destination is a neighbour the source reads": lambda: [stencil(src=view(), src_at=(0, 4), dst_at=(0, 0), n_cols=4, n_rows=8)],
    "overlap: the destination is the row above the source": lambda: [stencil(src=view(), src_at=(4, 0), dst_at=(0, 0), n_rows=4, n_cols=8)],
    # the destination begins where row 4 of the source view does: outside the 4 x 8 rectangle, but read as its neighbour
    "overlap: onto the row below what the source view holds": lambda: [stencil(view(BASE + 4 * 8 * 4, height=4), view(BASE), n_rows=4, n_cols=8)],
    "overlap: a member running into the next cell": lambda: [stencil(cells(0, stride=8), cells(8, stride=8))],
    "overlap: an f64 member running into the next cell": lambda: [stencil(cells(0, stride=16), cells(16, stride=16), F64)],
    "overlap: a member of other cells": lambda: [stencil(cells(8), cells(16), src_at=(0, 1))],
    "overlap: member to member with another pitch": lambda: [stencil(view(BASE + 8, 32, 4, 8, 16), cells(16))],
    "overlap: the right-hand side shifted by one element": lambda: [stencil(rhs=view(), rhs_at=(0, 1))],
    "overlap: the right-hand side shifted by one row": lambda: [stencil(rhs=view(), rhs_at=(1, 0))],
    "overlap: the right-hand side in place but with another pitch": lambda: [stencil(rhs=view(BASE, 4, 4, 8, 16))],
    "overlap: the right-hand side a member of other cells": lambda: [stencil(cells(8), cells(8, OTHER), rhs=cells(16), rhs_at=(0, 1))],
    "second entry bad": lambda: [stencil(), stencil(dst_at=(5, 0))],
}


def call(built_lib, entries):
    from stencilstream_amd import capi

    table = (capi.GridStencilDesc * max(len(entries), 1))(*entries)
    return getattr(built_lib, NAME)(len(entries), table, None)


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_are_refused_before_the_device(built_lib, case):
    """STSTHIP_ERR_INVALID, not "no GPU" (4), on a machine without one: validation comes first."""
    from stencilstream_amd import capi

    status = call(built_lib, BAD[case]())
    assert status == INVALID, (status, capi.last_error())
    assert capi.last_error().startswith("grid stencil"), capi.last_error()


def test_null_table_is_refused(built_lib):
    from stencilstream_amd import capi

    assert getattr(built_lib, NAME)(1, None, None) == INVALID
    assert capi.last_error().startswith("grid stencil")


def test_the_wrappers_raise(built_lib):
    from stencilstream_amd import capi

    with pytest.raises(capi.StsthipError) as e:
        capi.grid_stencil([stencil(dst_at=(5, 0))])
    assert e.value.status == INVALID
    with pytest.raises(ValueError):
        capi.grid_stencil_desc(view(), view(OTHER), "<i4", BOX9, NINE, 4, 4)
    with pytest.raises(ValueError):
        capi.grid_stencil_desc(view(), view(OTHER), F32, BOX9, NINE[:8], 4, 4)
    nested = capi.grid_stencil_desc(view(), view(OTHER), F32, BOX9, [NINE[0:3], NINE[3:6], NINE[6:9]], 4, 4)
    assert list(nested.weight) == NINE and nested.has_rhs == 0 and nested.reserved == 0


def test_empty_rectangles_need_no_device(built_lib):
    """Nothing to compute: success on the host, also for null bases."""
    from stencilstream_amd import capi

    null = view(0)
    capi.grid_stencil([stencil(null, null, n_rows=0), stencil(n_cols=0), stencil(null, null, rhs=null, n_rows=0, n_cols=0),
                       stencil(null, null, shape=CROSS5, n_cols=0)])
    capi.grid_stencil([stencil(n_rows=0, dst_at=(100, 100), src_at=(50, 0))])  # an empty rectangle may start anywhere
    capi.grid_stencil([stencil(src=view(), n_rows=0)])  # ... and overlaps nothing


ACCEPTED = {
    "box": lambda: [stencil()],
    "cross": lambda: [stencil(shape=CROSS5)],
    "cross with corners of either zero": lambda: [stencil(shape=CROSS5, weights=[-0.0, 1, 0.0, 1, 1, 1, 0.0, 1, -0.0])],
    "doubles": lambda: [stencil(view(stride=8), view(OTHER, stride=8), F64)],
    "up to the last cell": lambda: [stencil(dst_at=(4, 4), src_at=(4, 4))],
    "a non-finite halo": lambda: [stencil(halo=NAN), stencil(halo=-INF)],
    "with a right-hand side": lambda: [stencil(rhs=view(THIRD), rhs_coef=0.25)],
    "a non-finite rhs_coef that is not used": lambda: [stencil(rhs_coef=NAN)],
    "the source another member of the destination's cells": lambda: [stencil(cells(8), cells(16))],
    "the member in front of it": lambda: [stencil(cells(0), cells(28))],
    "an f64 member beside it": lambda: [stencil(cells(0, stride=16), cells(8, stride=16), F64)],
    "the right-hand side is the destination": lambda: [stencil(rhs=view())],
    "the right-hand side is the destination, on an inner rectangle": lambda: [stencil(dst_at=(2, 3), rhs=view(), rhs_at=(2, 3))],
    "the right-hand side is the destination's member": lambda: [stencil(cells(8), cells(8, OTHER), rhs=cells(8))],
    "the right-hand side another member": lambda: [stencil(cells(8), cells(8, OTHER), rhs=cells(16))],
    "source and right-hand side both members of the destination's cells": lambda: [stencil(cells(8), cells(16), rhs=cells(0))],
    "the right-hand side is the source": lambda: [stencil(rhs=view(OTHER))],
    # rows 0..2 written, rows 4..6 the centre taps: row 3 is read and is not the destination's
    "apart by the one row the stencil reads": lambda: [stencil(src=view(), src_at=(4, 0), n_rows=3, n_cols=8)],
    # the same addresses as the refused case, but the source view ends with the rectangle: row 4 is halo and is not read
    "beside what it does not read": lambda: [stencil(view(BASE + 4 * 8 * 4, height=4), view(BASE, height=4), n_rows=4, n_cols=8)],
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
    box = [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]]
    cross = (0.25, 0.25, 0.0, 0.25, 0.25)
    bad = [
        lambda: plane.apply_stencil(other),  # neither box nor cross
        lambda: plane.apply_stencil(other, box=box, cross=cross),  # both
        lambda: plane.apply_stencil(other, box=NINE),  # not 3 x 3
        lambda: plane.apply_stencil(other, box=[[1, 2], [3, 4]]),
        lambda: plane.apply_stencil(other, cross=(1, 2, 3, 4)),
        lambda: plane.apply_stencil(other, cross=box),
        lambda: plane.apply_stencil(other, cross=(1, 2, float("nan"), 4, 5)),
        lambda: plane.apply_stencil(other, box=[[1, 2, 3], [4, float("inf"), 6], [7, 8, 9]]),
        lambda: plane.apply_stencil(other, cross=cross, rhs=other, rhs_coef=float("inf")),
        lambda: plane.apply_stencil(plane, cross=cross),  # in place
        lambda: grid.apply_stencil(grid, cross=cross, field="temp", src_field="temp"),
        lambda: grid.apply_stencil(plane, cross=cross),  # no field of a structured cell
        lambda: grid.apply_stencil(plane, cross=cross, field="pressure"),
        lambda: grid.apply_stencil(same, cross=cross, field="temp"),  # the source names no field
        lambda: grid.apply_stencil(same, cross=cross, field="temp", src_field="ez"),
        lambda: grid.apply_stencil(doubles, cross=cross, field="temp", src_field="temp"),  # another dtype
        lambda: grid.apply_stencil(plane, cross=cross, field="temp", rhs=doubles, rhs_field="power"),
        lambda: grid.apply_stencil(plane, cross=cross, field="temp", rhs=same),
        lambda: grid.apply_stencil(plane, cross=cross, field="temp", rhs_field="power"),  # no right-hand side to name a field of
        lambda: plane.apply_stencil(small, cross=cross),  # another extent
        lambda: plane.apply_stencil(other, cross=cross, rhs=small),
        lambda: plane.apply_stencil(other, cross=cross, rows=(0, 7)),
        lambda: plane.apply_stencil(other, cross=cross, cols=(5, 4)),
        lambda: ints.apply_stencil(ints, cross=cross, field="status", src_field="r"),  # not a float
        lambda: plane.apply_stencil(other, cross=cross, field="temp"),  # plain cells have no fields
    ]
    for number, attempt in enumerate(bad):
        with pytest.raises(ValueError):
            attempt()
            pytest.fail(f"attempt {number} was accepted")
    with pytest.raises(TypeError):
        plane.apply_stencil(other, box)  # the weights are keyword arguments
    # an empty range is nothing, and needs no device
    plane.apply_stencil(other, box=box, rows=(2, 2))
    plane.apply_stencil(other, cross=cross, rhs=plane, cols=(8, 8))

"""ststhip_grid_combine / ststhip_grid_resample without a GPU: the header declares them and the library exports them,
the ctypes mirrors have the layout of the C structs, every bad argument is refused before anything touches the device
(status 2, "grid algebra ..."), empty rectangles need no device, the overlap rules accept what they promise and nothing
else, and update.Grid's methods raise ValueError for bad input."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INVALID = 2  # STSTHIP_ERR_INVALID
BASE, OTHER, THIRD = 0x100000, 0x900000, 0x1100000  # made-up addresses: nothing here reaches a device
F32, F64 = "<f4", "<f8"
RESTRICT, PROLONG = 0, 1


def test_header_binding_and_symbols(built_lib):
    from stencilstream_amd import capi

    header = open(os.path.join(ROOT, "include", "ststhip.h")).read()
    for name in ("ststhip_grid_combine(", "ststhip_grid_resample(", "ststhip_grid_combine_desc", "ststhip_grid_term",
                 "ststhip_grid_resample_desc", "STSTHIP_RESTRICT_MEAN", "STSTHIP_PROLONG_BILINEAR"):
        assert name in header, name
    assert "operation by operation" in header.lower()
    for name in ("grid_combine", "grid_resample", "grid_combine_desc", "grid_resample_desc"):
        assert callable(getattr(capi, name))
    raw = C.CDLL(os.path.join(ROOT, "stencilstream_amd", "libststhip.so"))
    for name in ("ststhip_grid_combine", "ststhip_grid_resample"):
        assert hasattr(raw, name), f"libststhip.so lacks {name}"
    assert built_lib.ststhip_abi_version() == 6  # additive
    assert (capi.RESTRICT_MEAN, capi.PROLONG_BILINEAR) == (RESTRICT, PROLONG)


def test_ctypes_structs_mirror_the_c_structs(built_lib, tmp_path):
    from stencilstream_amd import capi

    names = {"ststhip_grid_term": capi.GridTerm, "ststhip_grid_combine_desc": capi.GridCombineDesc,
             "ststhip_grid_resample_desc": capi.GridResampleDesc}
    lines = ["#include <cstdio>", "#include <cstddef>", '#include "ststhip.h"', "int main() {",
             '    std::printf("modes %u %u\\n", STSTHIP_RESTRICT_MEAN, STSTHIP_PROLONG_BILINEAR);']
    for c_name, mirror in names.items():
        lines.append(f'    std::printf("{c_name} %zu\\n", sizeof({c_name}));')
        for member, _ in mirror._fields_:
            lines.append(f'    std::printf("{c_name}.{member} %zu\\n", offsetof({c_name}, {member}));')
    lines.append("}")
    source = tmp_path / "layout.cpp"
    source.write_text("\n".join(lines) + "\n")
    program = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(source), "-o", str(program)], check=True)
    out = subprocess.run([str(program)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == f"modes {capi.RESTRICT_MEAN} {capi.PROLONG_BILINEAR}"
    want = {key: int(value) for key, value in (line.split() for line in out[1:])}
    got = {}
    for c_name, mirror in names.items():
        got[c_name] = C.sizeof(mirror)
        for member, _ in mirror._fields_:
            got[f"{c_name}.{member}"] = getattr(mirror, member).offset
    assert got == want
    assert len(want) == 3 + sum(len(m._fields_) for m in names.values())


def view(base=BASE, stride=4, height=8, width=8, pitch=None):
    from stencilstream_amd import capi

    return capi.grid_view(base, stride, height, width, pitch)


def cells(offset=0, base=BASE, stride=32):
    """A member of the 32-byte cells of an 8 x 8 grid."""
    return view(base + offset, stride=stride)


def combine(dst=None, terms=None, dtype=F32, n_rows=4, n_cols=4, dst_at=(0, 0), **changes):
    """A valid combine of two planes into a third over a 4 x 4 rectangle of 8 x 8 planes; the arguments break it."""
    from stencilstream_amd import capi

    terms = [(1.0, view(OTHER)), (0.5, view(THIRD))] if terms is None else terms
    c = capi.grid_combine_desc(view() if dst is None else dst, dtype, terms, n_rows, n_cols, dst_at)
    for name, value in changes.items():
        setattr(c, name, value)
    return c


def resample(dst=None, src=None, dtype=F32, mode=RESTRICT, n_rows=4, n_cols=4, **kw):
    """A valid transfer between an 8 x 8 and a 4 x 4 plane (restrict: dst coarse; prolong: dst fine)."""
    from stencilstream_amd import capi

    changes = {k: kw.pop(k) for k in list(kw) if k in ("type",)}
    if dst is None:
        dst = view(height=4, width=4) if mode == RESTRICT else view()
    if src is None:
        src = view(OTHER) if mode == RESTRICT else view(OTHER, height=4, width=4)
    r = capi.grid_resample_desc(dst, src, dtype, mode, n_rows, n_cols, **kw)
    for name, value in changes.items():
        setattr(r, name, value)
    return r


COMBINE, RESAMPLE = "ststhip_grid_combine", "ststhip_grid_resample"

# name -> (entry point, entries)
BAD = {
    "combine: no entry": lambda: (COMBINE, []),
    "combine: nine entries": lambda: (COMBINE, [combine()] * 9),
    "resample: no entry": lambda: (RESAMPLE, []),
    "resample: nine entries": lambda: (RESAMPLE, [resample()] * 9),
    "combine: no term": lambda: (COMBINE, [combine(terms=[])]),
    "combine: five terms": lambda: (COMBINE, [combine(terms=[(1.0, view(OTHER))] * 5)]),
    "combine: unknown type": lambda: (COMBINE, [combine(type=2)]),
    "resample: unknown type": lambda: (RESAMPLE, [resample(type=7)]),
    "resample: unknown mode": lambda: (RESAMPLE, [resample(mode=2, dst=view(), src=view(OTHER))]),
    "combine: destination stride 0": lambda: (COMBINE, [combine(view(stride=0))]),
    "combine: term stride 0": lambda: (COMBINE, [combine(terms=[(1.0, view(OTHER)), (1.0, view(THIRD, stride=0))])]),
    "resample: destination stride 0": lambda: (RESAMPLE, [resample(view(stride=0, height=4, width=4))]),
    "resample: source stride 0": lambda: (RESAMPLE, [resample(src=view(OTHER, stride=0))]),
    "combine: destination pitch below the width": lambda: (COMBINE, [combine(view(pitch=7))]),
    "combine: term pitch below the width": lambda: (COMBINE, [combine(terms=[(1.0, view(OTHER, pitch=7))])]),
    "resample: source pitch below the width": lambda: (RESAMPLE, [resample(src=view(OTHER, pitch=7))]),
    "resample: destination pitch below the width": lambda: (RESAMPLE, [resample(mode=PROLONG, dst=view(pitch=7))]),
    "combine: null destination": lambda: (COMBINE, [combine(view(0))]),
    "combine: null term": lambda: (COMBINE, [combine(terms=[(1.0, view(OTHER)), (1.0, view(0))])]),
    "resample: null destination": lambda: (RESAMPLE, [resample(view(0, height=4, width=4))]),
    "resample: null source": lambda: (RESAMPLE, [resample(src=view(0))]),
    "combine: destination base off by two bytes": lambda: (COMBINE, [combine(view(BASE + 2))]),
    "combine: f64 term base off by four bytes": lambda: (COMBINE, [combine(view(stride=8), [(1.0, view(OTHER + 4, stride=8))], F64)]),
    "combine: stride no multiple of the element": lambda: (COMBINE, [combine(view(stride=6))]),
    "combine: f64 in twelve-byte cells": lambda: (COMBINE, [combine(view(stride=12), [(1.0, view(OTHER, stride=8))], F64)]),
    "resample: source base off by one byte": lambda: (RESAMPLE, [resample(src=view(OTHER + 1))]),
    "resample: f64 destination stride 4": lambda: (RESAMPLE, [resample(src=view(OTHER, stride=8), dtype=F64)]),
    "combine: extents past 2^63 bytes": lambda: (COMBINE, [combine(terms=[(1.0, view(OTHER, height=2 ** 62, pitch=2 ** 20))])]),
    "resample: extents past 2^63 bytes": lambda: (RESAMPLE, [resample(src=view(OTHER, height=2 ** 62, pitch=2 ** 20))]),
    "combine: destination rows past the view": lambda: (COMBINE, [combine(dst_at=(5, 0))]),
    "combine: destination columns past the view": lambda: (COMBINE, [combine(dst_at=(0, 5))]),
    "combine: destination row past 2^64": lambda: (COMBINE, [combine(dst_at=(2 ** 64 - 2, 0))]),
    "combine: term rows past the view": lambda: (COMBINE, [combine(terms=[(1.0, view(OTHER), (5, 0))])]),
    "combine: second term columns past the view": lambda: (COMBINE, [combine(terms=[(1.0, view(OTHER)), (1.0, view(THIRD), (0, 5))])]),
    "restrict: source past the view": lambda: (RESAMPLE, [resample(src_at=(1, 0))]),
    "restrict: source columns past the view": lambda: (RESAMPLE, [resample(src_at=(0, 1))]),
    "restrict: destination past the view": lambda: (RESAMPLE, [resample(dst_at=(0, 1))]),
    "prolong: destination past the view": lambda: (RESAMPLE, [resample(mode=PROLONG, dst_at=(1, 0))]),
    "prolong: source past the view": lambda: (RESAMPLE, [resample(mode=PROLONG, src_at=(0, 1))]),
    "prolong: fine side counted once only": lambda: (RESAMPLE, [resample(mode=PROLONG, dst=view(height=4, width=8))]),
    "combine: 2^31 rows": lambda: (COMBINE, [combine(view(height=2 ** 32), [(1.0, view(OTHER, height=2 ** 32))], n_rows=2 ** 31)]),
    "combine: 2^31 columns": lambda: (COMBINE, [combine(view(width=2 ** 32), [(1.0, view(OTHER + 2 ** 40, width=2 ** 32))], n_cols=2 ** 31)]),
    "combine: 2^31 rows of no columns": lambda: (COMBINE, [combine(n_rows=2 ** 31, n_cols=0)]),
    "resample: 2^30 coarse rows": lambda: (RESAMPLE, [resample(view(height=2 ** 32, width=4), view(OTHER + 2 ** 40, height=2 ** 33), n_rows=2 ** 30)]),
    "combine: a destination row of 2^31 bytes": lambda: (COMBINE, [combine(view(stride=2 ** 29))]),
    "combine: a term row of 2^31 bytes": lambda: (COMBINE, [combine(terms=[(1.0, view(OTHER + 2 ** 40, stride=2 ** 29))])]),
    "restrict: a fine row of 2^31 bytes": lambda: (RESAMPLE, [resample(src=view(OTHER + 2 ** 40, stride=2 ** 28))]),
    "prolong: a fine row of 2^31 bytes": lambda: (RESAMPLE, [resample(mode=PROLONG, dst=view(OTHER + 2 ** 40, stride=2 ** 28), src=view(height=4, width=4))]),
    "overlap: a term shifted by one element": lambda: (COMBINE, [combine(terms=[(1.0, view(), (0, 1))])]),
    "overlap: a term shifted by one row": lambda: (COMBINE, [combine(terms=[(1.0, view(OTHER)), (1.0, view(), (1, 0))])]),
    "overlap: in place but with another pitch": lambda: (COMBINE, [combine(terms=[(1.0, view(BASE, 4, 4, 8, 16))])]),
    "overlap: in place but with another stride": lambda: (COMBINE, [combine(view(stride=8), [(1.0, view(BASE, 4, 8, 16))])]),
    "overlap: a member running into the next cell": lambda: (COMBINE, [combine(cells(0, stride=8), [(1.0, cells(8, stride=8))])]),
    "overlap: an f64 member running into the next cell": lambda: (COMBINE, [combine(cells(0, stride=16), [(1.0, cells(16, stride=16))], F64)]),
    "overlap: a member of other cells": lambda: (COMBINE, [combine(cells(8), [(1.0, cells(16), (0, 1))])]),
    "overlap: member to member with another pitch": lambda: (COMBINE, [combine(view(BASE + 8, 32, 4, 8, 16), [(1.0, cells(16))])]),
    "overlap: rectangles whose spans interleave": lambda: (COMBINE, [combine(terms=[(1.0, view(), (0, 4))])]),
    "overlap: restrict in place": lambda: (RESAMPLE, [resample(view(height=4, width=4), view())]),
    "overlap: restrict into a member of the same cells": lambda: (RESAMPLE, [resample(cells(8), cells(16))]),
    "overlap: restrict into a corner of the source": lambda: (RESAMPLE, [resample(view(), view(), n_rows=2, n_cols=2, dst_at=(6, 6), src_at=(4, 4))]),
    "overlap: prolong in place": lambda: (RESAMPLE, [resample(mode=PROLONG, src=view(height=4, width=4))]),
    # the destination begins where row 4 of the source view does: outside the 4 x 4 rectangle, but read as its neighbour
    "overlap: prolong onto a neighbour it reads": lambda: (
        RESAMPLE, [resample(mode=PROLONG, dst=view(BASE + 4 * 8 * 4), src=view(BASE, height=8, width=8))]),
    "combine: second entry bad": lambda: (COMBINE, [combine(), combine(dst_at=(5, 0))]),
    "resample: second entry bad": lambda: (RESAMPLE, [resample(), resample(mode=3)]),
}


def call(built_lib, name, entries):
    from stencilstream_amd import capi

    kind = capi.GridCombineDesc if name == COMBINE else capi.GridResampleDesc
    table = (kind * max(len(entries), 1))(*entries)
    return getattr(built_lib, name)(len(entries), table, None)


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_are_refused_before_the_device(built_lib, case):
    """STSTHIP_ERR_INVALID, not "no GPU" (4), on a machine without one: validation comes first."""
    from stencilstream_amd import capi

    name, entries = BAD[case]()
    status = call(built_lib, name, entries)
    assert status == INVALID, (status, capi.last_error())
    assert capi.last_error().startswith("grid algebra"), capi.last_error()


def test_null_table_is_refused(built_lib):
    from stencilstream_amd import capi

    for name in (COMBINE, RESAMPLE):
        assert getattr(built_lib, name)(1, None, None) == INVALID
        assert capi.last_error().startswith("grid algebra")


def test_the_wrappers_raise(built_lib):
    from stencilstream_amd import capi

    for wrapper, entry in ((capi.grid_combine, combine(dst_at=(5, 0))), (capi.grid_resample, resample(src_at=(1, 0)))):
        with pytest.raises(capi.StsthipError) as e:
            wrapper([entry])
        assert e.value.status == INVALID
    with pytest.raises(ValueError):
        capi.grid_combine_desc(view(), "<i4", [(1.0, view(OTHER))], 4, 4)
    with pytest.raises(ValueError):
        capi.grid_resample_desc(view(), view(OTHER), "<f2", RESTRICT, 4, 4)


def test_empty_rectangles_need_no_device(built_lib):
    """Nothing to compute: success on the host, also for null bases."""
    from stencilstream_amd import capi

    null = view(0)
    capi.grid_combine([combine(null, [(1.0, null), (2.0, null)], n_rows=0), combine(n_cols=0),
                       combine(null, [(1.0, null)], n_rows=0, n_cols=0)])
    capi.grid_resample([resample(null, null, n_rows=0), resample(n_cols=0), resample(null, null, mode=PROLONG, n_cols=0)])
    # an empty rectangle may start anywhere
    capi.grid_combine([combine(n_rows=0, dst_at=(100, 100))])
    capi.grid_resample([resample(n_cols=0, src_at=(100, 0))])


ACCEPTED = {
    "combine": lambda: (COMBINE, [combine()]),
    "combine of four terms": lambda: (COMBINE, [combine(terms=[(1.0, view(OTHER)), (2.0, view(THIRD)), (3.0, view(OTHER)), (4.0, view(THIRD))])]),
    "combine up to the last cell": lambda: (COMBINE, [combine(dst_at=(4, 4), terms=[(1.0, view(OTHER), (4, 4))])]),
    "in place": lambda: (COMBINE, [combine(terms=[(0.5, view()), (1.0, view(OTHER))])]),
    "in place on an inner rectangle": lambda: (COMBINE, [combine(dst_at=(2, 3), terms=[(0.5, view(), (2, 3))])]),
    "in place on a member": lambda: (COMBINE, [combine(cells(8), [(2.0, cells(8))])]),
    "another member of the same cells": lambda: (COMBINE, [combine(cells(8), [(1.0, cells(16)), (1.0, cells(8))])]),
    "the member in front of it": lambda: (COMBINE, [combine(cells(0), [(1.0, cells(28))])]),
    "an f64 member beside it": lambda: (COMBINE, [combine(cells(0, stride=16), [(1.0, cells(8, stride=16))], F64)]),
    "disjoint rectangles of one plane": lambda: (COMBINE, [combine(dst_at=(4, 0), terms=[(1.0, view())])]),
    "terms that overlap each other": lambda: (COMBINE, [combine(terms=[(1.0, view(OTHER)), (1.0, view(OTHER), (0, 1))])]),
    "restrict": lambda: (RESAMPLE, [resample()]),
    "restrict from an odd row and column": lambda: (RESAMPLE, [resample(n_rows=3, n_cols=3, src_at=(1, 1))]),
    "prolong": lambda: (RESAMPLE, [resample(mode=PROLONG)]),
    # the same addresses, but the source view ends with the rectangle: row 4 is halo and is not read
    "prolong beside what it does not read": lambda: (
        RESAMPLE, [resample(mode=PROLONG, dst=view(BASE + 4 * 8 * 4), src=view(BASE, height=4, width=8))]),
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_a_valid_call_gets_as_far_as_the_device(built_lib, case):
    """Without a GPU a valid, non-empty call fails for want of a device: neither success nor a bad argument."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the made-up addresses must not reach it")
    name, entries = ACCEPTED[case]()
    assert call(built_lib, name, entries) not in (0, INVALID)


def test_grid_methods_refuse_bad_input(built_lib):
    from stencilstream_amd import update as U

    grid = U.Grid(6, 8, U.HOTSPOT_CELL, device="cpu")  # (no call below gets as far as the cells)
    same = U.Grid(6, 8, U.FDTD_CELL, device="cpu")
    plane = U.Grid(6, 8, "<f4", device="cpu")
    doubles = U.Grid(6, 8, U.HOTSPOT_CELL_F64, device="cpu")
    small = U.Grid(3, 4, "<f4", device="cpu")
    odd = U.Grid(3, 5, "<f4", device="cpu")
    ints = U.Grid(6, 8, U.SELFCHECK_CELL, device="cpu")
    bad = [
        lambda: grid.combine([(1.0, plane)]),  # no field of a structured cell
        lambda: grid.combine([(1.0, plane)], field="pressure"),
        lambda: grid.combine([], field="temp"),
        lambda: grid.combine([(1.0, plane)] * 5, field="temp"),
        lambda: grid.combine([(1.0, plane, None, 4)], field="temp"),
        lambda: grid.combine([(1.0, same)], field="temp"),  # the term names no field
        lambda: grid.combine([(1.0, same, "ez")], field="temp"),
        lambda: grid.combine([(1.0, doubles, "temp")], field="temp"),  # another dtype
        lambda: grid.combine([(1.0, small)], field="temp"),  # another extent
        lambda: grid.combine([(1.0, plane)], field="temp", rows=(0, 7)),
        lambda: grid.combine([(1.0, plane)], field="temp", cols=(5, 4)),
        lambda: ints.combine([(1.0, ints, "status")], field="status"),  # not a float
        lambda: plane.combine([(1.0, plane)], field="temp"),  # plain cells have no fields
        lambda: small.restrict_from(grid),
        lambda: small.restrict_from(grid, src_field="heat"),
        lambda: small.restrict_from(doubles, src_field="temp"),
        lambda: odd.restrict_from(plane),
        lambda: small.restrict_from(small),
        lambda: plane.restrict_from(small),  # the wrong way round
        lambda: plane.prolong_from(odd),
        lambda: plane.prolong_from(grid),
        lambda: grid.prolong_from(small),
        lambda: doubles.prolong_from(small, field="temp"),
        lambda: small.prolong_from(plane),  # the wrong way round
        lambda: ints.prolong_from(small, field="r"),
    ]
    for number, attempt in enumerate(bad):
        with pytest.raises(ValueError):
            attempt()
            pytest.fail(f"attempt {number} was accepted")

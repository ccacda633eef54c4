"""ststhip_grid_copy / _fill / _download / _upload without a GPU: the library exports them, the ctypes mirrors have the
layout of the C structs, every bad argument is refused before anything touches the device, empty rectangles need no
device, and update.Grid's region methods refuse ranges outside the grid."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INVALID = 2  # STSTHIP_ERR_INVALID
BASE, OTHER = 0x100000, 0x900000  # made-up addresses: nothing here reaches a device


def test_binding_and_symbols(built_lib):
    from stencilstream_amd import capi

    for name in ("grid_view", "grid_copy", "grid_fill", "grid_download", "grid_upload"):
        assert callable(getattr(capi, name))
    raw = C.CDLL(os.path.join(ROOT, "stencilstream_amd", "libststhip.so"))
    for name in ("ststhip_grid_copy", "ststhip_grid_fill", "ststhip_grid_download", "ststhip_grid_upload"):
        assert hasattr(raw, name), f"libststhip.so lacks {name}"
    assert built_lib.ststhip_abi_version() == 6  # additive


def test_ctypes_structs_mirror_the_c_structs(built_lib, tmp_path):
    from stencilstream_amd import capi

    names = {"ststhip_grid_view": capi.GridView, "ststhip_grid_copy_desc": capi.GridCopyDesc,
             "ststhip_grid_fill_desc": capi.GridFillDesc}
    lines = ["#include <cstdio>", "#include <cstddef>", '#include "ststhip.h"', "int main() {"]
    for c_name, mirror in names.items():
        lines.append(f'    std::printf("{c_name} %zu\\n", sizeof({c_name}));')
        for member, _ in mirror._fields_:
            lines.append(f'    std::printf("{c_name}.{member} %zu\\n", offsetof({c_name}, {member}));')
    lines.append("}")
    source = tmp_path / "layout.cpp"
    source.write_text("\n".join(lines) + "\n")
    program = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(source), "-o", str(program)], check=True)
    out = subprocess.run([str(program)], check=True, capture_output=True, text=True).stdout
    want = {key: int(value) for key, value in (line.split() for line in out.splitlines())}
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


def copy(dst=None, src=None, elem_size=4, n_rows=4, n_cols=4, **changes):
    """A valid copy of a 4 x 4 rectangle between two 8 x 8 planes of 4-byte elements; `changes` break it."""
    from stencilstream_amd import capi

    c = capi.grid_copy_desc(view() if dst is None else dst, view(OTHER) if src is None else src, elem_size, n_rows, n_cols)
    for name, value in changes.items():
        setattr(c, name, value)
    return c


def fill(dst=None, value=b"\0\0\0\0", n_rows=4, n_cols=4, **changes):
    from stencilstream_amd import capi

    f = capi.grid_fill_desc(view() if dst is None else dst, bytes(4) if value is None else value, n_rows, n_cols)
    if value is None:
        f.value = None
    for name, changed in changes.items():
        setattr(f, name, changed)
    return f


def cells(offset=0, base=BASE):
    """A member of the 32-byte cells of an 8 x 8 grid."""
    return view(base + offset, stride=32)


# name -> (entry point, entries)
BAD = {
    "copy: no entry": lambda: ("ststhip_grid_copy", []),
    "copy: nine entries": lambda: ("ststhip_grid_copy", [copy()] * 9),
    "fill: no entry": lambda: ("ststhip_grid_fill", []),
    "fill: nine entries": lambda: ("ststhip_grid_fill", [fill()] * 9),
    "download: nine entries": lambda: ("ststhip_grid_download", [copy()] * 9),
    "upload: no entry": lambda: ("ststhip_grid_upload", []),
    "copy: elem_size 0": lambda: ("ststhip_grid_copy", [copy(elem_size=0)]),
    "copy: elem_size 129": lambda: ("ststhip_grid_copy", [copy(view(stride=256), view(OTHER, stride=256), elem_size=129)]),
    "fill: elem_size 129": lambda: ("ststhip_grid_fill", [fill(view(stride=256), value=bytes(129))]),
    "copy: elem_size above the destination's stride": lambda: ("ststhip_grid_copy", [copy(src=view(OTHER, stride=8), elem_size=8)]),
    "copy: elem_size above the source's stride": lambda: ("ststhip_grid_copy", [copy(dst=view(stride=8), elem_size=8)]),
    "fill: elem_size above the stride": lambda: ("ststhip_grid_fill", [fill(value=bytes(8))]),
    "copy: destination stride 0": lambda: ("ststhip_grid_copy", [copy(dst=view(stride=0))]),
    "copy: source stride 0": lambda: ("ststhip_grid_copy", [copy(src=view(OTHER, stride=0))]),
    "fill: stride 0": lambda: ("ststhip_grid_fill", [fill(view(stride=0))]),
    "copy: destination pitch below the width": lambda: ("ststhip_grid_copy", [copy(dst=view(pitch=7))]),
    "copy: source pitch below the width": lambda: ("ststhip_grid_copy", [copy(src=view(OTHER, pitch=7))]),
    "fill: pitch below the width": lambda: ("ststhip_grid_fill", [fill(view(pitch=7))]),
    "copy: row step 0": lambda: ("ststhip_grid_copy", [copy(src_row_step=0)]),
    "copy: column step 0": lambda: ("ststhip_grid_copy", [copy(src_col_step=0)]),
    "download: column step 0": lambda: ("ststhip_grid_download", [copy(src_col_step=0)]),
    "copy: null destination": lambda: ("ststhip_grid_copy", [copy(dst=view(0))]),
    "copy: null source": lambda: ("ststhip_grid_copy", [copy(src=view(0))]),
    "fill: null destination": lambda: ("ststhip_grid_fill", [fill(view(0))]),
    "download: null host memory": lambda: ("ststhip_grid_download", [copy(dst=view(0))]),
    "upload: null host memory": lambda: ("ststhip_grid_upload", [copy(src=view(0))]),
    "fill: null value": lambda: ("ststhip_grid_fill", [fill(value=None)]),
    "fill: null value of an empty rectangle": lambda: ("ststhip_grid_fill", [fill(value=None, n_rows=0)]),
    "copy: extents past 2^63 bytes": lambda: ("ststhip_grid_copy", [copy(src=view(OTHER, height=2 ** 62, pitch=2 ** 20))]),
    "fill: extents past 2^63 bytes": lambda: ("ststhip_grid_fill", [fill(view(height=2 ** 62, pitch=2 ** 20))]),
    "copy: destination rows past the view": lambda: ("ststhip_grid_copy", [copy(dst_row=5)]),
    "copy: destination columns past the view": lambda: ("ststhip_grid_copy", [copy(dst_col=5)]),
    "copy: destination row past 2^64": lambda: ("ststhip_grid_copy", [copy(dst_row=2 ** 64 - 2)]),
    "copy: source rows past the view": lambda: ("ststhip_grid_copy", [copy(src_row=5)]),
    "copy: source columns past the view": lambda: ("ststhip_grid_copy", [copy(src_col=5)]),
    "copy: source rows past the view by their step": lambda: ("ststhip_grid_copy", [copy(src_row_step=3)]),
    "copy: source columns past the view by their step": lambda: ("ststhip_grid_copy", [copy(src_col=1, src_col_step=3)]),
    "copy: a step that overflows": lambda: ("ststhip_grid_copy", [copy(src_col_step=2 ** 63)]),
    "fill: rows past the view": lambda: ("ststhip_grid_fill", [fill(dst_row=5)]),
    "fill: columns past the view": lambda: ("ststhip_grid_fill", [fill(dst_col=7, n_cols=2)]),
    "download: source past the view": lambda: ("ststhip_grid_download", [copy(src_row=6)]),
    "download: host rectangle past its view": lambda: ("ststhip_grid_download", [copy(dst_col=5)]),
    "upload: destination past the view": lambda: ("ststhip_grid_upload", [copy(dst_col=6)]),
    "copy: 2^31 rows": lambda: ("ststhip_grid_copy", [copy(view(height=2 ** 32), view(OTHER, height=2 ** 32), n_rows=2 ** 31)]),
    "copy: 2^31 columns": lambda: ("ststhip_grid_copy", [copy(view(stride=1, width=2 ** 32), view(OTHER + 2 ** 40, stride=1, width=2 ** 32),
                                                              elem_size=1, n_cols=2 ** 31)]),
    "fill: 2^31 rows of no columns": lambda: ("ststhip_grid_fill", [fill(n_rows=2 ** 31, n_cols=0)]),
    "copy: a destination row of 2^31 bytes": lambda: ("ststhip_grid_copy", [copy(view(stride=2 ** 29, width=8), n_cols=4)]),
    "copy: a source row of 2^31 bytes by its step": lambda: ("ststhip_grid_copy", [copy(src=view(OTHER, stride=2 ** 20, width=2 ** 12),
                                                                                    n_cols=4, src_col_step=512)]),
    "fill: a row of 2^31 bytes": lambda: ("ststhip_grid_fill", [fill(view(stride=2 ** 29, width=8))]),
    "download: strided host memory": lambda: ("ststhip_grid_download", [copy(dst=view(stride=8))]),
    "upload: strided host memory": lambda: ("ststhip_grid_upload", [copy(src=view(OTHER, stride=8))]),
    "upload: a step": lambda: ("ststhip_grid_upload", [copy(src_row_step=2, n_rows=2)]),
    "overlap: a plane onto itself": lambda: ("ststhip_grid_copy", [copy(src=view())]),
    "overlap: a plane onto itself, shifted by a column": lambda: ("ststhip_grid_copy", [copy(src=view(), src_col=1)]),
    "overlap: rectangles whose spans interleave": lambda: ("ststhip_grid_copy", [copy(src=view(), dst_col=4)]),
    "overlap: member onto itself": lambda: ("ststhip_grid_copy", [copy(cells(8), cells(8))]),
    "overlap: member onto a member it overlaps": lambda: ("ststhip_grid_copy", [copy(cells(8), cells(10))]),
    "overlap: member to member with a step": lambda: ("ststhip_grid_copy", [copy(cells(8), cells(16), n_rows=2, src_row_step=2)]),
    "overlap: member to member of other cells": lambda: ("ststhip_grid_copy", [copy(cells(8), cells(16), src_col=1)]),
    "overlap: member to member with another pitch": lambda: ("ststhip_grid_copy", [copy(view(BASE + 8, 32, 4, 8, 16), cells(16))]),
    "overlap: member to member with another stride": lambda: ("ststhip_grid_copy", [copy(view(BASE + 8, 16, 8, 8), cells(16))]),
    "overlap: member into the next cell": lambda: ("ststhip_grid_copy", [copy(cells(30), cells(0), elem_size=4)]),
    "copy: second entry bad": lambda: ("ststhip_grid_copy", [copy(), copy(src_row_step=0)]),
    "fill: second entry bad": lambda: ("ststhip_grid_fill", [fill(), fill(dst_row=7)]),
    "download: second entry bad": lambda: ("ststhip_grid_download", [copy(), copy(dst=view(stride=8))]),
}


def call(built_lib, name, entries):
    from stencilstream_amd import capi

    kind = capi.GridFillDesc if name == "ststhip_grid_fill" else capi.GridCopyDesc
    table = (kind * max(len(entries), 1))(*entries)
    return getattr(built_lib, name)(len(entries), table, None)


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_are_refused_before_the_device(built_lib, case):
    """STSTHIP_ERR_INVALID, not "no GPU" (4), on a machine without one: validation comes first."""
    from stencilstream_amd import capi

    name, entries = BAD[case]()
    status = call(built_lib, name, entries)
    assert status == INVALID, (status, capi.last_error())
    assert "grid region" in capi.last_error()


def test_the_wrappers_raise(built_lib):
    from stencilstream_amd import capi

    for wrapper, entry in ((capi.grid_copy, copy(src_row_step=0)), (capi.grid_fill, fill(dst_row=7)),
                           (capi.grid_download, copy(src_row=6)), (capi.grid_upload, copy(dst_col=6))):
        with pytest.raises(capi.StsthipError) as e:
            wrapper([entry])
        assert e.value.status == INVALID


def test_empty_rectangles_need_no_device(built_lib):
    """Nothing to move: success on the host, also for a null base."""
    from stencilstream_amd import capi

    null = view(0)
    capi.grid_copy([copy(null, null, n_rows=0), copy(n_cols=0), copy(null, null, n_rows=0, n_cols=0)])
    capi.grid_fill([fill(null, n_rows=0), fill(n_cols=0)])
    capi.grid_download([copy(null, null, n_cols=0)])
    capi.grid_upload([copy(null, null, n_rows=0)])
    # an empty rectangle may start anywhere
    capi.grid_copy([copy(n_rows=0, dst_row=100, src_col=100)])


ACCEPTED = {
    "copy": lambda: ("ststhip_grid_copy", [copy()]),
    "copy with steps up to the last cell": lambda: ("ststhip_grid_copy", [copy(src_row=1, src_row_step=2, src_col_step=2, src_col=1)]),
    "member to member of the same cells": lambda: ("ststhip_grid_copy", [copy(cells(8), cells(16))]),
    "member to the member in front of it": lambda: ("ststhip_grid_copy", [copy(cells(0), cells(28))]),
    "disjoint rectangles of one plane": lambda: ("ststhip_grid_copy", [copy(src=view(), dst_row=4)]),
    "fill": lambda: ("ststhip_grid_fill", [fill()]),
    "download": lambda: ("ststhip_grid_download", [copy()]),
    "upload": lambda: ("ststhip_grid_upload", [copy()]),
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_a_valid_call_gets_as_far_as_the_device(built_lib, case):
    """Without a GPU a valid, non-empty call fails for want of a device: neither success nor a bad argument."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the made-up addresses must not reach it")
    name, entries = ACCEPTED[case]()
    assert call(built_lib, name, entries) not in (0, INVALID)


def test_grid_methods_refuse_ranges_outside_the_grid(built_lib):
    from stencilstream_amd import update as U

    grid = U.Grid(6, 9, U.HOTSPOT_CELL, device="cpu")  # (no call below gets as far as the cells)
    other = U.Grid(4, 4, U.HOTSPOT_CELL, device="cpu")
    bad = [
        lambda: grid.read(rows=(0, 7)),
        lambda: grid.read(cols=(3, 10)),
        lambda: grid.read(rows=(4, 3)),
        lambda: grid.read(rows=(-1, 3)),
        lambda: grid.read(step=(0, 1)),
        lambda: grid.read(field="pressure"),
        lambda: grid.write(np.zeros((2, 2), dtype=U.HOTSPOT_CELL), at=(5, 0)),
        lambda: grid.write(np.zeros((2, 2), dtype="<f4"), at=(0, 8), field="temp"),
        lambda: grid.write(np.zeros(4, dtype="<f4"), field="temp"),
        lambda: grid.fill(1.0, rows=(0, 7), field="power"),
        lambda: grid.fill((1.0, 2.0), cols=(9, 10)),
        lambda: grid.paste(other, at=(3, 0)),
        lambda: grid.paste(other, rows=(0, 5)),
        lambda: grid.paste(other, cols=(2, 5), at=(0, 0)),
        lambda: other.paste(grid, step=(1, 2)),  # 6 x 5 into 4 x 4
        lambda: grid.paste(U.Grid(4, 4, "<f4", device="cpu")),
    ]
    for attempt in bad:
        with pytest.raises(ValueError):
            attempt()

"""ststhip_grid_norms / ststhip_grid_distance without a GPU: the library exports them, the ctypes mirrors have the
layout of the C structs, and every bad argument is refused before anything touches the device."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

INVALID = 2  # STSTHIP_ERR_INVALID


def test_binding_and_symbols(built_lib):
    from stencilstream_amd import capi

    assert callable(capi.grid_norms) and callable(capi.norm_field)
    raw = C.CDLL(os.path.join(ROOT, "stencilstream_amd", "libststhip.so"))
    for name in ("ststhip_grid_norms", "ststhip_grid_distance"):
        assert hasattr(raw, name), f"libststhip.so lacks {name}"
    assert built_lib.ststhip_abi_version() == 6  # additive


def test_ctypes_structs_mirror_the_c_structs(built_lib, tmp_path):
    from stencilstream_amd import capi

    names = {"ststhip_norm_field": capi.NormField, "ststhip_norm_result": capi.NormResult}
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
    assert len(want) == 2 + len(capi.NormField._fields_) + len(capi.NormResult._fields_)


def field(**changes):
    """A valid description of an 8 x 8 plane of floats at a made-up, aligned address; `changes` break it."""
    from stencilstream_amd import capi

    f = capi.norm_field(0x10000, "<f4", 4, 8, 8)
    for name, value in changes.items():
        setattr(f, name, value)
    return f


BAD = {
    "no field": lambda: ([], None),
    "nine fields": lambda: ([field()] * 9, None),
    "unknown type": lambda: ([field(type=2)], None),
    "misaligned base": lambda: ([field(base=0x10002)], None),
    "misaligned base of a double": lambda: ([field(type=1, stride=8, base=0x10004)], None),
    "misaligned stride": lambda: ([field(stride=6)], None),
    "misaligned stride of a double": lambda: ([field(type=1, stride=12)], None),
    "stride 0": lambda: ([field(stride=0)], None),
    "null grid": lambda: ([field(base=None)], None),
    "pitch below the width": lambda: ([field(pitch=7)], None),
    "extents past 2^63 bytes": lambda: ([field(height=2 ** 62, pitch=2 ** 20)], None),
    "second field bad": lambda: ([field(), field(stride=0)], None),
    "distance: null second grid": lambda: ([field()], [0]),
    "distance: misaligned second grid": lambda: ([field()], [0x20002]),
    "distance: stride 0": lambda: ([field(stride=0)], [0x20000]),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_are_refused_before_the_device(built_lib, case):
    """STSTHIP_ERR_INVALID, not "no GPU" (4), on a machine without one: validation comes first."""
    from stencilstream_amd import capi

    fields, other = BAD[case]()
    n = len(fields)
    table = (capi.NormField * max(n, 1))(*fields)
    result = (capi.NormResult * max(n, 1))()
    if other is None:
        status = built_lib.ststhip_grid_norms(n, table, result, None)
    else:
        status = built_lib.ststhip_grid_distance(n, table, (C.c_void_p * n)(*other), result, None)
    assert status == INVALID, (status, capi.last_error())
    assert "grid norms" in capi.last_error()


def test_the_wrapper_raises(built_lib):
    from stencilstream_amd import capi

    with pytest.raises(capi.StsthipError) as e:
        capi.grid_norms([field(stride=0)])
    assert e.value.status == INVALID
    with pytest.raises(ValueError):
        capi.norm_field(0x10000, "<i4", 4, 8, 8)


def test_empty_rectangles_need_no_device(built_lib):
    """Nothing to read: the answer is known on the host (also for a null grid)."""
    from stencilstream_amd import capi

    empty = field(base=None, row_begin=3, row_end=3)
    past = field(base=None, col_begin=8, col_end=20)  # clipped to nothing
    for r in capi.grid_norms([empty, past]):
        assert (r.n_cells, r.n_nonfinite, r.sum, r.sum_abs, r.sum_sq) == (0, 0, 0.0, 0.0, 0.0)
        assert r.max_abs == float("-inf")

"""The case table of tests/test_large_extents_gpu.py in Python integers, without a GPU: every case crosses the threshold
it is named for, asks for no more memory than a test may, is admitted by the limits ststhip.h documents -- and its data
would expose a kernel that forms a row's byte offset in 32 bits.

Sensitivity is shown on the table, not by planting bugs in kernels.  Two models of a defective kernel address element
(i, j) of a rectangle at  first + f(i * row distance) + j * step  with f = the offset kept to 32 bits, and f = the
offset sign-extended from 32 bits.  For every rectangle of the geometries named for their row distances, every row
beyond the first whose offset a model changes then loads, in at least one cell (in fact in every cell looked at), a
value other than the coded one of the right cell: another cell's code, or the sentinel.  Both models change at least
one row of every such rectangle, and neither leaves the allocation: that is what the front guard is for."""
import pytest

import large_extents as LE
from large_extents import BY_ID, CASES, FRONT_GUARD, GiB

MODELS = {"kept to 32 bits": LE.kept_to_32_bits, "sign-extended from 32 bits": LE.sign_extended_from_32_bits}
ROW_DISTANCE_GEOMETRIES = ("G1", "G2", "G3", "G1xG2")


def device_rects(case):
    return [(op, r) for op in case.ops for r in op.rects() if r.view.buf is not None]


def test_the_two_models_on_numbers_worked_by_hand():
    assert LE.kept_to_32_bits((1 << 32) + 16) == 16 and LE.kept_to_32_bits((1 << 31) + 12) == (1 << 31) + 12
    assert LE.sign_extended_from_32_bits((1 << 31) + 12) == 12 - (1 << 31)
    assert LE.sign_extended_from_32_bits((1 << 32) + 16) == 16 and LE.sign_extended_from_32_bits(3 * (1 << 31) + 36) == 36 - (1 << 31)
    assert LE.code_of(0, 0, 0) == -125 and LE.code_of(1, 0, 0) == -108 and LE.code_of(0, 1, 0) == 6 and LE.code_of(0, 0, 36) == -124
    assert all(-125 <= LE.code_of(k, r, c) <= 125 for k in range(8) for r in range(4) for c in range(0, 9000, 17))


def test_every_case_has_a_unique_name_and_needs_40_gib_at_the_most():
    assert len(CASES) >= 20
    for case in CASES:
        assert 0 < case.need() <= LE.MAX_NEED, (case.id, case.need() / GiB)
    assert LE.G4_NEED <= LE.MAX_NEED and LE.AOS_NEED <= LE.MAX_NEED
    for app, sizes in (("jacobi", [4]), ("hotspot", [4, 4]), ("hotspot_aos", [8]), ("fdtd_coef_aos", [32]), ("conway", [1])):
        assert LE.sweep_need(sizes) <= LE.MAX_NEED, app


@pytest.mark.parametrize("case_id", sorted(BY_ID))
def test_a_case_crosses_the_threshold_it_is_named_for(case_id):
    case = BY_ID[case_id]
    rects = device_rects(case)
    assert rects
    for _, r in rects:
        assert r.admitted(), (case_id, r)
        assert r.last_byte() < r.view.extent() <= case.views()[r.view.buf].extent()
    highest = max(r.last_byte() for _, r in rects)
    if "2^31" in case.crosses:
        assert highest >= 1 << 31, case_id
    if "2^32" in case.crosses:
        assert highest >= 1 << 32, case_id
        for op in case.ops:  # every operation of it, in at least one operand
            assert max(r.last_byte() for r in op.rects() if r.view.buf is not None) >= 1 << 32, (case_id, op.name)
    if "row" in case.crosses:
        assert case.geometry == "G5"
        for op in case.ops:
            longest = max(r.row_extent() for r in op.rects())
            # a transfer's fine side has an even number of columns: 2 * (2^28 - 1) floats
            assert longest == ((1 << 31) - 8 if op.kind in ("restrict", "prolong") else (1 << 31) - 4), (case_id, op.name)
            for r in op.rects():
                assert r.admitted() and r.n_cols < 1 << 31 and r.row_extent() < 1 << 31
    if case.geometry == "G1":
        assert {r.view.row_bytes for _, r in rects if r.view.height == 4} <= {(1 << 31) + 12, (1 << 31) + 24}
        assert any(r.row + r.n_rows >= 3 for _, r in rects)  # a row that begins beyond 2^32
    if case.geometry == "G2":
        assert {r.row_distance() for _, r in rects if r.view.height == 3} <= {(1 << 32) + 16, (1 << 32) + 32}
    if case.geometry == "G3":
        assert all(r.view.row_bytes == 6 * GiB for _, r in rects)
        assert {r.first() % r.view.row_bytes for _, r in rects} <= {(1 << 31) + 4, (1 << 32) + 28, 1 << 32, (1 << 31) + 16}
        assert any(r.first() >= 1 << 32 for _, r in rects)


def test_g5_cells_and_admission():
    assert LE.G5_CELLS == (1 << 30) - 2
    v = LE.geometry_views("G5")["P"]
    assert v.width * 4 == (1 << 31) - 4 and v.pitch == (1 << 29) + 1
    one_more = LE.Rect(LE.plane("P", 0, (1 << 29) + 1, 2, 1 << 29), 0, 0, 2, 1 << 29)
    assert not one_more.admitted()  # 2^31 bytes: the first row ststhip.h refuses


@pytest.mark.parametrize("case_id", sorted(LE.G4))
def test_g4_rows_have_more_segments_than_a_launch_has_workgroups(case_id):
    family, layout, n_cols = LE.G4[case_id]
    segment, cap = LE.segments_of(family)[layout]
    # floats of a row per workgroup: 16 KiB (regions, algebra) or 8 KiB (norms, dot) of a dense row, 1024 cells of a
    # strided one and of every row of the general stencil kernel (the dense stencil kernel has no cap)
    dense = {"regions": 4096, "algebra": 4096, "norms": 2048, "dot": 2048, "stencil": 1024}[family]
    assert cap == 2048 and segment == (dense if layout == "dense" else 1024)
    assert n_cols > cap * segment
    segments, _ = LE.g4_segments(case_id)
    assert segments > cap  # plan_blocks: `down` becomes 1 and gridDim.x exceeds the cap


def test_scatter_and_sweep_extents():
    assert LE.AOS_CELLS * LE.AOS_CELL_BYTES == (1 << 32) + 96
    for size in (1, 4, 8, 32):
        pitch = LE.sweep_pitch(size)
        distance = pitch * size
        assert LE.SWEEP_ROW_DISTANCE <= distance < LE.SWEEP_ROW_DISTANCE + size and pitch < 1 << 31
        assert 7 * distance < 1 << 31 <= 8 * distance and 15 * distance < 1 << 32 <= 16 * distance
    assert LE.sweep_pitch(4) * 4 == LE.SWEEP_ROW_DISTANCE == LE.sweep_pitch(1)


@pytest.mark.parametrize("case_id", sorted(c.id for c in CASES if c.geometry in ROW_DISTANCE_GEOMETRIES))
def test_the_data_exposes_a_row_offset_formed_in_32_bits(case_id):
    case = BY_ID[case_id]
    looked_at, far_firsts, exposing = 0, set(), set()
    for op, r in device_rects(case):
        v = r.view
        if r.n_rows == 1 or v.row_bytes < 1 << 31:  # (the small coarse grid of a transfer)
            continue
        cols = sorted({0, 1, 2, 3, 4, 5, r.n_cols // 2, r.n_cols - 1})
        for name, model in MODELS.items():
            changed = [i for i in range(1, r.n_rows) if model(i * r.row_distance()) != i * r.row_distance()]
            if name.startswith("sign") or (r.n_rows - 1) * r.row_distance() >= 1 << 32:
                assert changed, (case_id, op.name, name)
                exposing.add(name)
            if v.row_bytes >= 1 << 32 or name.startswith("sign"):
                assert changed == list(range(1, r.n_rows)), (case_id, op.name, name)
            for i in changed:
                exposed = 0
                for j in cols:
                    right_r, right_c = r.row + i * r.row_step, r.col + j * r.col_step
                    wrong = r.first() + model(i * r.row_distance()) + j * r.col_step * v.stride
                    assert -FRONT_GUARD <= wrong and wrong + v.elem <= v.extent() + LE.BACK_GUARD, "the model leaves the allocation"
                    assert wrong != v.at(right_r, right_c)
                    exposed += LE.value_at_byte(r, wrong) != LE.code_of(v.k, right_r, right_c)
                    looked_at += 1
                assert exposed >= 1, (case_id, op.name, name, i)
                assert exposed == len(cols), (case_id, op.name, name, i)
        if case.geometry == "G3":  # the same for the offset of the rectangle's first element, far into a row
            for name, model in MODELS.items():
                if model(r.first()) == r.first():  # (byte 2^31 + 4 of a row, kept to 32 bits)
                    continue
                far_firsts.add(name)
                for i in range(r.n_rows):
                    for j in cols:
                        wrong = model(r.first()) + i * r.row_distance() + j * r.col_step * v.stride
                        assert -FRONT_GUARD <= wrong and wrong + v.elem <= v.extent() + LE.BACK_GUARD
                        assert LE.value_at_byte(r, wrong) != LE.code_of(v.k, r.row + i * r.row_step, r.col + j * r.col_step)
    assert looked_at > 0
    assert case.geometry != "G3" or far_firsts == set(MODELS)
    assert exposing == set(MODELS)  # (a rectangle of two rows 2^31 + 12 bytes apart shows the second model only)

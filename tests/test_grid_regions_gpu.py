"""ststhip_grid_copy / _fill / _download / _upload on the device, through capi, against numpy slicing on the host.

Every device buffer has GUARD bytes in front of and behind the grid and holds random bytes everywhere; the host keeps a
model of all of it.  A call is mirrored on the model with a numpy slice assignment on byte views
(dst[r:r+n, c:c+m] = src[rs:rs+n*sr:sr, cs:cs+m*sc:sc], the element's bytes), and then the WHOLE buffer is compared
with the model: the rectangle holds what it should, every other byte of the grid -- cells outside the rectangle, other
members of the cells inside it, the pitch padding -- and both guards are untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096


class Buffer:
    """height x pitch cells of `stride` bytes in HBM between two guards, and the host's model of all of it."""

    def __init__(self, device, height, pitch, stride, seed, width=None):
        self.height, self.pitch, self.stride = height, pitch, stride
        self.width = pitch if width is None else width
        self.n = height * pitch * stride
        self.model = np.random.default_rng(seed).integers(0, 256, size=GUARD + self.n + GUARD, dtype=np.uint8)
        self.device = torch.from_numpy(self.model.copy()).to(device)
        self.base = self.device.data_ptr() + GUARD

    def bytes(self):
        """The model's cells as height x pitch x stride bytes (a view: assigning to it changes the model)."""
        return self.model[GUARD:GUARD + self.n].reshape(self.height, self.pitch, self.stride)

    def view(self, offset=0):
        from stencilstream_amd import capi

        return capi.grid_view(self.base + offset, self.stride, self.height, self.width, self.pitch)

    def check(self, what):
        torch.cuda.synchronize()
        got = self.device.cpu().numpy()
        assert np.array_equal(got[:GUARD], self.model[:GUARD]), f"{what}: bytes in front of the grid changed"
        assert np.array_equal(got[GUARD + self.n:], self.model[GUARD + self.n:]), f"{what}: bytes behind the grid changed"
        if not np.array_equal(got, self.model):
            wrong = np.flatnonzero(got != self.model) - GUARD
            cell, byte = np.divmod(wrong, self.stride)
            row, col = np.divmod(cell, self.pitch)
            raise AssertionError(f"{what}: {wrong.size} bytes differ, the first at row {row[0]}, column {col[0]}, "
                                 f"byte {byte[0]} of the cell")


def mirror(dst, src, elem, n_rows, n_cols, dst_at=(0, 0), src_at=(0, 0), step=(1, 1), dst_offset=0, src_offset=0):
    """The reference: one numpy slice assignment on the models' bytes."""
    (r, c), (rs, cs), (sr, sc) = dst_at, src_at, step
    taken = src.bytes()[rs:rs + n_rows * sr:sr, cs:cs + n_cols * sc:sc, src_offset:src_offset + elem].copy()
    assert taken.shape == (n_rows, n_cols, elem)
    dst.bytes()[r:r + n_rows, c:c + n_cols, dst_offset:dst_offset + elem] = taken


def copy(dst, src, elem, n_rows, n_cols, dst_at=(0, 0), src_at=(0, 0), step=(1, 1), dst_offset=0, src_offset=0):
    """The description of a copy, and the same copy on the models."""
    from stencilstream_amd import capi

    mirror(dst, src, elem, n_rows, n_cols, dst_at, src_at, step, dst_offset, src_offset)
    return capi.grid_copy_desc(dst.view(dst_offset), src.view(src_offset), elem, n_rows, n_cols, dst_at, src_at, step)


# ------------------------------------------------------------------ dense planes
@pytest.mark.parametrize("width", [1, 3, 4, 5, 63, 64, 65, 257])
@pytest.mark.parametrize("elem", [1, 4, 8])
def test_dense_planes_at_every_alignment(gpu, elem, width):
    """Rows 0..3 of a 5-row plane into rows 1..4 of another, pitch = width + 3, from source column offsets 0..4 to
    destination column offsets 0..4, up to the last column: the same alignment modulo 16 bytes and every other, heads and
    tails of every length."""
    from stencilstream_amd import capi

    src = Buffer(gpu, 5, width + 3, elem, seed=1000 * elem + width, width=width)
    dst = Buffer(gpu, 5, width + 3, elem, seed=2000 * elem + width, width=width)
    n_calls = 0
    for d in range(5):
        for s in range(5):
            n_cols = width - max(d, s)
            if n_cols < 1:
                continue
            capi.grid_copy([copy(dst, src, elem, 4, n_cols, dst_at=(1, d), src_at=(0, s))])
            dst.check(f"{elem}-byte plane of width {width}, column {s} -> column {d}")
            n_calls += 1
    assert n_calls >= 1
    src.check("the source")


def test_dense_single_element_and_last_cell(gpu):
    from stencilstream_amd import capi

    for elem in (1, 4, 8):
        src = Buffer(gpu, 5, 20, elem, seed=31 + elem, width=17)
        dst = Buffer(gpu, 7, 9, elem, seed=41 + elem)
        capi.grid_copy([copy(dst, src, elem, 1, 1, dst_at=(6, 8), src_at=(4, 16))])  # last cell to last cell
        dst.check("a single element")
        capi.grid_copy([copy(dst, src, elem, 1, 1, dst_at=(3, 3), src_at=(2, 5))])
        dst.check("a single element in the middle")
        capi.grid_copy([copy(dst, src, elem, 5, 9, src_at=(0, 8))])  # ends in the source's last row and column
        dst.check("a rectangle up to the source's last cell")
        src.check("the source")


# ------------------------------------------------------------------ strided: members of cells
CELLS = {
    "8 bytes": np.dtype([("a", "<f4"), ("b", "<f4")]),
    "20 bytes": np.dtype([("a", "<f4"), ("b", "<f8"), ("c", "<f4"), ("d", "<u2"), ("e", "<u2")]),  # packed: b at 4
    "32 bytes": np.dtype([(n, "<f4") for n in ("ex", "ey", "hz", "hz_sum", "ca", "cb", "da", "db")]),
    "88 bytes": np.dtype([(f"f{i}", "<f8") for i in range(11)]),
    "5 bytes": np.dtype([("a", "u1"), ("b", "<f4")]),  # packed: nothing is aligned
}
assert [CELLS[k].itemsize for k in CELLS] == [8, 20, 32, 88, 5]
H, W = 37, 53


@pytest.mark.parametrize("cell", sorted(CELLS))
def test_members_of_cells(gpu, cell):
    from stencilstream_amd import capi

    dt = CELLS[cell]
    stride = dt.itemsize
    grid = Buffer(gpu, H, W, stride, seed=7 * stride)
    second = Buffer(gpu, H, W, stride, seed=9 * stride)
    members = [(name, dt.fields[name][0].itemsize, dt.fields[name][1]) for name in dt.names]
    for name, size, offset in members:
        # member -> dense plane (with a pitch) -> the same member of a second grid, elsewhere
        plane = Buffer(gpu, H, W + 3, size, seed=stride + offset, width=W)
        capi.grid_copy([copy(plane, grid, size, H - 2, W - 3, dst_at=(0, 1), src_at=(2, 3), src_offset=offset)])
        plane.check(f"{cell}: member {name} -> plane")
        capi.grid_copy([copy(second, plane, size, H - 2, W - 3, dst_at=(1, 0), src_at=(0, 1), dst_offset=offset)])
        second.check(f"{cell}: plane -> member {name}")
        # ... and the whole grid's member
        capi.grid_copy([copy(plane, grid, size, H, W, src_offset=offset)])
        plane.check(f"{cell}: all of member {name} -> plane")
    # a whole cell
    capi.grid_copy([copy(second, grid, stride, H - 1, W - 2, dst_at=(1, 2))])
    second.check(f"{cell}: whole cells")
    capi.grid_copy([copy(second, grid, stride, H, W)])
    second.check(f"{cell}: the whole grid")
    # member to member of the same cells: the one overlap that is accepted
    (_, size_a, offset_a), (_, size_b, offset_b) = members[0], members[1]
    size = min(size_a, size_b)
    capi.grid_copy([copy(grid, grid, size, H - 3, W - 1, dst_at=(3, 1), src_at=(3, 1), dst_offset=offset_b, src_offset=offset_a)])
    grid.check(f"{cell}: member to member")
    capi.grid_copy([copy(grid, grid, size, H, W, dst_offset=offset_a, src_offset=offset_b)])
    grid.check(f"{cell}: member to member, the other way, all cells")
    # element sizes that are no member's: 3 and 12 bytes from byte 1 of the cell
    for elem in (3, 12):
        if 1 + elem > stride:
            continue
        plane = Buffer(gpu, H, W + 1, elem, seed=elem, width=W)
        capi.grid_copy([copy(plane, grid, elem, H, W, src_offset=1)])
        plane.check(f"{cell}: {elem} bytes of every cell -> plane")
        capi.grid_copy([copy(second, plane, elem, H - 5, W - 7, dst_at=(5, 7), src_at=(0, 0), dst_offset=1)])
        second.check(f"{cell}: plane -> {elem} bytes of every cell")
    grid.check("the first grid")


# ------------------------------------------------------------------ steps
@pytest.mark.parametrize("step", [(1, 1), (2, 3), (7, 1), (1, 5)])
def test_steps(gpu, step):
    """130 x 1031: more than one row segment, more rows than a small launch has workgroups down the rows."""
    from stencilstream_amd import capi

    h, w = 130, 1031
    grid = Buffer(gpu, h, w, 8, seed=step[0] * 16 + step[1])
    n_rows, n_cols = -(-(h - 1) // step[0]), -(-(w - 2) // step[1])
    plane = Buffer(gpu, n_rows + 1, n_cols + 2, 4, seed=5)
    capi.grid_copy([copy(plane, grid, 4, n_rows, n_cols, dst_at=(1, 2), src_at=(1, 2), step=step, src_offset=4)])
    plane.check(f"member with step {step}")
    cells = Buffer(gpu, n_rows, n_cols, 8, seed=6)
    capi.grid_copy([copy(cells, grid, 8, n_rows, n_cols, src_at=(1, 2), step=step)])
    cells.check(f"cells with step {step}")
    dense = Buffer(gpu, h, w, 4, seed=8)
    capi.grid_copy([copy(plane, dense, 4, n_rows, n_cols, dst_at=(1, 2), src_at=(1, 2), step=step)])
    plane.check(f"plane to plane with step {step}")
    grid.check("the source")


def test_a_step_larger_than_the_rectangle(gpu):
    from stencilstream_amd import capi

    grid = Buffer(gpu, 9, 11, 8, seed=77)
    plane = Buffer(gpu, 3, 3, 4, seed=78)
    # rows 5:8:10 and columns 6:10:10 are one cell
    capi.grid_copy([copy(plane, grid, 4, 1, 1, dst_at=(2, 2), src_at=(5, 6), step=(10, 10))])
    plane.check("a step larger than the rectangle")
    capi.grid_copy([copy(plane, grid, 4, 2, 1, src_at=(0, 10), step=(8, 1000))])  # rows 0 and 8 of the last column
    plane.check("a column step past the grid with one column")


# ------------------------------------------------------------------ eight entries
def test_eight_entries_in_one_call(gpu):
    from stencilstream_amd import capi

    grid = Buffer(gpu, H, W, 88, seed=88)
    entries, targets = [], []
    shapes = [(1, 8, 0, (H, W), (0, 0)), (2, 16, 2, (5, 7), (3, 4)), (3, 24, 1, (H - 1, W - 1), (1, 1)),
              (4, 32, 0, (1, W), (36, 0)), (8, 40, 0, (H, 1), (0, 52)), (12, 48, 4, (11, 13), (7, 9)),
              (16, 64, 0, (H, W), (0, 0)), (88, 0, 0, (20, 30), (17, 23))]
    for i, (elem, offset, pad, (n_rows, n_cols), at) in enumerate(shapes):
        target = Buffer(gpu, n_rows + 1, n_cols + pad, elem, seed=800 + i)
        entries.append(copy(target, grid, elem, n_rows, n_cols, dst_at=(1, pad // 2), src_at=at, src_offset=offset))
        targets.append(target)
    capi.grid_copy(entries)
    for (elem, *_), target in zip(shapes, targets):
        target.check(f"entry of {elem} bytes")
    grid.check("the source")


# ------------------------------------------------------------------ fill
NAN_WITH_PAYLOAD = np.array([0x7FF8DEADBEEF0001], dtype="<u8").tobytes()
MINUS_ZERO = np.array([-0.0], dtype="<f8").tobytes()


@pytest.mark.parametrize("rect", ["1 x 1", "3 x 3", "a whole row", "the whole grid"])
def test_fill(gpu, rect):
    from stencilstream_amd import capi

    (r, c), (n_rows, n_cols) = {"1 x 1": ((36, 52), (1, 1)), "3 x 3": ((11, 17), (3, 3)), "a whole row": ((5, 0), (1, W)),
                                "the whole grid": ((0, 0), (H, W))}[rect]
    grid = Buffer(gpu, H, W + 2, 88, seed=len(rect), width=W)

    def fill(value, offset):
        grid.bytes()[r:r + n_rows, c:c + n_cols, offset:offset + len(value)] = np.frombuffer(value, dtype=np.uint8)
        return capi.grid_fill_desc(grid.view(offset), value, n_rows, n_cols, dst_at=(r, c))

    for value in (NAN_WITH_PAYLOAD, MINUS_ZERO):
        capi.grid_fill([fill(value, 24)])
        grid.check(f"member of {rect}")
    cell = (NAN_WITH_PAYLOAD + MINUS_ZERO) * 5 + np.array([1.5], dtype="<f8").tobytes()
    assert len(cell) == 88
    capi.grid_fill([fill(cell, 0)])
    grid.check(f"whole cells of {rect}")
    # two entries, members of different sizes of the packed 5-byte cells
    packed = Buffer(gpu, H, W, 5, seed=55)
    n_r, n_c = min(n_rows, H), min(n_cols, W)

    def fill_packed(value, offset):
        packed.bytes()[r:r + n_r, c:c + n_c, offset:offset + len(value)] = np.frombuffer(value, dtype=np.uint8)
        return capi.grid_fill_desc(packed.view(offset), value, n_r, n_c, dst_at=(r, c))

    capi.grid_fill([fill_packed(b"\x81", 0), fill_packed(np.array([-0.0], dtype="<f4").tobytes(), 1)])
    packed.check(f"two members of packed cells of {rect}")


# ------------------------------------------------------------------ download and upload
def test_download_with_a_host_pitch_and_decimated(gpu):
    from stencilstream_amd import capi

    grid = Buffer(gpu, H, W, 32, seed=321)
    hz = grid.bytes()[:, :, 8:12].copy().view("<f4")[:, :, 0]
    # host rows longer than the rectangle's, the rectangle not at their start
    host = np.full((H + 1, W + 5), 7.0, dtype="<f4")
    want = host.copy()
    want[1:, 2:2 + W - 3] = hz[:, 3:]
    view = capi.grid_view(host.ctypes.data, 4, H + 1, W + 5)
    capi.grid_download([capi.grid_copy_desc(view, grid.view(8), 4, H, W - 3, dst_at=(1, 2), src_at=(0, 3))])
    assert np.array_equal(host.view(np.uint32), want.view(np.uint32))
    # decimated, dense
    small = np.zeros((10, 11), dtype="<f4")
    capi.grid_download([capi.grid_copy_desc(capi.grid_view(small.ctypes.data, 4, 10, 11), grid.view(8), 4, 10, 11,
                                            src_at=(0, 1), step=(4, 5))])
    assert np.array_equal(small.view(np.uint32), hz[0:40:4, 1:56:5].view(np.uint32))
    # whole cells, and two entries in one call
    cells = np.zeros((4, 6, 32), dtype=np.uint8)
    one = np.zeros((1, 1), dtype="<f4")
    capi.grid_download([capi.grid_copy_desc(capi.grid_view(cells.ctypes.data, 32, 4, 6), grid.view(), 32, 4, 6, src_at=(33, 47)),
                        capi.grid_copy_desc(capi.grid_view(one.ctypes.data, 4, 1, 1), grid.view(8), 4, 1, 1, src_at=(36, 52))])
    assert np.array_equal(cells, grid.bytes()[33:, 47:, :])
    assert one.view(np.uint32)[0, 0] == hz.view(np.uint32)[36, 52]
    grid.check("the grid after downloads")


def test_upload_round_trip_and_reuse_of_the_host_array(gpu):
    from stencilstream_amd import capi

    grid = Buffer(gpu, H, W, 88, seed=654)
    rng = np.random.default_rng(11)
    # a member from host rows with a pitch
    host = rng.integers(0, 2 ** 63, size=(9, 20), dtype=np.int64).view("<f8")
    sent = host.copy()
    view = capi.grid_view(host.ctypes.data, 8, 9, 20)
    capi.grid_upload([capi.grid_copy_desc(grid.view(16), view, 8, 9, 13, dst_at=(28, 40), src_at=(0, 7))])
    host[...] = 0.0  # the caller's array is free when the call has returned
    grid.bytes()[28:37, 40:53, 16:24] = sent[:, 7:].copy().view(np.uint8).reshape(9, 13, 8)
    grid.check("member uploaded from host rows with a pitch")
    back = np.zeros((9, 13), dtype="<f8")
    capi.grid_download([capi.grid_copy_desc(capi.grid_view(back.ctypes.data, 8, 9, 13), grid.view(16), 8, 9, 13, src_at=(28, 40))])
    assert np.array_equal(back.view(np.uint64), sent[:, 7:].view(np.uint64))
    # whole cells of the packed grid: nothing aligned, odd row length
    packed = Buffer(gpu, H, W, 5, seed=656)
    cells = rng.integers(0, 256, size=(H, W, 5), dtype=np.uint8)
    sent = cells.copy()
    capi.grid_upload([capi.grid_copy_desc(packed.view(), capi.grid_view(cells.ctypes.data, 5, H, W), 5, H, W)])
    cells[...] = 0
    packed.bytes()[...] = sent
    packed.check("whole packed grid uploaded")
    back = np.zeros((H, W, 5), dtype=np.uint8)
    capi.grid_download([capi.grid_copy_desc(capi.grid_view(back.ctypes.data, 5, H, W), packed.view(), 5, H, W)])
    assert np.array_equal(back, sent)


# ------------------------------------------------------------------ stream order
def test_copy_is_ordered_on_the_stream(gpu):
    """A chain of torch kernels on the stream produces the source in front of grid_copy, a torch kernel reads the target
    right behind it: no synchronisation in between."""
    from stencilstream_amd import capi

    h, w = 512, 2048
    start = np.arange(h * w, dtype=np.int32).reshape(h, w)
    want = start.copy()
    for _ in range(40):
        want = want * np.int32(3) + np.int32(1)  # (wraps, on both sides alike)
    stream = torch.cuda.Stream(gpu)
    held = torch.from_numpy(start).to(gpu)
    target = torch.full((h // 2, w // 2), -1, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        source = held
        for _ in range(40):
            source = source * 3 + 1
        dst = capi.grid_view(target.data_ptr(), 4, h // 2, w // 2)
        src = capi.grid_view(source.data_ptr(), 4, h, w)
        capi.grid_copy([capi.grid_copy_desc(dst, src, 4, h // 2, w // 2, src_at=(1, 0), step=(2, 2))], stream.cuda_stream)
        seen = target + 0
    stream.synchronize()
    assert np.array_equal(seen.cpu().numpy(), want[1::2, 0::2])


# ------------------------------------------------------------------ update.Grid
def test_grid_methods_against_numpy(gpu):
    from stencilstream_amd import update as U

    rng = np.random.default_rng(3)
    model = np.zeros((61, 83), dtype=U.HOTSPOT_CELL)
    model["temp"] = rng.random((61, 83), dtype=np.float32)
    model["power"] = rng.random((61, 83), dtype=np.float32)
    grid = U.Grid.from_numpy(model, gpu)

    def same(a, b):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).tobytes()

    assert same(grid.read(), model)
    assert same(grid.read(rows=(3, 61), cols=(0, 80), step=(4, 7)), model[3:61:4, 0:80:7])
    assert same(grid.read(field="power", rows=(60, 61)), model["power"][60:61])
    assert same(grid.read(field="temp", step=(2, 2)), model["temp"][::2, ::2])
    assert grid.read(rows=(5, 5)).shape == (0, 83)

    patch = rng.random((7, 5), dtype=np.float32)
    grid.write(patch, at=(54, 78), field="temp")
    model["temp"][54:61, 78:83] = patch
    block = np.zeros((2, 3), dtype=U.HOTSPOT_CELL)
    block["temp"], block["power"] = -1.0, -2.0
    grid.write(block, at=(0, 0))
    model[0:2, 0:3] = block
    assert same(grid.to_numpy(), model)

    grid.fill(np.float32(-0.0), rows=(10, 13), cols=(20, 23), field="power")
    model["power"][10:13, 20:23] = np.float32(-0.0)
    grid.fill((5.0, 6.0), rows=(60, 61))
    model[60:61] = (5.0, 6.0)
    assert same(grid.to_numpy(), model)

    other_model = np.zeros((40, 50), dtype=U.HOTSPOT_CELL)
    other_model["temp"] = 9.0
    other = U.Grid.from_numpy(other_model, gpu)
    other.paste(grid, rows=(1, 61), cols=(3, 83), at=(10, 10), step=(2, 2))  # 30 x 40
    other_model[10:40, 10:50] = model[1:61:2, 3:83:2]
    assert same(other.to_numpy(), other_model)
    grid.paste(other, rows=(0, 5), at=(56, 33))
    model[56:61, 33:83] = other_model[0:5]
    assert same(grid.to_numpy(), model)


def test_a_block_filled_in_between_two_updates(gpu, oracle):
    """jacobi5general on 300 x 700: 21 generations, a 3 x 3 block filled in where the cells are, 21 more; the oracle runs
    the same way with the block set on the host."""
    from stencilstream_amd import update as U

    rng = np.random.default_rng(0x5EED)
    start = rng.random((300, 700), dtype=np.float32)
    coef = [0.1, 0.2, 0.3, 0.25, 0.15]
    update = U.StencilUpdate(U.Params(U.jacobi("Jacobi5General", coef), halo_value=np.float32(0.0), n_iterations=21))
    grid = update(U.Grid.from_numpy(start, gpu))
    grid.fill(np.float32(50.0), rows=(150, 153), cols=(400, 403))
    got = update(grid).to_numpy()

    want = oracle.jacobi("Jacobi5General", coef, start, 21, halo=0.0, n_threads=4)
    want[150:153, 400:403] = np.float32(50.0)
    want = oracle.jacobi("Jacobi5General", coef, want, 21, halo=0.0, n_threads=4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[151, 401] > 1.0  # (the block is there: nothing else exceeds 1)

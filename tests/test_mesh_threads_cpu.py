"""The host-only pieces of mesh_threads.py (the ranks of a mesh as threads, tests/test_mesh_apps_gpu.py): cells to the
planes of a registered function and back, and the ways a mailbox ends a wait -- none of them by running out a limit."""
import queue

import numpy as np
import pytest


def test_split_and_join_planes_round_trip(oracle):
    from stencilstream_amd import capi

    from mesh_threads import join_planes, split_planes

    rng = np.random.default_rng(7)
    for app, dtype in (("selfcheck1", oracle.SELFCHECK_CELL), ("selfcheck1_soa", oracle.SELFCHECK_CELL),
                       ("hotspot_f64", oracle.HOTSPOT_CELL_F64), ("hotspot_aos", oracle.HOTSPOT_CELL),
                       ("fdtd_coef", oracle.FDTD_CELL), ("fdtd_coef_grouped", oracle.FDTD_CELL),
                       ("fdtd_coef_aos", oracle.FDTD_CELL), ("jacobi25general", np.dtype("<f4"))):
        info = capi.app_info(app)
        assert info.cell_size == dtype.itemsize
        cells = rng.integers(0, 256, (5, 7 * dtype.itemsize), dtype=np.uint8).view(dtype).reshape(5, 7)
        planes = split_planes(info, cells)
        assert [p.shape for p in planes] == [(5, 7 * info.plane_elem_size[i]) for i in range(info.n_planes)]
        for i, plane in enumerate(planes):  # plane i holds bytes [offset, offset + size) of every cell
            size, offset = info.plane_elem_size[i], info.field_offset[i]
            assert np.array_equal(plane.reshape(5, 7, size), cells.view(np.uint8).reshape(5, 7, -1)[:, :, offset:offset + size])
        as_downloaded = [p.view(np.dtype(f"V{info.plane_elem_size[i]}")) for i, p in enumerate(planes)]
        back = join_planes(info, as_downloaded, dtype, np.zeros_like(cells))
        assert np.array_equal(back.view(np.uint8), cells.view(np.uint8))


def test_a_wait_ends_at_once_when_another_rank_has_failed():
    from mesh_threads import Mailbox, MeshError

    box = Mailbox(3, 1, timeout=3600.0)
    box.failed.set()
    with pytest.raises(MeshError, match="another rank has failed"):
        box._take(1, (0, "down"), [0], [64], None)


def test_a_message_of_the_wrong_size_is_an_error():
    from mesh_threads import Mailbox, MeshError

    box = Mailbox(2, 2, timeout=3600.0)
    box.edges[(0, "right")].put([bytearray(48)])
    with pytest.raises(MeshError, match=r"rank 1: edge right of rank 0: expected \[64\] bytes, received \[48\]"):
        box._take(1, (0, "right"), [0], [64], None)
    assert box.failed.is_set()


def test_every_edge_holds_one_message():
    from mesh_threads import Mailbox

    box = Mailbox(3, 3)
    assert len(box.edges) == 36 and all(q.maxsize == 1 for q in box.edges.values())
    box.edges[(4, "up")].put(b"", block=False)
    with pytest.raises(queue.Full):
        box.edges[(4, "up")].put(b"", block=False)


def test_the_rank_that_failed_first_names_the_cause():
    from mesh_threads import Mailbox, MeshError, run_ranks

    box = Mailbox(3, 1, timeout=3600.0)

    def body(rank):
        if rank == 1:
            raise ValueError("rank 1 is refused")
        box._take(rank, (1, "up" if rank == 0 else "down"), [0], [8], None)  # waits for rank 1, which never sends

    with pytest.raises(ValueError, match="rank 1 is refused"):
        run_ranks(box, body)

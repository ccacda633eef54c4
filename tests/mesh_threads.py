"""The ranks of a strip chain or a block mesh as THREADS of the test process: one process with the GPU open, ghost rows
and packed ghost columns through a mailbox in host memory (a queue.Queue per directed edge) behind the exchange
callbacks of capi.Strip and capi.Block.  ctypes releases the GIL inside ststhip_strip_advance and the callback takes it
again, so the ranks run side by side as processes would -- without the tens of seconds a process group costs.

Every wait is bounded: a get or put that is not served within `timeout` seconds raises, capi turns the exception into
an error status of the rank's advance, and the failed rank tells the others, which then stop waiting at once."""
import ctypes as C
import queue
import threading

import numpy as np

from stencilstream_amd import capi


class MeshError(RuntimeError):
    pass


class Mailbox:
    """One queue of one message per directed edge of a mesh_rows x mesh_cols mesh (a chain of strips: n x 1)."""

    def __init__(self, mesh_rows, mesh_cols=1, timeout=30.0):
        self.mesh_rows, self.mesh_cols, self.timeout = mesh_rows, mesh_cols, timeout
        self.failed = threading.Event()
        self.edges = {(rank, direction): queue.Queue(maxsize=1)
                      for rank in range(mesh_rows * mesh_cols) for direction in ("up", "down", "left", "right")}

    def _wait(self, what, rank, edge, n_bytes, action):
        """action(timeout) on a queue, in slices, so that a rank that has failed elsewhere ends the wait."""
        waited = 0.0
        while True:
            if self.failed.is_set():
                raise MeshError(f"rank {rank}: another rank has failed")
            try:
                return action(0.05)
            except (queue.Empty, queue.Full):
                waited += 0.05
                if waited >= self.timeout:
                    self.failed.set()
                    raise MeshError(f"rank {rank}: {what} on edge {edge[1]} of rank {edge[0]}: {n_bytes} bytes expected, "
                                    f"nothing within {self.timeout} s") from None

    def _put(self, rank, direction, pointers, sizes, stream):
        lib = capi.load()
        message = [C.create_string_buffer(n) for n in sizes]
        for buffer, ptr, n in zip(message, pointers, sizes):
            capi.check(lib.ststhip_memcpy_d2h(buffer, C.c_void_p(ptr), n, C.c_void_p(stream)), "ststhip_memcpy_d2h")
        capi.check(lib.ststhip_stream_synchronize(C.c_void_p(stream)), "ststhip_stream_synchronize")
        edge = (rank, direction)
        self._wait("put", rank, edge, sum(sizes), lambda t: self.edges[edge].put(message, timeout=t))

    def _take(self, rank, edge, pointers, sizes, stream):
        lib = capi.load()
        message = self._wait("get", rank, edge, sum(sizes), lambda t: self.edges[edge].get(timeout=t))
        if [len(b) for b in message] != list(sizes):
            self.failed.set()
            raise MeshError(f"rank {rank}: edge {edge[1]} of rank {edge[0]}: expected {list(sizes)} bytes, received "
                            f"{[len(b) for b in message]}")
        for buffer, ptr, n in zip(message, pointers, sizes):
            capi.check(lib.ststhip_memcpy_h2d(C.c_void_p(ptr), buffer, n, C.c_void_p(stream)), "ststhip_memcpy_h2d")
        capi.check(lib.ststhip_stream_synchronize(C.c_void_p(stream)), "ststhip_stream_synchronize")

    def _exchange(self, rank, first, second, to_first, to_second):
        """first / second: the neighbour ranks (None: the grid's edge); to_first / to_second: the edges' names"""
        def exchange(n_planes, send_first, send_second, recv_first, recv_second, row_bytes, n_rows, stream):
            sizes = [row_bytes[p] * n_rows for p in range(n_planes)]
            try:
                capi.check(capi.load().ststhip_stream_synchronize(C.c_void_p(stream)), "ststhip_stream_synchronize")
                if first is not None:
                    self._put(rank, to_first, send_first, sizes, stream)
                if second is not None:
                    self._put(rank, to_second, send_second, sizes, stream)
                if first is not None:
                    self._take(rank, (first, to_second), recv_first, sizes, stream)
                if second is not None:
                    self._take(rank, (second, to_first), recv_second, sizes, stream)
            except Exception:
                self.failed.set()
                raise
        return exchange

    def exchange_rows(self, rank):
        r = rank // self.mesh_cols
        return self._exchange(rank, rank - self.mesh_cols if r > 0 else None,
                              rank + self.mesh_cols if r + 1 < self.mesh_rows else None, "up", "down")

    def exchange_cols(self, rank):
        c = rank % self.mesh_cols
        return self._exchange(rank, rank - 1 if c > 0 else None, rank + 1 if c + 1 < self.mesh_cols else None,
                              "left", "right")


def run_ranks(mailbox, body, limit=120.0):
    """body(rank) in one thread per rank (at most 9); their results in rank order, or the first rank's exception."""
    n = mailbox.mesh_rows * mailbox.mesh_cols
    assert 1 <= n <= 9
    capi._sync_options()  # here, once: the ranks must not re-read the options while another one plans with them
    results, errors = [None] * n, [None] * n

    def rank_thread(rank):
        try:
            results[rank] = body(rank)
        except BaseException as e:  # noqa: BLE001 -- handed to the test
            errors[rank] = e
            mailbox.failed.set()

    threads = [threading.Thread(target=rank_thread, args=(rank,), daemon=True) for rank in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(limit)
        if t.is_alive():
            mailbox.failed.set()
            raise MeshError("a rank did not finish")
    # the rank that failed first names the cause; the others only report that it did
    causes = [e for e in errors if e is not None and "another rank has failed" not in str(e)]
    for e in causes + [e for e in errors if e is not None]:
        raise e
    return results


# ------------------------------------------------------------------ cells <-> the planes of a registered function
def split_planes(info, cells):
    """The planes ststhip_app_info describes (plane p: bytes [field_offset[p], + plane_elem_size[p]) of every cell) of
    an H x W array of cells, each as an H x (W * element size) array of bytes."""
    h, w = cells.shape
    raw = np.ascontiguousarray(cells).view(np.uint8).reshape(h, w, info.cell_size)
    return [np.ascontiguousarray(raw[:, :, info.field_offset[p]:info.field_offset[p] + info.plane_elem_size[p]])
            .reshape(h, w * info.plane_elem_size[p]) for p in range(info.n_planes)]


def join_planes(info, planes, dtype, template):
    """The inverse; bytes no plane holds (padding) come from `template`, an array of cells of the same shape."""
    h, w = template.shape
    raw = np.ascontiguousarray(template).view(np.uint8).reshape(h, w, info.cell_size).copy()
    for p, plane in enumerate(planes):
        size = info.plane_elem_size[p]
        raw[:, :, info.field_offset[p]:info.field_offset[p] + size] = np.asarray(plane).view(np.uint8).reshape(h, w, size)
    return raw.reshape(h, w * info.cell_size).view(dtype).reshape(h, w)


def run_decomposed(app, tf_params, halo_bytes, cells, calls, mesh=None, n_strips=None, timeout=30.0):
    """`cells` (H x W, the app's cell dtype) through capi.Strip on n_strips ranks or capi.Block on a mesh of
    (mesh_rows, mesh_cols) ranks, `calls` = [(iteration_offset, n_generations), ...] advance calls; returns the
    assembled grid and every rank's (launches, exchanges)."""
    info = capi.app_info(app)
    h, w = cells.shape
    mesh_rows, mesh_cols = (n_strips, 1) if mesh is None else mesh
    mailbox = Mailbox(mesh_rows, mesh_cols, timeout)
    out = cells.copy()
    alone = mesh_rows * mesh_cols == 1

    def body(rank):
        rows_cb = None if alone else mailbox.exchange_rows(rank)
        if mesh is None:
            part = capi.Strip(app, tf_params, halo_bytes, h, w, rank, n_strips, exchange=rows_cb)
            rs, cs = slice(part.row_begin, part.row_end), slice(0, w)
        else:
            part = capi.Block(app, tf_params, halo_bytes, h, w, rank, mesh_rows, mesh_cols, exchange_rows=rows_cb,
                              exchange_cols=None if alone else mailbox.exchange_cols(rank))
            rs, cs = slice(part.row_begin, part.row_end), slice(part.col_begin, part.col_end)
        try:
            mine = np.ascontiguousarray(cells[rs, cs])
            for p, plane in enumerate(split_planes(info, mine)):
                part.upload(p, plane)
            for i, (offset, n) in enumerate(calls):
                part.advance(offset, n, blocking=i + 1 == len(calls))
            planes = [part.download(p, np.dtype(f"V{info.plane_elem_size[p]}")) for p in range(info.n_planes)]
            out[rs, cs] = join_planes(info, planes, cells.dtype, mine)
            return part.counters()
        finally:
            part.close()

    return out, run_ranks(mailbox, body)

"""Python mirror of stencil::hip::Grid / stencil::hip::StencilUpdate for the precompiled
transition functions (reference interface: StencilStream/cuda/Grid.hpp:50-188,
StencilStream/cuda/StencilUpdate.hpp:41-198).  Device memory and streams are torch's; every sweep
runs in libststhip.so through the C ABI.
"""
import ctypes as C
import time
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np
import torch

from . import capi


@dataclass
class TransitionFunction:
    """A precompiled transition function: registry name + its parameter block."""

    app: str
    params: C.Structure = field(default_factory=capi.NoParams)
    cell_dtype: np.dtype = None  # numpy dtype of one AoS cell

    def info(self):
        return capi.app_info(self.app)


def jacobi(variant="Jacobi5General", coef=()):
    p = capi.JacobiParams()
    for i, c in enumerate(coef):
        p.coef[i] = float(np.float32(c))
    return TransitionFunction(variant.lower(), p, np.dtype("<f4"))


HOTSPOT_CELL = np.dtype([("temp", "<f4"), ("power", "<f4")])
SELFCHECK_CELL = np.dtype(
    [("r", "<i4"), ("c", "<i4"), ("i_iteration", "<i4"), ("i_subiteration", "<i4"), ("status", "<i4")]
)
FDTD_CELL = np.dtype([(n, "<f4") for n in ("ex", "ey", "hz", "hz_sum", "ca", "cb", "da", "db")])


def hotspot(Rx_1, Ry_1, Rz_1, Cap_1, split_cell_structure=True):
    p = capi.HotspotParams(Rx_1, Ry_1, Rz_1, Cap_1)
    return TransitionFunction("hotspot" if split_cell_structure else "hotspot_aos", p, HOTSPOT_CELL)


HOTSPOT_CELL_F64 = np.dtype([("temp", "<f8"), ("power", "<f8")])


def hotspot_f64(Rx_1, Ry_1, Rz_1, Cap_1, split_cell_structure=True):
    """HotSpot with the reference's formula evaluated in fp64 (the reference itself is fp32)."""
    p = capi.HotspotParamsF64(Rx_1, Ry_1, Rz_1, Cap_1)
    return TransitionFunction("hotspot_f64" if split_cell_structure else "hotspot_f64_aos", p, HOTSPOT_CELL_F64)


def conway():
    return TransitionFunction("conway", capi.NoParams(), np.dtype("u1"))


def selfcheck(radius=1, split_cell_structure=False):
    name = f"selfcheck{radius}" + ("_soa" if split_cell_structure else "")
    return TransitionFunction(name, capi.NoParams(), SELFCHECK_CELL)


def fdtd(params, split_cell_structure=True, layout=None):
    """layout: "grouped" (two planes of 16 bytes: fields / material coefficients; the fastest, default for a split
    request), "planes" (one plane per field, the reference's SoA protocol) or "aos"."""
    if layout is None:
        layout = "grouped" if split_cell_structure else "aos"
    app = {"grouped": "fdtd_coef_grouped", "planes": "fdtd_coef", "aos": "fdtd_coef_aos"}[layout]
    return TransitionFunction(app, params, FDTD_CELL)


# What Grid.norms returns per field (ststhip_norm_result): over the cells of the rectangle whose value v is finite,
# max |v| (-inf if there is none) and the sums of v, |v| and v*v in double; n_nonfinite counts the others.
Norms = namedtuple("Norms", "n_cells n_nonfinite max_abs sum sum_abs sum_sq")
# the sums of a*b, a*a and b*b in double over the cells where both are finite; n_nonfinite counts the others.
Dot = namedtuple("Dot", "n_cells n_nonfinite dot sum_aa sum_bb")


class Grid:
    """H x W row-major AoS cells in HBM (a torch uint8 tensor of H*W*cell_size bytes)."""

    dimensions = 2

    def __init__(self, height, width, cell_dtype, device=None, _cells=None):
        self.cell_dtype = np.dtype(cell_dtype)
        self.height, self.width = int(height), int(width)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        n = self.height * self.width * self.cell_dtype.itemsize
        self.cells = _cells if _cells is not None else torch.zeros(max(n, 1), dtype=torch.uint8, device=self.device)

    @classmethod
    def from_numpy(cls, array, device=None):
        array = np.ascontiguousarray(array)
        assert array.ndim == 2
        g = cls(array.shape[0], array.shape[1], array.dtype, device)
        g.copy_from_buffer(array)
        return g

    def copy_from_buffer(self, array):
        array = np.ascontiguousarray(array)
        if array.shape != (self.height, self.width):
            raise ValueError("The target buffer has not the same size as the grid")
        if self.cell_dtype == np.dtype("u1") and array.dtype != np.bool_ and array.size and int(array.max()) > 1:
            # one-byte cells are the C++ `bool` cells of the Game of Life (examples/conway/conway.cpp:35):
            # bytes 0 / 1 only.  The kernel on words of four cells relies on it (ststhip.h, ststhip_app_run)
            raise ValueError("one-byte cells are C++ bools: every byte must be 0 or 1")
        raw = torch.from_numpy(array.view(np.uint8).reshape(-1).copy())
        if raw.numel():
            self.cells[: raw.numel()].copy_(raw)

    def copy_to_buffer(self, array):
        if array.shape != (self.height, self.width):
            raise ValueError("The target buffer has not the same size as the grid")
        array[...] = self.to_numpy()

    def to_numpy(self):
        n = self.height * self.width * self.cell_dtype.itemsize
        host = self.cells[:n].cpu().numpy()
        return host.view(self.cell_dtype).reshape(self.height, self.width).copy()

    def get_grid_height(self):
        return self.height

    def get_grid_width(self):
        return self.width

    def get_grid_range(self):
        return (self.height, self.width)

    def make_similar(self):
        return Grid(self.height, self.width, self.cell_dtype, self.device)

    def domain(self):
        return capi.Domain(self.height, self.width, 0, self.height, self.width)

    def norms(self, fields=None, other=None, rows=None, cols=None):
        """Norms of the grid's float fields, computed where the cells are (ststhip_grid_norms): {field name: Norms}, the
        key is None for a grid whose cells are plain floats.  `fields`: names of `<f4` / `<f8` members of the cell
        (default: all of them); `other`: a grid of the same extent and cell type, the values are then this grid's minus
        the other's, in double (ststhip_grid_distance); rows / cols = (begin, end), clipped to the grid.  Blocks until
        the numbers are known.  A run that has converged shows in norms(other=previous)[name].max_abs; one that has
        diverged in n_nonfinite."""
        dt = self.cell_dtype
        if dt.names is None:
            if fields is not None and list(fields) != [None]:
                raise ValueError("the cells of this grid have no named fields")
            members = [(None, dt, 0)]
        else:
            floats = [n for n in dt.names if dt.fields[n][0].str in ("<f4", "<f8")]
            names = floats if fields is None else ([fields] if isinstance(fields, str) else list(fields))
            for n in names:
                if n not in dt.names:
                    raise ValueError(f"the cell has no field {n!r}")
            members = [(n, dt.fields[n][0], dt.fields[n][1]) for n in names]
        for name, kind, _ in members:
            if kind.str not in ("<f4", "<f8"):
                raise ValueError(f"field {name!r} is {kind}: norms reduce <f4 and <f8 fields")
        if not 1 <= len(members) <= 8:
            raise ValueError("norms reduce 1 to 8 fields per call")
        if other is not None and ((other.height, other.width) != (self.height, self.width) or other.cell_dtype != dt):
            raise ValueError("the other grid has not the same size and cell type as the grid")
        capi.init(self.device.index if self.device.index is not None else -1)
        with capi.on_stream(self.device) as torch_stream:
            base = self.cells.data_ptr()
            table = [capi.norm_field(base + offset, kind.str, dt.itemsize, self.height, self.width, rows=rows, cols=cols)
                     for _, kind, offset in members]
            there = None if other is None else [other.cells.data_ptr() + offset for _, _, offset in members]
            result = capi.grid_norms(table, there, stream=torch_stream.cuda_stream)
        return {name: Norms(r.n_cells, r.n_nonfinite, r.max_abs, r.sum, r.sum_abs, r.sum_sq)
                for (name, _, _), r in zip(members, result)}

    # ---- parts of the grid, moved where the cells are (ststhip_grid_download / _upload / _fill / _copy) ----
    @staticmethod
    def _axis(given, extent, what):
        """(begin, end) of a range of rows or columns; None = the whole axis.  Nothing is clipped."""
        begin, end = (0, extent) if given is None else (int(given[0]), int(given[1]))
        if not 0 <= begin <= end <= extent:
            raise ValueError(f"{what} {begin}:{end} leave the grid ({extent})")
        return begin, end

    @staticmethod
    def _steps(step):
        rows, cols = int(step[0]), int(step[1])
        if rows < 1 or cols < 1:
            raise ValueError("a step is 1 or more")
        return rows, cols

    def _element(self, field):
        """(dtype, byte offset in the cell) of what a region call moves: the whole cell, or the member `field`."""
        if field is None:
            return self.cell_dtype, 0
        if self.cell_dtype.names is None or field not in self.cell_dtype.names:
            raise ValueError(f"the cell has no field {field!r}")
        return self.cell_dtype.fields[field][0], self.cell_dtype.fields[field][1]

    def _view(self, offset=0):
        return capi.grid_view(self.cells.data_ptr() + offset, self.cell_dtype.itemsize, self.height, self.width)

    def _on_device(self):
        capi.init(self.device.index if self.device.index is not None else -1)
        return capi.on_stream(self.device)

    def read(self, rows=None, cols=None, step=(1, 1), field=None):
        """The cells of rows[0]:rows[1]:step[0], cols[0]:cols[1]:step[1] (None = the whole axis), or their member
        `field`, as a numpy array -- what to_numpy()[r0:r1:sr, c0:c1:sc] (or that [field]) holds, without bringing
        the rest of the grid to the host.  A range that leaves the grid raises ValueError."""
        (r0, r1), (c0, c1) = self._axis(rows, self.height, "rows"), self._axis(cols, self.width, "columns")
        sr, sc = self._steps(step)
        kind, offset = self._element(field)
        n_rows, n_cols = -(-(r1 - r0) // sr), -(-(c1 - c0) // sc)
        out = np.empty((n_rows, n_cols), dtype=kind)
        if out.size:
            with self._on_device() as torch_stream:
                host = capi.grid_view(out.ctypes.data, kind.itemsize, n_rows, n_cols)
                capi.grid_download([capi.grid_copy_desc(host, self._view(offset), kind.itemsize, n_rows, n_cols,
                                                        src_at=(r0, c0), step=(sr, sc))], torch_stream.cuda_stream)
        return out

    def write(self, array, at=(0, 0), field=None):
        """array (2-D, the cell's dtype or the member's) into the cells from (at[0], at[1]) on, or into their member
        `field`; the other members keep their bytes.  The array may be reused when the call returns."""
        kind, offset = self._element(field)
        array = np.ascontiguousarray(array, dtype=kind)
        if array.ndim != 2:
            raise ValueError("a region is two-dimensional")
        r0, c0 = int(at[0]), int(at[1])
        self._axis((r0, r0 + array.shape[0]), self.height, "rows")
        self._axis((c0, c0 + array.shape[1]), self.width, "columns")
        if array.size:
            with self._on_device() as torch_stream:
                host = capi.grid_view(array.ctypes.data, kind.itemsize, array.shape[0], array.shape[1])
                capi.grid_upload([capi.grid_copy_desc(self._view(offset), host, kind.itemsize, array.shape[0],
                                                      array.shape[1], dst_at=(r0, c0))], torch_stream.cuda_stream)

    def fill(self, value, rows=None, cols=None, field=None):
        """One value (a cell, or a member `field`) into every cell of rows[0]:rows[1], cols[0]:cols[1]; its bytes
        arrive as they are (NaN payloads, -0.0).  Queued behind the work on the grid; does not wait."""
        (r0, r1), (c0, c1) = self._axis(rows, self.height, "rows"), self._axis(cols, self.width, "columns")
        kind, offset = self._element(field)
        cell = np.zeros((), dtype=kind)
        cell[...] = value
        if r1 > r0 and c1 > c0:
            with self._on_device() as torch_stream:
                capi.grid_fill([capi.grid_fill_desc(self._view(offset), cell.tobytes(), r1 - r0, c1 - c0,
                                                    dst_at=(r0, c0))], torch_stream.cuda_stream)

    def paste(self, source, rows=None, cols=None, at=(0, 0), step=(1, 1)):
        """The cells rows[0]:rows[1]:step[0], cols[0]:cols[1]:step[1] of grid `source` (same cell type) into this grid
        from (at[0], at[1]) on, device to device.  Queued; does not wait."""
        if source.cell_dtype != self.cell_dtype:
            raise ValueError("the source grid has not the same cell type as the grid")
        (r0, r1), (c0, c1) = source._axis(rows, source.height, "rows"), source._axis(cols, source.width, "columns")
        sr, sc = self._steps(step)
        n_rows, n_cols = -(-(r1 - r0) // sr), -(-(c1 - c0) // sc)
        a0, a1 = int(at[0]), int(at[1])
        self._axis((a0, a0 + n_rows), self.height, "rows")
        self._axis((a1, a1 + n_cols), self.width, "columns")
        if n_rows and n_cols:
            with self._on_device() as torch_stream:
                capi.grid_copy([capi.grid_copy_desc(self._view(), source._view(), self.cell_dtype.itemsize, n_rows,
                                                    n_cols, dst_at=(a0, a1), src_at=(r0, c0), step=(sr, sc))],
                               torch_stream.cuda_stream)

    # ---- computing with grids where the cells are (ststhip_grid_combine / ststhip_grid_resample) ----
    def _float_element(self, field):
        """(dtype, byte offset in the cell) of the float a grid-algebra call computes with: the member `field`, or the
        cell itself where cells are plain floats."""
        kind, offset = self._element(field)
        if kind.str not in ("<f4", "<f8"):
            what = "the cells are" if field is None else f"field {field!r} is"
            raise ValueError(f"{what} {kind}: the grid algebra computes with <f4 and <f8 elements")
        return kind, offset

    def combine(self, terms, field=None, rows=None, cols=None):
        """this[field] = coef_0 * x_0 (+ coef_1 * x_1 ...) over rows[0]:rows[1], cols[0]:cols[1] (None = the whole
        axis).  `terms`: one to four (coef, grid) or (coef, grid, field) of grids of this grid's extent (any cell type)
        whose element has this element's dtype; the same rectangle applies to all.  Every product and every sum is
        rounded once in that dtype, left to right, so numpy in the same dtype gives the same bits.  A term may be this
        grid's own element (in place) or another member of its cells.  Queued; does not wait."""
        kind, offset = self._float_element(field)
        terms = [tuple(t) for t in terms]
        if not 1 <= len(terms) <= 4:
            raise ValueError("a combine takes 1 to 4 terms")
        (r0, r1), (c0, c1) = self._axis(rows, self.height, "rows"), self._axis(cols, self.width, "columns")
        sources = []
        for term in terms:
            if len(term) not in (2, 3):
                raise ValueError("a term is (coef, grid) or (coef, grid, field)")
            grid, its_field = term[1], (term[2] if len(term) == 3 else None)
            if (grid.height, grid.width) != (self.height, self.width):
                raise ValueError("a term's grid has not the same size as the grid")
            its_kind, its_offset = grid._float_element(its_field)
            if its_kind != kind:
                raise ValueError(f"a term's element is {its_kind}, the destination's {kind}")
            sources.append((float(term[0]), grid, its_offset))
        if r1 > r0 and c1 > c0:
            with self._on_device() as torch_stream:
                table = [(coef, grid._view(its_offset), (r0, c0)) for coef, grid, its_offset in sources]
                capi.grid_combine([capi.grid_combine_desc(self._view(offset), kind.str, table, r1 - r0, c1 - c0,
                                                          dst_at=(r0, c0))], torch_stream.cuda_stream)

    def _transfer(self, other, mode, coarse, fine, field, src_field, halo):
        kind, offset = self._float_element(field)
        its_kind, its_offset = other._float_element(src_field)
        if its_kind != kind:
            raise ValueError(f"the source's element is {its_kind}, the destination's {kind}")
        if (fine.height, fine.width) != (2 * coarse.height, 2 * coarse.width):
            raise ValueError(f"the fine grid ({fine.height} x {fine.width}) has not twice the extents of the coarse "
                             f"one ({coarse.height} x {coarse.width})")
        if coarse.height and coarse.width:
            with self._on_device() as torch_stream:
                capi.grid_resample([capi.grid_resample_desc(self._view(offset), other._view(its_offset), kind.str, mode,
                                                            coarse.height, coarse.width, halo=halo)],
                                   torch_stream.cuda_stream)

    def restrict_from(self, fine, field=None, src_field=None):
        """This (coarse) grid's element becomes the mean of the 2 x 2 cells of `fine`, whose extents are twice this
        grid's: ((s(2i,2j) + s(2i,2j+1)) + (s(2i+1,2j) + s(2i+1,2j+1))) * 0.25, one rounding each.  Queued."""
        self._transfer(fine, capi.RESTRICT_MEAN, self, fine, field, src_field, 0.0)

    def prolong_from(self, coarse, halo=0.0, field=None, src_field=None):
        """This (fine) grid's element becomes the cell-centred bilinear interpolation (weights 0.75 / 0.25 per axis) of
        `coarse`, whose extents are half this grid's; a neighbour outside the coarse grid reads `halo`.  Queued."""
        self._transfer(coarse, capi.PROLONG_BILINEAR, coarse, self, field, src_field, float(halo))

    # ---- a 3 x 3 linear operator applied once (ststhip_grid_stencil) ----
    def apply_stencil(self, src, *, box=None, cross=None, halo=0.0, rhs=None, rhs_coef=1.0, field=None, src_field=None,
                      rhs_field=None, rows=None, cols=None):
        """this[field] = sum of w(a, b) * src[src_field](i + a, j + b) (+ rhs_coef * rhs[rhs_field](i, j)) over
        rows[0]:rows[1], cols[0]:cols[1] (None = the whole axis); the same rectangle applies to all three grids, which
        have this grid's extents (any cell type) and elements of this element's dtype.  Exactly one of `box` (3 x 3
        weights, row-major: all nine taps, also those whose weight is zero) and `cross` ((n, w, c, e, s): five taps,
        the corners are not read) is given; the shape is never inferred from zeros.  The taps are taken in row-major
        order, acc = w_first * s_first, then acc = acc + w_k * s_k, then the right-hand side: every product and every
        sum is rounded once in that dtype, so numpy in the same dtype gives the same bits.  A neighbour outside the
        GRID reads `halo`, one outside the rectangle reads the grid.  `src` may be another member of this grid's cells
        but not the destination itself; `rhs` may be either.  A residual r = f - A u: weights -A, rhs=f; a relaxation
        with a source: cross=(.25, .25, 0, .25, .25), rhs=f, rhs_coef=h*h/4.  Queued; does not wait."""
        kind, offset = self._float_element(field)
        if (box is None) == (cross is None):
            raise ValueError("a stencil is given as box= (3 x 3 weights) or as cross= (n, w, c, e, s), one of the two")
        if box is not None:
            weights = np.asarray(box, dtype=np.float64)
            if weights.shape != (3, 3):
                raise ValueError(f"box= takes 3 x 3 weights, not an array of shape {weights.shape}")
            shape, weights = capi.STENCIL_BOX9, [float(w) for w in weights.reshape(-1)]
        else:
            taps = np.asarray(cross, dtype=np.float64)
            if taps.shape != (5,):
                raise ValueError(f"cross= takes five weights (n, w, c, e, s), not an array of shape {taps.shape}")
            n, w, c, e, s = (float(t) for t in taps)
            shape, weights = capi.STENCIL_CROSS5, [0.0, n, 0.0, w, c, e, 0.0, s, 0.0]
        if not np.all(np.isfinite(weights)):
            raise ValueError("a weight of the stencil is not finite")
        (r0, r1), (c0, c1) = self._axis(rows, self.height, "rows"), self._axis(cols, self.width, "columns")
        others = [("the source", src, src_field)]
        if rhs is not None:
            others.append(("the right-hand side", rhs, rhs_field))
            if not np.isfinite(float(rhs_coef)):
                raise ValueError("rhs_coef is not finite")
        elif rhs_field is not None:
            raise ValueError("rhs_field names a member of a right-hand side that is not given")
        views = []
        for what, grid, its_field in others:
            if (grid.height, grid.width) != (self.height, self.width):
                raise ValueError(f"{what}'s grid has not the same size as the grid")
            its_kind, its_offset = grid._float_element(its_field)
            if its_kind != kind:
                raise ValueError(f"{what}'s element is {its_kind}, the destination's {kind}")
            views.append((grid, its_offset))
        if views[0][0].cells.data_ptr() == self.cells.data_ptr() and views[0][1] == offset:
            raise ValueError("the source is the destination itself: a stencil in place is a race")
        if r1 > r0 and c1 > c0:
            with self._on_device() as torch_stream:
                f = None if rhs is None else views[1][0]._view(views[1][1])
                capi.grid_stencil([capi.grid_stencil_desc(self._view(offset), views[0][0]._view(views[0][1]), kind.str,
                                                          shape, weights, r1 - r0, c1 - c0, (r0, c0), (r0, c0),
                                                          float(halo), f, float(rhs_coef), (r0, c0))],
                                  torch_stream.cuda_stream)

    # ---- red-black relaxation in place (ststhip_grid_relax) ----
    def relax(self, *, cross, halo=0.0, rhs=None, rhs_coef=1.0, field=None, rhs_field=None, rows=None, cols=None,
              first_colour=0, half_sweeps=2, parity=0):
        """`half_sweeps` red-black half-sweeps of this[field] IN PLACE over rows[0]:rows[1], cols[0]:cols[1] (None = the
        whole axis).  Cell (r, q) of the GRID has the colour (r + q + parity) & 1, whatever the rectangle; half-sweep k
        updates the rectangle's cells of colour (first_colour + k) & 1 with the five taps cross = (n, w, c, e, s) in
        that order, acc = n * N, then acc = acc + w * W ..., then + rhs_coef * rhs[rhs_field](i, j): every product and
        every sum is rounded once in the element's dtype, so numpy in the same dtype gives the same bits.  The four
        neighbours of a cell have the other colour, so nothing is read that the same half-sweep writes.  A neighbour
        outside the GRID reads `halo`, one outside the rectangle reads the grid.  `rhs` has this grid's extents and may be
        another member of this grid's cells, never the relaxed element itself.  Gauss-Seidel for
        (4u - N - W - E - S) / h^2 = f: cross=(.25, .25, 0, .25, .25), rhs=f, rhs_coef=h*h/4; SOR with factor w:
        cross=(w/4, w/4, 1 - w, w/4, w/4), rhs_coef=w*h*h/4.  Queued; does not wait."""
        kind, offset = self._float_element(field)
        taps = np.asarray(cross, dtype=np.float64)
        if taps.shape != (5,):
            raise ValueError(f"cross= takes five weights (n, w, c, e, s), not an array of shape {taps.shape}")
        if not np.all(np.isfinite(taps)):
            raise ValueError("a weight of the relaxation is not finite")
        for what, value, allowed in (("first_colour", first_colour, (0, 1)), ("parity", parity, (0, 1)),
                                     ("half_sweeps", half_sweeps, range(1, 1025))):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value not in allowed:
                raise ValueError(f"{what} is {value!r}: it takes {allowed[0]} to {allowed[-1]}")
        (r0, r1), (c0, c1) = self._axis(rows, self.height, "rows"), self._axis(cols, self.width, "columns")
        its_offset = None
        if rhs is not None:
            if not np.isfinite(float(rhs_coef)):
                raise ValueError("rhs_coef is not finite")
            if (rhs.height, rhs.width) != (self.height, self.width):
                raise ValueError("the right-hand side's grid has not the same size as the grid")
            its_kind, its_offset = rhs._float_element(rhs_field)
            if its_kind != kind:
                raise ValueError(f"the right-hand side's element is {its_kind}, the relaxed one {kind}")
            if rhs.cells.data_ptr() == self.cells.data_ptr() and its_offset == offset:
                raise ValueError("the right-hand side is the relaxed element itself")
        elif rhs_field is not None:
            raise ValueError("rhs_field names a member of a right-hand side that is not given")
        if r1 > r0 and c1 > c0:
            with self._on_device() as torch_stream:
                f = None if rhs is None else rhs._view(its_offset)
                capi.grid_relax([capi.grid_relax_desc(self._view(offset), kind.str, [float(t) for t in taps], r1 - r0,
                                                      c1 - c0, (r0, c0), float(halo), f, float(rhs_coef), (r0, c0),
                                                      int(first_colour), int(half_sweeps), int(parity))],
                                torch_stream.cuda_stream)

    # ---- the five-point operator with face coefficients in two grids (ststhip_grid_diffusion) ----
    def diffusion(self, src, kx, ky, *, mode="apply", sigma=0.0, scale=1.0, omega=1.0, halo=0.0, k_halo=0.0, rhs=None,
                  rhs_coef=1.0, field=None, src_field=None, kx_field=None, ky_field=None, rhs_field=None, rows=None,
                  cols=None):
        """The finite-volume operator A u = sigma u + scale * sum of k (u_c - u_neighbour) over the four faces of a
        cell, with the face coefficients in two grids: kx[kx_field](i, j) is the EAST face of cell (i, j),
        ky[ky_field](i, j) its SOUTH face; the west face is kx(i, j-1), the north face ky(i-1, j).  Over rows[0]:rows[1],
        cols[0]:cols[1] (None = the whole axis; one rectangle applies to all grids, which have this grid's extents, any
        cell type and elements of this element's dtype):
            acc = kn*(c-n); acc = acc + kw*(c-w); acc = acc + ke*(c-e); acc = acc + ks*(c-s)
            d = sigma + scale*(((kn + kw) + ke) + ks)
            mode="apply":       this[field] = sigma*c + scale*acc (+ rhs_coef * rhs)
            mode="jacobi":      this[field] = c + omega * ((rhs_coef*rhs - (sigma*c + scale*acc)) / d)
            mode="solve_diag":  this[field] = (rhs_coef * rhs) / d          (src may be None; a src and src_field
                                                                             that are given are ignored, unchecked)
        Every operation is rounded once in that dtype and `/` is the IEEE quotient, so numpy in the same dtype gives
        the same bits.  A neighbour of `src` outside the GRID reads `halo`; the west face of column 0 and the north face
        of row 0 read `k_halo`.  "jacobi" and "solve_diag" need `rhs`.  `src`, `kx` and `ky` may be other members of this
        grid's cells but not the destination itself; `rhs` may be either.  Queued; does not wait."""
        kind, offset = self._float_element(field)
        modes = {"apply": capi.DIFFUSION_APPLY, "jacobi": capi.DIFFUSION_JACOBI, "solve_diag": capi.DIFFUSION_SOLVE_DIAG}
        if mode not in modes:
            raise ValueError(f"mode is {mode!r}: it takes 'apply', 'jacobi' or 'solve_diag'")
        if mode != "apply" and rhs is None:
            raise ValueError(f"mode {mode!r} needs a right-hand side")
        if src is None and mode != "solve_diag":
            raise ValueError(f"mode {mode!r} needs a source; only 'solve_diag' reads none")
        if src is None and src_field is not None:
            raise ValueError("src_field names a member of a source that is not given")
        for what, value, read in (("sigma", sigma, True), ("scale", scale, True), ("omega", omega, mode == "jacobi"),
                                  ("rhs_coef", rhs_coef, rhs is not None)):
            if read and not np.isfinite(float(value)):
                raise ValueError(f"{what} is not finite")
        (r0, r1), (c0, c1) = self._axis(rows, self.height, "rows"), self._axis(cols, self.width, "columns")
        others = [("the east faces", kx, kx_field), ("the south faces", ky, ky_field)]
        if mode != "solve_diag":
            others.append(("the source", src, src_field))
        if rhs is not None:
            others.append(("the right-hand side", rhs, rhs_field))
        elif rhs_field is not None:
            raise ValueError("rhs_field names a member of a right-hand side that is not given")
        views = {}
        for what, grid, its_field in others:
            if (grid.height, grid.width) != (self.height, self.width):
                raise ValueError(f"{what}'s grid has not the same size as the grid")
            its_kind, its_offset = grid._float_element(its_field)
            if its_kind != kind:
                raise ValueError(f"{what}'s element is {its_kind}, the destination's {kind}")
            if what != "the right-hand side" and grid.cells.data_ptr() == self.cells.data_ptr() and its_offset == offset:
                raise ValueError(f"{what} is the destination itself: an operator in place is a race")
            views[what] = grid._view(its_offset)
        if r1 > r0 and c1 > c0:
            with self._on_device() as torch_stream:
                at = (r0, c0)
                capi.grid_diffusion([capi.grid_diffusion_desc(
                    self._view(offset), views.get("the source"), views["the east faces"], views["the south faces"],
                    kind.str, modes[mode], r1 - r0, c1 - c0, at, at, at, at, float(sigma), float(scale), float(omega),
                    float(halo), float(k_halo), views.get("the right-hand side"), float(rhs_coef), at)],
                    torch_stream.cuda_stream)

    # ---- the inner product of two grids (ststhip_grid_dot) ----
    def dot(self, other=None, field=None, other_field=None, rows=None, cols=None, other_at=None):
        """Dot(n_cells, n_nonfinite, dot, sum_aa, sum_bb): the sums of a * b, a * a and b * b in double over
        rows[0]:rows[1], cols[0]:cols[1] of this grid (None = the whole axis), where a is this grid's element `field`
        and b the element `other_field` of `other` (any extent, any cell type, the same element dtype) in the
        rectangle of the same size that begins at other_at = (row, col); the default is the same place.  other=None is
        this grid itself: with `other_field`, two members of the same cells; without, a . a, whose three sums are the
        same bits.  Cells where a or b is NaN or infinite are counted in n_nonfinite and left out of the sums.  Nothing
        is clipped: a rectangle that leaves either grid raises ValueError.  Blocks until the numbers are known; the
        same call on the same data returns the same bits, and dot(a, b).dot == dot(b, a).dot."""
        kind, offset = self._float_element(field)
        there = self if other is None else other
        its_kind, its_offset = there._float_element(field if other is None and other_field is None else other_field)
        if its_kind != kind:
            raise ValueError(f"the other element is {its_kind}, this one {kind}")
        (r0, r1), (c0, c1) = self._axis(rows, self.height, "rows"), self._axis(cols, self.width, "columns")
        o0, o1 = (r0, c0) if other_at is None else (int(other_at[0]), int(other_at[1]))
        there._axis((o0, o0 + (r1 - r0)), there.height, "rows of the other grid")
        there._axis((o1, o1 + (c1 - c0)), there.width, "columns of the other grid")
        if r1 == r0 or c1 == c0:
            return Dot(0, 0, 0.0, 0.0, 0.0)
        with self._on_device() as torch_stream:
            r = capi.grid_dot([capi.grid_dot_desc(self._view(offset), there._view(its_offset), kind.str, r1 - r0,
                                                  c1 - c0, (r0, c0), (o0, o1))], torch_stream.cuda_stream)[0]
        return Dot(r.n_cells, r.n_nonfinite, r.dot, r.sum_aa, r.sum_bb)


@dataclass
class Params:
    """Same fields and order as cuda::StencilUpdate::Params (cuda/StencilUpdate.hpp:54-105)."""

    transition_function: TransitionFunction
    halo_value: object = None  # one cell (numpy scalar / tuple); default = zero-initialised Cell()
    iteration_offset: int = 0
    n_iterations: int = 1
    device: object = None
    blocking: bool = False
    profiling: bool = False


class StencilUpdate:
    def __init__(self, params):
        self.params = params
        self.n_processed_cells = 0
        self.walltime = 0.0
        self.kernel_runtime = 0.0
        self.info = params.transition_function.info()

    def get_params(self):
        return self.params

    def get_n_processed_cells(self):
        return self.n_processed_cells

    def get_walltime(self):
        return self.walltime

    def get_kernel_runtime(self):
        return self.kernel_runtime

    def _halo_bytes(self):
        dt = self.params.transition_function.cell_dtype
        cell = np.zeros((), dtype=dt)
        if self.params.halo_value is not None:
            cell[...] = self.params.halo_value
        return cell.tobytes()

    def __call__(self, source):
        p = self.params
        tf = p.transition_function
        info = self.info
        if source.cell_dtype.itemsize != info.cell_size:
            raise ValueError("grid cell type does not match the transition function")
        if p.n_iterations == 0:
            return source  # handle onto the same cells, as the reference's AoS path
        capi.init(source.device.index if source.device.index is not None else -1)
        started = time.perf_counter()
        with capi.on_stream(source.device) as torch_stream:
            result, run = self._run(source, torch_stream)
        self.walltime += time.perf_counter() - started
        self.kernel_runtime += run.kernel_time_s
        self.n_processed_cells += p.n_iterations * source.height * source.width
        return result

    def _run(self, source, torch_stream):
        p = self.params
        tf = p.transition_function
        info = self.info
        stream = torch_stream.cuda_stream

        result = source.make_similar()
        dom = source.domain()
        n_cells = source.height * source.width
        if info.n_planes == 1:
            run = capi.app_run(tf.app, tf.params, self._halo_bytes(), dom, [source.cells.data_ptr()],
                               [result.cells.data_ptr()], p.iteration_offset, p.n_iterations,
                               blocking=p.blocking, profiling=p.profiling, stream=stream)
        else:
            n = info.n_planes
            sizes = [info.plane_elem_size[i] for i in range(n)]
            offsets = [info.field_offset[i] for i in range(n)]
            a = [torch.empty(max(n_cells * s, 1), dtype=torch.uint8, device=source.device) for s in sizes]
            b = [torch.empty(max(n_cells * s, 1), dtype=torch.uint8, device=source.device) for s in sizes]
            capi.scatter_fields(source.cells.data_ptr(), info.cell_size, n_cells, offsets, sizes,
                                [t.data_ptr() for t in a], stream)
            run = capi.app_run(tf.app, tf.params, self._halo_bytes(), dom, [t.data_ptr() for t in a],
                               [t.data_ptr() for t in b], p.iteration_offset, p.n_iterations,
                               blocking=False, profiling=p.profiling, stream=stream)
            capi.gather_fields(result.cells.data_ptr(), info.cell_size, n_cells, offsets, sizes,
                               [t.data_ptr() for t in b], stream)
            for t in a + b:
                t.record_stream(torch_stream)
            if p.blocking:
                torch_stream.synchronize()
        result.cells.record_stream(torch_stream)
        return result, run

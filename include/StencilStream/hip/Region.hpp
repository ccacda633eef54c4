// Parts of a stencil::hip::Grid, moved where the cells are -- an EXTENSION of the reference's API.  Its only way to the
// cells of a grid is the GridAccessor, and that moves the whole grid: constructing one downloads every byte of every
// cell, and a writing one makes the next StencilUpdate upload the whole grid again.  An application that looks at its
// grid, or nudges it, BETWEEN two update calls asks for the part it needs instead.  The FDTD example's save_frame
// (examples/fdtd/src/fdtd.cpp:114-116: a read accessor on a grid of 32-byte cells, of which it writes out one float
// per cell) becomes
//
//     std::vector<float> hz = stencil::hip::read(grid, &Cell::hz, {0, n_rows, 0, n_cols});          // one eighth
//     std::vector<float> small = stencil::hip::read(grid, &Cell::hz, {0, n_rows, 0, n_cols}, {4, 4}); // every 4th cell
//
// and a source injected between two calls
//
//     stencil::hip::fill(grid, &Cell::hz, {r, r + 3, c, c + 3}, 1.0f);   // queued behind the update, no transfer
//     grid = update(grid);
//
// read / write move a rectangle (of whole cells, or of one member) between HBM and dense host memory
// (ststhip_grid_download / ststhip_grid_upload), fill and copy stay on the device (ststhip_grid_fill /
// ststhip_grid_copy: queued on the runtime's stream, not waited for).  Rectangles are half-open and are NOT clipped: one
// that leaves the grid throws std::range_error, as copy_from_buffer does for a buffer of another size.
//
// Validity: readers see a newer host mirror (it is uploaded first, as for a StencilUpdate); after a writer the host
// mirror no longer counts, so the next GridAccessor downloads the grid and the next StencilUpdate uploads nothing.
// Copies of a Grid share their cells: what is written here is seen through every handle of the grid.
#pragma once
#include "Grid.hpp"

#include <cstddef>
#include <stdexcept>
#include <vector>

namespace stencil {
namespace hip {

struct Rect {
    std::size_t row_begin, row_end, col_begin, col_end; // half-open
};
struct Step {
    std::size_t rows = 1, cols = 1;
};

namespace internal {

// Elements per axis of `rect` taken every `step`-th: ceil(rows / step.rows) x ceil(cols / step.cols).
struct RegionShape {
    std::size_t rows, cols;
};
template <typename Cell> RegionShape region_shape(Grid<Cell> const &grid, Rect rect, Step step = {}) {
    if (rect.row_begin > rect.row_end || rect.col_begin > rect.col_end || rect.row_end > grid.get_grid_height() ||
        rect.col_end > grid.get_grid_width())
        throw std::range_error("The rectangle does not lie inside the grid");
    if (step.rows == 0 || step.cols == 0)
        throw std::range_error("A step is 1 or more");
    return RegionShape{(rect.row_end - rect.row_begin + step.rows - 1) / step.rows,
                       (rect.col_end - rect.col_begin + step.cols - 1) / step.cols};
}

template <typename Cell> ststhip_grid_view grid_view(Grid<Cell> const &grid, const void *cells, std::size_t offset) {
    return ststhip_grid_view{const_cast<char *>(static_cast<const char *>(cells)) + offset, sizeof(Cell),
                             grid.get_grid_width(), grid.get_grid_height(), grid.get_grid_width()};
}
inline ststhip_grid_view host_view(const void *dense, std::size_t elem_size, RegionShape shape) {
    return ststhip_grid_view{const_cast<void *>(dense), elem_size, shape.cols, shape.rows, shape.cols};
}
template <typename Cell, typename M> std::size_t member_offset(M Cell::*member) {
    Cell probe{};
    return std::size_t(reinterpret_cast<const char *>(&(probe.*member)) - reinterpret_cast<const char *>(&probe));
}

template <typename Cell>
void region_read(Grid<Cell> &grid, std::size_t offset, std::size_t elem_size, Rect rect, Step step, RegionShape shape,
                 void *dense) {
    if (shape.rows == 0 || shape.cols == 0)
        return;
    ensure_runtime(-1);
    ststhip_grid_copy_desc c{};
    c.src = grid_view(grid, grid.device_cells(), offset);
    c.dst = host_view(dense, elem_size, shape);
    c.elem_size = std::uint32_t(elem_size);
    c.src_row = rect.row_begin;
    c.src_col = rect.col_begin;
    c.n_rows = shape.rows;
    c.n_cols = shape.cols;
    c.src_row_step = step.rows;
    c.src_col_step = step.cols;
    check(ststhip_grid_download(1, &c, default_stream()), "ststhip_grid_download");
}

template <typename Cell>
void region_write(Grid<Cell> &grid, std::size_t offset, std::size_t elem_size, Rect rect, RegionShape shape,
                  const void *dense) {
    if (shape.rows == 0 || shape.cols == 0)
        return;
    ensure_runtime(-1);
    ststhip_grid_copy_desc c{};
    c.dst = grid_view(grid, grid.device_cells_for_update(), offset);
    c.src = host_view(dense, elem_size, shape);
    c.elem_size = std::uint32_t(elem_size);
    c.dst_row = rect.row_begin;
    c.dst_col = rect.col_begin;
    c.n_rows = shape.rows;
    c.n_cols = shape.cols;
    c.src_row_step = c.src_col_step = 1;
    check(ststhip_grid_upload(1, &c, default_stream()), "ststhip_grid_upload");
}

template <typename Cell>
void region_fill(Grid<Cell> &grid, std::size_t offset, std::size_t elem_size, Rect rect, RegionShape shape,
                 const void *value) {
    if (shape.rows == 0 || shape.cols == 0)
        return;
    ensure_runtime(-1);
    ststhip_grid_fill_desc f{};
    f.dst = grid_view(grid, grid.device_cells_for_update(), offset);
    f.elem_size = std::uint32_t(elem_size);
    f.dst_row = rect.row_begin;
    f.dst_col = rect.col_begin;
    f.n_rows = shape.rows;
    f.n_cols = shape.cols;
    f.value = value;
    check(ststhip_grid_fill(1, &f, default_stream()), "ststhip_grid_fill");
}

} // namespace internal

// The cells of `rect`, every step.rows-th row and step.cols-th column of it: ceil(rows / step.rows) x
// ceil(cols / step.cols) cells, dense, row-major.  Blocks until they are on the host.
template <typename Cell> std::vector<Cell> read(Grid<Cell> &grid, Rect rect, Step step = {}) {
    const internal::RegionShape shape = internal::region_shape(grid, rect, step);
    std::vector<Cell> dense(shape.rows * shape.cols);
    internal::region_read(grid, 0, sizeof(Cell), rect, step, shape, dense.data());
    return dense;
}
// The same of one member of the cells.
template <typename Cell, typename M> std::vector<M> read(Grid<Cell> &grid, M Cell::*member, Rect rect, Step step = {}) {
    const internal::RegionShape shape = internal::region_shape(grid, rect, step);
    std::vector<M> dense(shape.rows * shape.cols);
    internal::region_read(grid, internal::member_offset(member), sizeof(M), rect, step, shape, dense.data());
    return dense;
}

// `dense` (rows x cols of `rect`, row-major) into the cells of `rect`, or into one member of them: the other members
// keep their bytes.  Blocks until `dense` has been read.
template <typename Cell> void write(Grid<Cell> &grid, Rect rect, Cell const *dense) {
    internal::region_write(grid, 0, sizeof(Cell), rect, internal::region_shape(grid, rect), dense);
}
template <typename Cell, typename M> void write(Grid<Cell> &grid, M Cell::*member, Rect rect, M const *dense) {
    internal::region_write(grid, internal::member_offset(member), sizeof(M), rect, internal::region_shape(grid, rect), dense);
}

// One value into every cell of `rect`, or into one member of them.  Queued on the runtime's stream; does not wait.
template <typename Cell> void fill(Grid<Cell> &grid, Rect rect, Cell const &value) {
    internal::region_fill(grid, 0, sizeof(Cell), rect, internal::region_shape(grid, rect), &value);
}
template <typename Cell, typename M> void fill(Grid<Cell> &grid, M Cell::*member, Rect rect, M const &value) {
    internal::region_fill(grid, internal::member_offset(member), sizeof(M), rect, internal::region_shape(grid, rect), &value);
}

// The cells of `rect` of `src` (every step-th) into `dst` from (row, col) on, device to device.  Queued on the
// runtime's stream; does not wait.  Within one grid the two rectangles must not share cells.
template <typename Cell>
void copy(Grid<Cell> &dst, std::size_t row, std::size_t col, Grid<Cell> &src, Rect rect, Step step = {}) {
    const internal::RegionShape shape = internal::region_shape(src, rect, step);
    if (row > dst.get_grid_height() || shape.rows > dst.get_grid_height() - row || col > dst.get_grid_width() ||
        shape.cols > dst.get_grid_width() - col)
        throw std::range_error("The rectangle does not lie inside the target grid");
    if (shape.rows == 0 || shape.cols == 0)
        return;
    internal::ensure_runtime(-1);
    ststhip_grid_copy_desc c{};
    c.src = internal::grid_view(src, src.device_cells(), 0);
    c.dst = internal::grid_view(dst, dst.device_cells_for_update(), 0);
    c.elem_size = std::uint32_t(sizeof(Cell));
    c.dst_row = row;
    c.dst_col = col;
    c.src_row = rect.row_begin;
    c.src_col = rect.col_begin;
    c.n_rows = shape.rows;
    c.n_cols = shape.cols;
    c.src_row_step = step.rows;
    c.src_col_step = step.cols;
    internal::check(ststhip_grid_copy(1, &c, internal::default_stream()), "ststhip_grid_copy");
}

} // namespace hip
} // namespace stencil

// Device-side reductions over a stencil::hip::Grid -- an EXTENSION of the reference's API (it has none): an
// application that checks convergence between StencilUpdate calls (examples/convection/convection.cpp:412-438 scans
// the whole grid through a host accessor every `nerr` iterations) asks the device for the few numbers it needs
// instead of downloading every cell.
//
//     auto m = stencil::hip::max_abs(grid, {stencil::hip::over(&Cell::ErrV, nx, ny + 1),
//                                           stencil::hip::over(&Cell::Vx, nx + 1, ny)});
//     // m[i] = max |field i| over rows < row_limit, columns < col_limit; -infinity if that range is empty
//
// One pass over the AoS cells in HBM (ststhip_reduce_max_abs: wave DPP reduce + one atomic per wave and field).
//
// What a "run until converged" loop needs beyond that -- how far two grids are apart, an L2 norm, a sum that should be
// conserved, whether anything has become NaN -- comes from norms() and distance() (ststhip_grid_norms /
// ststhip_grid_distance: no atomics, the same bits on every call and every device):
//
//     auto n = stencil::hip::norms(grid, {stencil::hip::over(&Cell::T, 1, ny - 1, 1, nx - 1)});  // rows, then columns
//     auto d = stencil::hip::distance(after, before, {stencil::hip::over(&Cell::T, ny, nx)});
//     // d[i].max_abs, .sum, .sum_abs, .sum_sq over the cells whose value is finite; .n_nonfinite counts the others
//     auto e = stencil::hip::distance(after, before);   // Grid<float> / Grid<double>: the cell is the field
//
// StencilUpdate never writes its input grid, so the caller still holds both states after a call:
//
//     for (;;) {
//         Grid<Cell> next = update(grid);                      // k generations (Params::n_iterations = k)
//         auto d = stencil::hip::distance(next, grid, {stencil::hip::over(&Cell::T, ny, nx)})[0];
//         grid = next;
//         if (d.n_nonfinite > 0) throw std::runtime_error("the run has diverged");
//         if (d.max_abs < tolerance) break;
//     }
#pragma once
#include "Grid.hpp"

#include <cstddef>
#include <initializer_list>
#include <stdexcept>
#include <type_traits>
#include <vector>

namespace stencil {
namespace hip {

// One field of the cell and the sub-rectangle [0, row_limit) x [0, col_limit) it is reduced over.
struct ReduceField {
    ststhip_reduce_field raw;
};

template <typename Cell, typename Real>
ReduceField over(Real Cell::*member, std::size_t row_limit, std::size_t col_limit) {
    static_assert(std::is_same_v<Real, float> || std::is_same_v<Real, double>,
                  "max_abs reduces float and double fields");
    Cell probe{};
    ReduceField f;
    f.raw.offset = std::uint32_t(reinterpret_cast<const char *>(&(probe.*member)) -
                                 reinterpret_cast<const char *>(&probe));
    f.raw.type = std::is_same_v<Real, double> ? STSTHIP_F64 : STSTHIP_F32;
    f.raw.row_limit = row_limit;
    f.raw.col_limit = col_limit;
    return f;
}

// One field and the rectangle [row_begin, row_limit) x [col_begin, col_limit) norms() and distance() reduce it over.  A
// ReduceField (a rectangle from (0, 0)) converts to it, so over(member, row_limit, col_limit) serves both max_abs and
// the norms; a field with a begin is a NormField only, and max_abs does not take it.
struct NormField {
    ststhip_reduce_field raw;
    std::size_t row_begin = 0, col_begin = 0;
    NormField() = default;
    NormField(ReduceField const &f) : raw(f.raw) {}
};

// The same with a begin: rows [row_begin, row_end), columns [col_begin, col_end).
template <typename Cell, typename Real>
NormField over(Real Cell::*member, std::size_t row_begin, std::size_t row_end, std::size_t col_begin,
               std::size_t col_end) {
    NormField f = over(member, row_end, col_end);
    f.row_begin = row_begin;
    f.col_begin = col_begin;
    return f;
}

// Grids whose cell is itself a float or a double (the Jacobi grids) have no member to name: the cell is the field.
template <typename Real> ReduceField over(std::size_t row_limit, std::size_t col_limit) {
    static_assert(std::is_same_v<Real, float> || std::is_same_v<Real, double>, "norms reduce float and double cells");
    ReduceField f;
    f.raw.offset = 0;
    f.raw.type = std::is_same_v<Real, double> ? STSTHIP_F64 : STSTHIP_F32;
    f.raw.row_limit = row_limit;
    f.raw.col_limit = col_limit;
    return f;
}
template <typename Real>
NormField over(std::size_t row_begin, std::size_t row_end, std::size_t col_begin, std::size_t col_end) {
    NormField f = over<Real>(row_end, col_end);
    f.row_begin = row_begin;
    f.col_begin = col_begin;
    return f;
}

// Maximum of |field| per entry of `fields` (at most 8), computed on the device; blocks until it is known.
template <typename Cell> std::vector<double> max_abs(Grid<Cell> &grid, std::initializer_list<ReduceField> fields) {
    std::vector<ststhip_reduce_field> raw;
    for (ReduceField const &f : fields)
        raw.push_back(f.raw);
    std::vector<double> result(raw.size());
    if (raw.empty())
        return result;
    internal::ensure_runtime(-1);
    internal::check(ststhip_reduce_max_abs(grid.device_cells(), sizeof(Cell), grid.get_grid_height(),
                                           grid.get_grid_width(), grid.get_grid_width(), int(raw.size()),
                                           raw.data(), result.data(), internal::default_stream()),
                    "ststhip_reduce_max_abs");
    return result;
}

// One record per field: n_cells, n_nonfinite, max_abs (-infinity if no cell has a finite value), sum, sum_abs, sum_sq.
using Norms = ststhip_norm_result;

namespace internal {
template <typename Cell>
std::vector<Norms> grid_norms(Cell const *a, Cell const *b, std::size_t height, std::size_t width,
                              std::vector<NormField> const &fields) {
    std::vector<ststhip_norm_field> raw;
    std::vector<const void *> other;
    for (NormField const &f : fields) {
        ststhip_norm_field n{};
        n.base = reinterpret_cast<const char *>(a) + f.raw.offset;
        n.stride = sizeof(Cell);
        n.pitch = width;
        n.height = height;
        n.width = width;
        n.row_begin = f.row_begin;
        n.row_end = f.raw.row_limit;
        n.col_begin = f.col_begin;
        n.col_end = f.raw.col_limit;
        n.type = f.raw.type;
        raw.push_back(n);
        other.push_back(b ? reinterpret_cast<const char *>(b) + f.raw.offset : nullptr);
    }
    std::vector<Norms> result(raw.size());
    if (raw.empty())
        return result;
    if (b)
        check(ststhip_grid_distance(int(raw.size()), raw.data(), other.data(), result.data(), default_stream()),
              "ststhip_grid_distance");
    else
        check(ststhip_grid_norms(int(raw.size()), raw.data(), result.data(), default_stream()), "ststhip_grid_norms");
    return result;
}
} // namespace internal

// Norms of up to 8 fields of the grid, computed on the device; blocks until they are known.
template <typename Cell> std::vector<Norms> norms(Grid<Cell> &grid, std::initializer_list<NormField> fields) {
    internal::ensure_runtime(-1);
    return internal::grid_norms<Cell>(grid.device_cells(), nullptr, grid.get_grid_height(), grid.get_grid_width(),
                                      std::vector<NormField>(fields));
}

// The same of a - b, cell by cell in double.  Throws std::range_error if the grids' extents differ.
template <typename Cell>
std::vector<Norms> distance(Grid<Cell> &a, Grid<Cell> &b, std::initializer_list<NormField> fields) {
    if (a.get_grid_height() != b.get_grid_height() || a.get_grid_width() != b.get_grid_width())
        throw std::range_error("The two grids have not the same size");
    internal::ensure_runtime(-1);
    Cell const *cells_a = a.device_cells();
    Cell const *cells_b = b.device_cells();
    return internal::grid_norms<Cell>(cells_a, cells_b, a.get_grid_height(), a.get_grid_width(),
                                      std::vector<NormField>(fields));
}

// Grid<float> / Grid<double>: the whole grid, one record.
template <typename Cell> Norms norms(Grid<Cell> &grid) {
    return norms(grid, {over<Cell>(grid.get_grid_height(), grid.get_grid_width())})[0];
}
template <typename Cell> Norms distance(Grid<Cell> &a, Grid<Cell> &b) {
    return distance(a, b, {over<Cell>(a.get_grid_height(), a.get_grid_width())})[0];
}

} // namespace hip
} // namespace stencil

// Computing with stencil::hip::Grids where the cells are -- an EXTENSION of the reference's API, beside Reduce.hpp (look
// at a grid) and Region.hpp (move parts of it).  A Jacobi sweep alone is a smoother; the routes from there to a solver
// need a linear combination of a few grids and a 2:1 transfer between a fine and a coarse grid:
//
//     // weighted Jacobi: u <- (1 - w) u + w J(u)
//     Grid<float> ju = update(u);
//     stencil::hip::combine(field(u), whole, {term(1.0 - w, u), term(w, ju)});
//
//     // two-grid correction: u <- u + P(e)
//     stencil::hip::restrict_mean(field(coarse_r), coarse_all, field(fine_r), 0, 0);
//     ... solve for e on the coarse grid ...
//     stencil::hip::prolong_bilinear(field(fine_e), 0, 0, field(coarse_e), coarse_all, 0.0f);
//     stencil::hip::combine(field(u), whole, {term(1.0, u), term(1.0, fine_e)});
//
// A field is one float or double per cell: a member of the cells of a grid, field(grid, &Cell::member), or the cells of
// a grid of plain floats, field(grid).  A term is (coefficient, field): term(coef, grid, &Cell::member) or
// term(coef, grid); its grid may be of another cell type than the destination's, its element type may not -- a
// Term<double> in a combine of floats does not compile, and where the types are erased (AnyField / AnyTerm) it throws
// std::invalid_argument.
//
// The results are defined operation by operation (ststhip.h, "Grid algebra"): every product and every sum is rounded
// once in the element's type, left to right, never fused, so the same formula in plain host C++ built with
// -ffp-contract=off gives the same bits.  Rectangles are half-open and NOT clipped: one that leaves a grid throws
// std::range_error.  The calls are queued on the runtime's stream and do not wait.
//
// Validity, as for the regions: sources are readers (a newer host mirror is uploaded first), the destination goes
// through Grid::device_cells_for_update(), after which the host mirror no longer counts.
#pragma once
#include "Region.hpp"

#include <functional>
#include <initializer_list>
#include <type_traits>
#include <vector>

namespace stencil {
namespace hip {

// One float or double per cell of some grid; the cell type is erased.  Holds a handle of the grid (handles share cells).
struct AnyField {
    std::uint32_t type = STSTHIP_F32; // STSTHIP_F32 or STSTHIP_F64
    std::size_t height = 0, width = 0;
    std::function<ststhip_grid_view()> for_reading; // brings the device copy up to date
    std::function<ststhip_grid_view()> for_update;  // the same, and the host mirror no longer counts
};
template <typename M> struct Field : AnyField {
    static_assert(std::is_same_v<M, float> || std::is_same_v<M, double>, "a field is a float or a double per cell");
};
struct AnyTerm {
    double coef;
    AnyField field;
};
template <typename M> struct Term {
    double coef;
    Field<M> field;
    operator AnyTerm() const { return AnyTerm{coef, field}; }
};

namespace internal {
template <typename M, typename Cell> Field<M> make_field(Grid<Cell> &grid, std::size_t offset) {
    Field<M> f;
    f.type = std::is_same_v<M, double> ? STSTHIP_F64 : STSTHIP_F32;
    f.height = grid.get_grid_height();
    f.width = grid.get_grid_width();
    f.for_reading = [grid, offset]() mutable { return grid_view(grid, grid.device_cells(), offset); };
    f.for_update = [grid, offset]() mutable { return grid_view(grid, grid.device_cells_for_update(), offset); };
    return f;
}
inline void require_inside(AnyField const &f, Rect rect, const char *what) {
    if (rect.row_begin > rect.row_end || rect.col_begin > rect.col_end || rect.row_end > f.height || rect.col_end > f.width)
        throw std::range_error(what);
}
inline Rect rect_at(std::size_t row, std::size_t col, std::size_t n_rows, std::size_t n_cols) {
    return Rect{row, row + n_rows, col, col + n_cols};
}
} // namespace internal

template <typename Cell, typename M> Field<M> field(Grid<Cell> &grid, M Cell::*member) {
    return internal::make_field<M>(grid, internal::member_offset(member));
}
template <typename Cell> Field<Cell> field(Grid<Cell> &grid) { return internal::make_field<Cell>(grid, 0); }
template <typename Cell, typename M> Term<M> term(double coef, Grid<Cell> &grid, M Cell::*member) {
    return Term<M>{coef, field(grid, member)};
}
template <typename Cell> Term<Cell> term(double coef, Grid<Cell> &grid) { return Term<Cell>{coef, field(grid)}; }

// dst = coef_0 * x_0 (+ coef_1 * x_1 (+ ...)) over `rect`, which applies to the destination and to every term alike:
// one to four terms of the destination's element type.  A term may be the destination itself (in place) or another
// member of its cells; any other overlap with the destination is refused by the library.
inline void combine(AnyField const &dst, Rect rect, std::vector<AnyTerm> const &terms) {
    if (terms.size() < 1 || terms.size() > 4)
        throw std::invalid_argument("A combine takes one to four terms");
    for (AnyTerm const &t : terms)
        if (t.field.type != dst.type)
            throw std::invalid_argument("A term's element type differs from the destination's");
    internal::require_inside(dst, rect, "The rectangle does not lie inside the target grid");
    for (AnyTerm const &t : terms)
        internal::require_inside(t.field, rect, "The rectangle does not lie inside a term's grid");
    if (rect.row_begin == rect.row_end || rect.col_begin == rect.col_end)
        return;
    internal::ensure_runtime(-1);
    ststhip_grid_combine_desc c{};
    c.type = dst.type;
    c.n_terms = std::uint32_t(terms.size());
    c.dst_row = rect.row_begin;
    c.dst_col = rect.col_begin;
    c.n_rows = rect.row_end - rect.row_begin;
    c.n_cols = rect.col_end - rect.col_begin;
    for (std::size_t t = 0; t < terms.size(); t++) { // readers first: the destination's mirror stops counting last
        c.term[t].src = terms[t].field.for_reading();
        c.term[t].row = rect.row_begin;
        c.term[t].col = rect.col_begin;
        c.term[t].coef = terms[t].coef;
    }
    c.dst = dst.for_update();
    internal::check(ststhip_grid_combine(1, &c, internal::default_stream()), "ststhip_grid_combine");
}
template <typename M> void combine(Field<M> const &dst, Rect rect, std::initializer_list<Term<M>> terms) {
    combine(static_cast<AnyField const &>(dst), rect, std::vector<AnyTerm>(terms.begin(), terms.end()));
}

namespace internal {
inline void resample(AnyField const &dst, AnyField const &src, std::uint32_t mode, Rect dst_rect, Rect src_rect,
                     std::size_t n_rows, std::size_t n_cols, double halo) {
    if (src.type != dst.type)
        throw std::invalid_argument("The source's element type differs from the destination's");
    require_inside(dst, dst_rect, "The rectangle does not lie inside the target grid");
    require_inside(src, src_rect, "The rectangle does not lie inside the source grid");
    if (n_rows == 0 || n_cols == 0)
        return;
    ensure_runtime(-1);
    ststhip_grid_resample_desc r{};
    r.type = dst.type;
    r.mode = mode;
    r.dst_row = dst_rect.row_begin;
    r.dst_col = dst_rect.col_begin;
    r.src_row = src_rect.row_begin;
    r.src_col = src_rect.col_begin;
    r.n_rows = n_rows;
    r.n_cols = n_cols;
    r.halo = halo;
    r.src = src.for_reading();
    r.dst = dst.for_update();
    check(ststhip_grid_resample(1, &r, default_stream()), "ststhip_grid_resample");
}
inline Rect checked(Rect rect) {
    if (rect.row_begin > rect.row_end || rect.col_begin > rect.col_end)
        throw std::range_error("The rectangle's end lies in front of its beginning");
    return rect;
}
} // namespace internal

// The cells of `coarse_rect` of `coarse` become the means of 2 x 2 fine cells, read from `fine` from (fine_row, fine_col)
// on:  ((s(2i,2j) + s(2i,2j+1)) + (s(2i+1,2j) + s(2i+1,2j+1))) * 0.25.
template <typename M>
void restrict_mean(Field<M> const &coarse, Rect coarse_rect, Field<M> const &fine, std::size_t fine_row = 0,
                   std::size_t fine_col = 0) {
    internal::checked(coarse_rect);
    const std::size_t n_rows = coarse_rect.row_end - coarse_rect.row_begin, n_cols = coarse_rect.col_end - coarse_rect.col_begin;
    internal::resample(coarse, fine, STSTHIP_RESTRICT_MEAN, coarse_rect,
                       internal::rect_at(fine_row, fine_col, 2 * n_rows, 2 * n_cols), n_rows, n_cols, 0.0);
}

// The 2 x 2 fine cells of every coarse cell of `coarse_rect`, written to `fine` from (fine_row, fine_col) on, by
// cell-centred bilinear interpolation (weights 0.75 / 0.25 per axis).  A neighbour outside the coarse GRID reads `halo`;
// one outside the rectangle reads the grid.
template <typename M>
void prolong_bilinear(Field<M> const &fine, std::size_t fine_row, std::size_t fine_col, Field<M> const &coarse,
                      Rect coarse_rect, M halo = M()) {
    internal::checked(coarse_rect);
    const std::size_t n_rows = coarse_rect.row_end - coarse_rect.row_begin, n_cols = coarse_rect.col_end - coarse_rect.col_begin;
    internal::resample(fine, coarse, STSTHIP_PROLONG_BILINEAR, internal::rect_at(fine_row, fine_col, 2 * n_rows, 2 * n_cols),
                       coarse_rect, n_rows, n_cols, double(halo));
}

} // namespace hip
} // namespace stencil

// A 3 x 3 linear operator applied to a stencil::hip::Grid once, with an optional right-hand side -- an EXTENSION of the
// reference's API, beside Algebra.hpp, whose fields, rectangles and error conventions it uses.  The piece of the routes
// from a smoother to a solver that reads neighbours:
//
//     // residual r = f - A u of the five-point Laplacian A = (4 u - N - W - E - S) / h^2
//     stencil::hip::apply(field(r), whole, Cross5{1 / h2, 1 / h2, -4 / h2, 1 / h2, 1 / h2}, field(u), 0.0f, 1.0, field(f));
//
//     // Jacobi relaxation with a source term: u' = 1/4 (N + W + E + S) + 1/4 h^2 f
//     stencil::hip::apply(field(next), whole, Cross5{0.25, 0.25, 0.0, 0.25, 0.25}, field(u), 0.0f, 0.25 * h2, field(f));
//
// The result is defined operation by operation (ststhip.h, "Grid stencils"): the taps of the shape in row-major order,
// acc = w_first * s_first, then acc = acc + w_k * s_k, then acc = acc + rhs_coef * rhs; every product and every sum is
// rounded once in the element's type and never fused, so the same formula in plain host C++ built with
// -ffp-contract=off gives the same bits.  A Box9 multiplies all nine taps, also those whose weight is zero (0 * inf is
// NaN); a Cross5 neither reads nor multiplies the corners.  A neighbour outside the source GRID reads `halo`, one outside
// the rectangle reads the grid.  The same rectangle applies to dst, src and rhs; it is half-open and NOT clipped: one
// that leaves a grid throws std::range_error.  Fields of different element types throw std::invalid_argument where the
// types are erased (AnyField), and do not compile otherwise.
//
// src may be another member of the destination's cells, but not the destination itself (a stencil in place is a race:
// the library refuses it); rhs may be either.  Validity is the algebra's: sources are readers, the destination goes
// through Grid::device_cells_for_update().  The calls are queued on the runtime's stream and do not wait.
#pragma once
#include "Algebra.hpp"

#include <cmath>

namespace stencil {
namespace hip {

// The five taps of a cross: north (i - 1, j), west (i, j - 1), centre, east (i, j + 1), south (i + 1, j).
struct Cross5 {
    double n, w, c, e, s;
};
// All nine taps: w[a + 1][b + 1] multiplies src(i + a, j + b).
struct Box9 {
    double w[3][3];
};

namespace internal {
inline void apply_stencil(AnyField const &dst, Rect rect, std::uint32_t shape, const double (&weight)[9], AnyField const &src,
                          double halo, const AnyField *rhs, double rhs_coef) {
    if (src.type != dst.type)
        throw std::invalid_argument("The source's element type differs from the destination's");
    if (rhs && rhs->type != dst.type)
        throw std::invalid_argument("The right-hand side's element type differs from the destination's");
    for (int k = 0; k < 9; k++) {
        if (!std::isfinite(weight[k]))
            throw std::invalid_argument("A weight of the stencil is not finite");
        if (shape == STSTHIP_STENCIL_CROSS5 && k % 2 == 0 && k != 4 && weight[k] != 0.0)
            throw std::invalid_argument("A corner weight of a five-point stencil is not zero");
    }
    require_inside(dst, rect, "The rectangle does not lie inside the target grid");
    require_inside(src, rect, "The rectangle does not lie inside the source grid");
    if (rhs)
        require_inside(*rhs, rect, "The rectangle does not lie inside the right-hand side's grid");
    if (rect.row_begin == rect.row_end || rect.col_begin == rect.col_end)
        return;
    ensure_runtime(-1);
    ststhip_grid_stencil_desc d{};
    d.type = dst.type;
    d.shape = shape;
    d.has_rhs = rhs ? 1u : 0u;
    d.dst_row = d.src_row = d.rhs_row = rect.row_begin;
    d.dst_col = d.src_col = d.rhs_col = rect.col_begin;
    d.n_rows = rect.row_end - rect.row_begin;
    d.n_cols = rect.col_end - rect.col_begin;
    for (int k = 0; k < 9; k++)
        d.weight[k] = weight[k];
    d.rhs_coef = rhs ? rhs_coef : 0.0;
    d.halo = halo;
    d.src = src.for_reading(); // readers first: the destination's mirror stops counting last
    if (rhs)
        d.rhs = rhs->for_reading();
    d.dst = dst.for_update();
    check(ststhip_grid_stencil(1, &d, default_stream()), "ststhip_grid_stencil");
}
struct Weights {
    std::uint32_t shape;
    double w[9];
};
inline Weights weights_of(Cross5 const &k) {
    return Weights{STSTHIP_STENCIL_CROSS5, {0.0, k.n, 0.0, k.w, k.c, k.e, 0.0, k.s, 0.0}};
}
inline Weights weights_of(Box9 const &k) {
    return Weights{STSTHIP_STENCIL_BOX9,
                   {k.w[0][0], k.w[0][1], k.w[0][2], k.w[1][0], k.w[1][1], k.w[1][2], k.w[2][0], k.w[2][1], k.w[2][2]}};
}
} // namespace internal

// The type-erased form: nine row-major weights and a shape (STSTHIP_STENCIL_CROSS5 / STSTHIP_STENCIL_BOX9); a CROSS5
// with a non-zero corner weight and fields of different element types throw std::invalid_argument.
inline void apply(AnyField const &dst, Rect rect, std::uint32_t shape, const double (&weight)[9], AnyField const &src,
                  double halo = 0.0) {
    internal::apply_stencil(dst, rect, shape, weight, src, halo, nullptr, 0.0);
}
inline void apply(AnyField const &dst, Rect rect, std::uint32_t shape, const double (&weight)[9], AnyField const &src,
                  double halo, double rhs_coef, AnyField const &rhs) {
    internal::apply_stencil(dst, rect, shape, weight, src, halo, &rhs, rhs_coef);
}

// dst = K src over `rect`.
template <typename M> void apply(Field<M> const &dst, Rect rect, Cross5 const &k, Field<M> const &src, std::type_identity_t<M> halo = M()) {
    const internal::Weights w = internal::weights_of(k);
    internal::apply_stencil(dst, rect, w.shape, w.w, src, double(halo), nullptr, 0.0);
}
template <typename M> void apply(Field<M> const &dst, Rect rect, Box9 const &k, Field<M> const &src, std::type_identity_t<M> halo = M()) {
    const internal::Weights w = internal::weights_of(k);
    internal::apply_stencil(dst, rect, w.shape, w.w, src, double(halo), nullptr, 0.0);
}
// dst = K src + rhs_coef * rhs over `rect`.
template <typename M>
void apply(Field<M> const &dst, Rect rect, Cross5 const &k, Field<M> const &src, std::type_identity_t<M> halo, double rhs_coef, Field<M> const &rhs) {
    const internal::Weights w = internal::weights_of(k);
    internal::apply_stencil(dst, rect, w.shape, w.w, src, double(halo), &rhs, rhs_coef);
}
template <typename M>
void apply(Field<M> const &dst, Rect rect, Box9 const &k, Field<M> const &src, std::type_identity_t<M> halo, double rhs_coef, Field<M> const &rhs) {
    const internal::Weights w = internal::weights_of(k);
    internal::apply_stencil(dst, rect, w.shape, w.w, src, double(halo), &rhs, rhs_coef);
}

} // namespace hip
} // namespace stencil

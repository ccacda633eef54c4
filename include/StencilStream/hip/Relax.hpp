// Red-black relaxation of a stencil::hip::Grid IN PLACE -- an EXTENSION of the reference's API, beside Operator.hpp,
// whose Cross5, fields, rectangles and error conventions it uses.  The smoother of a multigrid cycle without a second
// grid:
//
//     // two Gauss-Seidel sweeps (four half-sweeps, red first) for (4 u - N - W - E - S) / h^2 = f
//     stencil::hip::relax(field(u), whole, Cross5{0.25, 0.25, 0.0, 0.25, 0.25}, 0.0f, 0, 4, 0.25 * h2, field(f));
//
//     // one SOR sweep with factor 1.5: sor(omega) = Cross5{omega/4, omega/4, 1 - omega, omega/4, omega/4}
//     stencil::hip::relax(field(u), whole, stencil::hip::sor(1.5), 0.0f, 0, 2, 1.5 * 0.25 * h2, field(f));
//
// Cell (r, q) of the GRID has the colour (r + q + parity) & 1, whatever the rectangle; half-sweep k updates the
// rectangle's cells of colour (first_colour + k) & 1.  The update is defined operation by operation (ststhip.h, "Grid
// relaxation") and is the CROSS5 of apply(): acc = n * N, then acc = acc + w * W, + c * C, + e * E, + s * S, then
// acc = acc + rhs_coef * rhs; every product and every sum is rounded once in the element's type and never fused, so the
// same formula in plain host C++ built with -ffp-contract=off gives the same bits.  The four neighbours of a cell have
// the other colour: a half-sweep reads nothing that it writes.  A neighbour outside the GRID reads `halo`, one outside
// the rectangle reads the grid.  The rectangle is half-open and NOT clipped: one that leaves a grid throws
// std::range_error.  Fields of different element types throw std::invalid_argument where the types are erased
// (AnyField), and do not compile otherwise.
//
// rhs may be another member of the relaxed field's cells, but not the relaxed field itself (the library refuses it).
// Validity is the algebra's: the right-hand side is a reader, the relaxed field goes through
// Grid::device_cells_for_update().  The calls are queued on the runtime's stream and do not wait.
#pragma once
#include "Operator.hpp"

namespace stencil {
namespace hip {

// The Cross5 of successive over-relaxation with factor omega for the five-point Laplacian (4 u - N - W - E - S) / h^2;
// the matching rhs_coef is omega * h^2 / 4.  omega = 1 is Gauss-Seidel.
inline Cross5 sor(double omega) { return Cross5{omega / 4, omega / 4, 1 - omega, omega / 4, omega / 4}; }

namespace internal {
inline void relax_field(AnyField const &u, Rect rect, Cross5 const &k, double halo, unsigned first_colour, unsigned half_sweeps,
                        const AnyField *rhs, double rhs_coef, unsigned parity) {
    if (rhs && rhs->type != u.type)
        throw std::invalid_argument("The right-hand side's element type differs from the relaxed field's");
    const double weight[5] = {k.n, k.w, k.c, k.e, k.s};
    for (double w : weight)
        if (!std::isfinite(w))
            throw std::invalid_argument("A weight of the relaxation is not finite");
    if (first_colour > 1 || parity > 1)
        throw std::invalid_argument("A colour or a parity is 0 or 1");
    if (half_sweeps < 1 || half_sweeps > 1024)
        throw std::invalid_argument("A relaxation takes 1 to 1024 half-sweeps");
    require_inside(u, rect, "The rectangle does not lie inside the relaxed grid");
    if (rhs)
        require_inside(*rhs, rect, "The rectangle does not lie inside the right-hand side's grid");
    if (rect.row_begin == rect.row_end || rect.col_begin == rect.col_end)
        return;
    ensure_runtime(-1);
    ststhip_grid_relax_desc d{};
    d.type = u.type;
    d.has_rhs = rhs ? 1u : 0u;
    d.first_colour = first_colour;
    d.n_half_sweeps = half_sweeps;
    d.parity = parity;
    d.u_row = d.rhs_row = rect.row_begin;
    d.u_col = d.rhs_col = rect.col_begin;
    d.n_rows = rect.row_end - rect.row_begin;
    d.n_cols = rect.col_end - rect.col_begin;
    for (int i = 0; i < 5; i++)
        d.weight[i] = weight[i];
    d.rhs_coef = rhs ? rhs_coef : 0.0;
    d.halo = halo;
    if (rhs)
        d.rhs = rhs->for_reading(); // the reader first: the relaxed field's mirror stops counting last
    d.u = u.for_update();
    check(ststhip_grid_relax(1, &d, default_stream()), "ststhip_grid_relax");
}
} // namespace internal

// The type-erased form; fields of different element types throw std::invalid_argument.
inline void relax(AnyField const &u, Rect rect, Cross5 const &k, double halo, unsigned first_colour, unsigned half_sweeps) {
    internal::relax_field(u, rect, k, halo, first_colour, half_sweeps, nullptr, 0.0, 0);
}
inline void relax(AnyField const &u, Rect rect, Cross5 const &k, double halo, unsigned first_colour, unsigned half_sweeps,
                  double rhs_coef, AnyField const &rhs, unsigned parity = 0) {
    internal::relax_field(u, rect, k, halo, first_colour, half_sweeps, &rhs, rhs_coef, parity);
}

// `half_sweeps` half-sweeps of u = K u over `rect`, the colour `first_colour` first.
template <typename M>
void relax(Field<M> const &u, Rect rect, Cross5 const &k, std::type_identity_t<M> halo = M(), unsigned first_colour = 0,
           unsigned half_sweeps = 2) {
    internal::relax_field(u, rect, k, double(halo), first_colour, half_sweeps, nullptr, 0.0, 0);
}
// ... of u = K u + rhs_coef * rhs; `parity` moves the colours by one cell (a strip whose first row is an odd row of the
// whole grid).
template <typename M>
void relax(Field<M> const &u, Rect rect, Cross5 const &k, std::type_identity_t<M> halo, unsigned first_colour, unsigned half_sweeps,
           double rhs_coef, Field<M> const &rhs, unsigned parity = 0) {
    internal::relax_field(u, rect, k, double(halo), first_colour, half_sweeps, &rhs, rhs_coef, parity);
}

} // namespace hip
} // namespace stencil

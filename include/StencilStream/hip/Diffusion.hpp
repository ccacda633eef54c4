// The five-point finite-volume operator whose weights are FACE COEFFICIENTS STORED IN TWO FIELDS -- an EXTENSION of the
// reference's API, beside Operator.hpp and Relax.hpp, whose fields, rectangles and error conventions it uses.  What the
// constant weights of apply() and relax() cannot express: heterogeneous conduction, div(k grad u) with jumps, an
// implicit heat step (sigma + A) u = b, masked cells, Neumann walls, and the Jacobi preconditioner of conjugate gradients:
//
//     Faces<float> faces{field(kx), field(ky), 1.0f};              // east faces, south faces, the faces outside the grid
//     stencil::hip::diffuse(field(q), whole, faces, 0.0, 1.0, field(p), 0.0f);                 // q = A p
//     stencil::hip::diffuse(field(r), whole, faces, 0.0, -1.0, field(u), 0.0f, 1.0, field(f)); // r = f - A u
//     stencil::hip::jacobi_step(field(next), whole, faces, 0.0, 1.0, field(u), 0.0f, 0.8, 1.0, field(f));
//     stencil::hip::diagonal_solve(field(z), whole, faces, 0.0, 1.0, 1.0, field(r));          // z = r / diag(A)
//
// kx(i, j) is the EAST face of cell (i, j) and ky(i, j) its SOUTH face; the west face is kx(i, j - 1), the north face
// ky(i - 1, j), so the operator is symmetric by construction.  A zero face is an insulated wall.  The result is defined
// operation by operation (ststhip.h, "Grid diffusion"):
//     acc = kn*(c-n);  acc = acc + kw*(c-w);  acc = acc + ke*(c-e);  acc = acc + ks*(c-s)
//     d = kn + kw;  d = d + ke;  d = d + ks;  d = scale*d;  d = sigma + d
//     diffuse:         y = sigma*c;  y = y + scale*acc;  with a right-hand side:  y = y + rhs_coef*f
//     jacobi_step:     t = sigma*c;  t = t + scale*acc;  r = rhs_coef*f;  r = r - t;  y = c + omega*(r/d)
//     diagonal_solve:  y = (rhs_coef*f)/d
// Every operation is rounded once in the element's type and never fused and `/` is the IEEE quotient, so the same
// formula in plain host C++ built with -ffp-contract=off gives the same bits.  A neighbour of src outside the GRID reads
// `halo`, the west face of column 0 and the north face of row 0 read Faces::outside; a cell outside the rectangle reads
// the grid.  The same rectangle applies to every field; it is half-open and NOT clipped: one that leaves a grid throws
// std::range_error.  Fields of different element types throw std::invalid_argument where the types are erased
// (AnyField), and do not compile otherwise.
//
// src, kx and ky may be other members of the destination's cells, but not the destination itself (the library refuses
// it); rhs may be either.  Validity is the algebra's: sources are readers, the destination goes through
// Grid::device_cells_for_update().  The calls are queued on the runtime's stream and do not wait.
#pragma once
#include "Operator.hpp"

namespace stencil {
namespace hip {

// The face coefficients of a grid: kx holds east faces, ky south faces; `outside` is what the west face of the first
// column and the north face of the first row read.
struct AnyFaces {
    AnyField kx, ky;
    double outside = 0.0;
};
template <typename M> struct Faces {
    Field<M> kx, ky;
    M outside = M();
};

namespace internal {
inline void diffusion(AnyField const &dst, Rect rect, std::uint32_t mode, AnyFaces const &faces, double sigma, double scale,
                      double omega, const AnyField *src, double halo, const AnyField *rhs, double rhs_coef) {
    if (faces.kx.type != dst.type || faces.ky.type != dst.type)
        throw std::invalid_argument("A face field's element type differs from the destination's");
    if (src && src->type != dst.type)
        throw std::invalid_argument("The source's element type differs from the destination's");
    if (rhs && rhs->type != dst.type)
        throw std::invalid_argument("The right-hand side's element type differs from the destination's");
    if (!std::isfinite(sigma) || !std::isfinite(scale))
        throw std::invalid_argument("sigma or scale is not finite");
    if (rhs && !std::isfinite(rhs_coef))
        throw std::invalid_argument("rhs_coef is not finite");
    if (mode == STSTHIP_DIFFUSION_JACOBI && !std::isfinite(omega))
        throw std::invalid_argument("omega is not finite");
    require_inside(dst, rect, "The rectangle does not lie inside the target grid");
    if (src)
        require_inside(*src, rect, "The rectangle does not lie inside the source grid");
    require_inside(faces.kx, rect, "The rectangle does not lie inside the east faces' grid");
    require_inside(faces.ky, rect, "The rectangle does not lie inside the south faces' grid");
    if (rhs)
        require_inside(*rhs, rect, "The rectangle does not lie inside the right-hand side's grid");
    if (rect.row_begin == rect.row_end || rect.col_begin == rect.col_end)
        return;
    ensure_runtime(-1);
    ststhip_grid_diffusion_desc d{};
    d.type = dst.type;
    d.mode = mode;
    d.has_rhs = rhs ? 1u : 0u;
    d.dst_row = d.u_row = d.kx_row = d.ky_row = d.rhs_row = rect.row_begin;
    d.dst_col = d.u_col = d.kx_col = d.ky_col = d.rhs_col = rect.col_begin;
    d.n_rows = rect.row_end - rect.row_begin;
    d.n_cols = rect.col_end - rect.col_begin;
    d.sigma = sigma;
    d.scale = scale;
    d.omega = mode == STSTHIP_DIFFUSION_JACOBI ? omega : 0.0;
    d.rhs_coef = rhs ? rhs_coef : 0.0;
    d.halo = halo;
    d.k_halo = faces.outside;
    if (src)
        d.u = src->for_reading(); // readers first: the destination's mirror stops counting last
    d.kx = faces.kx.for_reading();
    d.ky = faces.ky.for_reading();
    if (rhs)
        d.rhs = rhs->for_reading();
    d.dst = dst.for_update();
    check(ststhip_grid_diffusion(1, &d, default_stream()), "ststhip_grid_diffusion");
}
template <typename M> AnyFaces erased(Faces<M> const &faces) { return AnyFaces{faces.kx, faces.ky, double(faces.outside)}; }
} // namespace internal

// The type-erased forms; fields of different element types throw std::invalid_argument.
inline void diffuse(AnyField const &dst, Rect rect, AnyFaces const &faces, double sigma, double scale, AnyField const &src,
                    double halo = 0.0) {
    internal::diffusion(dst, rect, STSTHIP_DIFFUSION_APPLY, faces, sigma, scale, 0.0, &src, halo, nullptr, 0.0);
}
inline void diffuse(AnyField const &dst, Rect rect, AnyFaces const &faces, double sigma, double scale, AnyField const &src,
                    double halo, double rhs_coef, AnyField const &rhs) {
    internal::diffusion(dst, rect, STSTHIP_DIFFUSION_APPLY, faces, sigma, scale, 0.0, &src, halo, &rhs, rhs_coef);
}
inline void jacobi_step(AnyField const &dst, Rect rect, AnyFaces const &faces, double sigma, double scale, AnyField const &src,
                        double halo, double omega, double rhs_coef, AnyField const &rhs) {
    internal::diffusion(dst, rect, STSTHIP_DIFFUSION_JACOBI, faces, sigma, scale, omega, &src, halo, &rhs, rhs_coef);
}
inline void diagonal_solve(AnyField const &dst, Rect rect, AnyFaces const &faces, double sigma, double scale, double rhs_coef,
                           AnyField const &rhs) {
    internal::diffusion(dst, rect, STSTHIP_DIFFUSION_SOLVE_DIAG, faces, sigma, scale, 0.0, nullptr, 0.0, &rhs, rhs_coef);
}

// dst = (sigma + scale * A_k) src over `rect`.
template <typename M>
void diffuse(Field<M> const &dst, Rect rect, Faces<M> const &faces, double sigma, double scale, Field<M> const &src,
             std::type_identity_t<M> halo = M()) {
    internal::diffusion(dst, rect, STSTHIP_DIFFUSION_APPLY, internal::erased(faces), sigma, scale, 0.0, &src, double(halo),
                        nullptr, 0.0);
}
// dst = (sigma + scale * A_k) src + rhs_coef * rhs over `rect`.
template <typename M>
void diffuse(Field<M> const &dst, Rect rect, Faces<M> const &faces, double sigma, double scale, Field<M> const &src,
             std::type_identity_t<M> halo, double rhs_coef, Field<M> const &rhs) {
    internal::diffusion(dst, rect, STSTHIP_DIFFUSION_APPLY, internal::erased(faces), sigma, scale, 0.0, &src, double(halo),
                        &rhs, rhs_coef);
}
// One damped Jacobi step for (sigma + scale * A_k) u = rhs_coef * rhs: dst = src + omega * (residual / diagonal).
template <typename M>
void jacobi_step(Field<M> const &dst, Rect rect, Faces<M> const &faces, double sigma, double scale, Field<M> const &src,
                 std::type_identity_t<M> halo, double omega, double rhs_coef, Field<M> const &rhs) {
    internal::diffusion(dst, rect, STSTHIP_DIFFUSION_JACOBI, internal::erased(faces), sigma, scale, omega, &src,
                        double(halo), &rhs, rhs_coef);
}
// dst = rhs_coef * rhs / diag(sigma + scale * A_k): the Jacobi preconditioner.
template <typename M>
void diagonal_solve(Field<M> const &dst, Rect rect, Faces<M> const &faces, double sigma, double scale, double rhs_coef,
                    Field<M> const &rhs) {
    internal::diffusion(dst, rect, STSTHIP_DIFFUSION_SOLVE_DIAG, internal::erased(faces), sigma, scale, 0.0, nullptr, 0.0,
                        &rhs, rhs_coef);
}

} // namespace hip
} // namespace stencil

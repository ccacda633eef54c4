// Linear-form declarations for transition functions of the reference's examples, which are built unchanged: this
// header is put in front of the example's source with `-include` (Makefile, the jacobi_%_hip rules) and knows nothing
// of it but a name.  Its five-point Jacobi with general coefficients is the declared expression of
// stencil::hip::LinearCross5, coefficient i of its `coef` array belonging to N, W, S, E, C in this order.
#pragma once
#include <StencilStream/hip/LinearForm.hpp>

struct Jacobi5General;

namespace stencil {
namespace hip {
template <> struct LinearCross5<Jacobi5General> {
    // (a template: the function's members are known only where this is called)
    template <typename F> static void coefficients(F const &f, float (&c)[5]) {
        for (int i = 0; i < 5; i++)
            c[i] = f.coef[i];
    }
};
} // namespace hip
} // namespace stencil

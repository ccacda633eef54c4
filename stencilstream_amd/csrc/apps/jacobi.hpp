// Jacobi transition functions, precompiled into libststhip.so.
// Arithmetic parity: examples/jacobi/kernels.hpp:34-319 of the reference -- same operand order
// per variant (N, W, S, E, C), Cell = float, radius 1, one sub-iteration, no time-dependent value.
#pragma once
#include <StencilStream/BaseTransitionFunction.hpp>
#include <StencilStream/Stencil.hpp>
#include <cstdint>
#include <ststhip.h>

namespace stencil {
namespace apps {

enum class JacobiVariant {
    General1,  // c0*C                                    kernels.hpp:63-66
    Constant2, // (N+S)*0.5                               kernels.hpp:95-98
    Constant3, // (N+C+S)*0.33333334                      kernels.hpp:127-130
    Constant4, // (N+W+S+E)*0.25                          kernels.hpp:159-162
    Constant5, // (N+W+S+E+C)*0.2                         kernels.hpp:191-195
    General4,  // c0*N+c1*W+c2*S+c3*E                     kernels.hpp:229-233
    General5,  // c0*N+c1*W+c2*S+c3*E+c4*C                kernels.hpp:267-271
    General9   // sum over rows then columns of c[r][c]*x kernels.hpp:307-318
};

template <JacobiVariant V> struct Jacobi : public BaseTransitionFunction {
    using Cell = float;
    using Block = ststhip_jacobi_params;
    static constexpr JacobiVariant variant = V;

    float coef[9];

    static Jacobi from_params(Block const &p) {
        Jacobi j;
        for (int i = 0; i < 9; i++)
            j.coef[i] = p.coef[i];
        return j;
    }

    STST_HD float operator()(Stencil<float, 1> const &s) const {
        const float n = s[-1][0], w = s[0][-1], c = s[0][0], e = s[0][1], so = s[1][0];
        if constexpr (V == JacobiVariant::General1) {
            return coef[0] * c;
        } else if constexpr (V == JacobiVariant::Constant2) {
            return (n + so) * 0.5f;
        } else if constexpr (V == JacobiVariant::Constant3) {
            return (n + c + so) * 0.33333334f;
        } else if constexpr (V == JacobiVariant::Constant4) {
            return (n + w + so + e) * 0.25f;
        } else if constexpr (V == JacobiVariant::Constant5) {
            return (n + w + so + e + c) * 0.2f;
        } else if constexpr (V == JacobiVariant::General4) {
            return coef[0] * n + coef[1] * w + coef[2] * so + coef[3] * e;
        } else if constexpr (V == JacobiVariant::General5) {
#ifdef STSTHIP_FMA_FLAVOUR
            // The flavour built with fused multiply-adds ("jacobi5general_fma").  With -ffp-contract=fast the compiler
            // picks per kernel instantiation WHICH product of c0*N + c1*W it fuses, so the check-free code, the edge
            // code and the stages of one launch rounded differently and a result depended on the launch's chunk plan
            // (up to 3 ulp, tests/test_launch_geometry_gpu.py).  The fusion is spelled out instead, in the order gcc
            // gives the oracle's fused build (oracle/Makefile, liboracle_fma.so): the first product of the sum is fused
            // into the first addition, every later product into its own.  One multiplication and four fused
            // multiply-adds, as before.
            return __builtin_fmaf(coef[4], c, __builtin_fmaf(coef[3], e, __builtin_fmaf(coef[2], so,
                                  __builtin_fmaf(coef[0], n, coef[1] * w))));
#else
            return coef[0] * n + coef[1] * w + coef[2] * so + coef[3] * e + coef[4] * c;
#endif
        } else {
            float sum = 0.0f;
#pragma unroll
            for (int r = -1; r <= 1; r++)
#pragma unroll
                for (int k = -1; k <= 1; k++)
                    sum += coef[(r + 1) * 3 + (k + 1)] * s[r][k];
            return sum;
        }
    }
};

// A dense 5 x 5 Jacobi of radius 2: Jacobi9General's loop (kernels.hpp:307-318) over a radius-2 stencil.  Not an
// application of the reference (SURVEY 8(f)4 asks for a tuned radius > 1 kernel); it exercises the radius-2
// stencil indexing (Stencil.hpp:120-146) and two-cell halos in the sweep.
struct Jacobi25 {
    using Cell = float;
    using TimeDependentValue = std::monostate;
    using Block = ststhip_jacobi25_params;
    static constexpr std::size_t stencil_radius = 2;
    static constexpr std::size_t n_subiterations = 1;

    float coef[25];

    static Jacobi25 from_params(Block const &p) {
        Jacobi25 j;
        for (int i = 0; i < 25; i++)
            j.coef[i] = p.coef[i];
        return j;
    }
    STST_HD std::monostate get_time_dependent_value(std::size_t) const { return {}; }

    STST_HD float operator()(Stencil<float, 2> const &s) const {
        float sum = 0.0f;
#pragma unroll
        for (int r = -2; r <= 2; r++)
#pragma unroll
            for (int c = -2; c <= 2; c++)
                sum += coef[(r + 2) * 5 + (c + 2)] * s[r][c];
        return sum;
    }
};

} // namespace apps
} // namespace stencil

// the product-carrying form for five equal coefficients (Jacobi5Uniform) and its tuning: public, since the template
// layer routes declared user functors to it
#include <StencilStream/hip/forms/Jacobi5Uniform.hpp>

namespace stencil {
namespace hip {
template <typename F, bool SOA> struct SweepTuning;
// The dense 3 x 3 (17 flops and six lane shifts per cell) is bound by its instructions at any depth; four
// generations per launch leave the fewest warm-up rows and halo columns that HBM still hides
// (profiles/r02_tune_radius.txt, 16384^2: K=4 T=8: 1815, T=4: 1947, K=3 T=8: 1733, K=2 T=8: 1630, K=3 T=12: 1623).
template <> struct SweepTuning<apps::Jacobi<apps::JacobiVariant::General9>, false> {
    static constexpr int cells_per_lane = 4;
    static constexpr int max_generations = 4;
    static constexpr int prefetch_rows = 4;
    static constexpr bool interior_variant = true;
    static constexpr int min_waves_per_simd = 1;
};
} // namespace hip
} // namespace stencil

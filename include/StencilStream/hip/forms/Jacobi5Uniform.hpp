// The product-carrying form of the five-point Jacobi with five equal coefficients.  Public since the template
// layer routes declared user functors to it (hip/LinearForm.hpp, hip/StencilUpdate.hpp).  libststhip.so precompiles
// its kernels (stencilstream_amd/csrc/app_jacobi_uniform.hip) for ststhip_app_run("jacobi5general") and for that
// route: StencilUpdate launches the precompiled kernels and instantiates none in the application's translation
// unit.  The form keeps the namespace it had as a library-internal header (stencil::apps), so the kernels keep
// their symbols.
#pragma once
#include "../../BaseTransitionFunction.hpp"
#include "../../Stencil.hpp"

namespace stencil {
namespace apps {

// Jacobi5General for the case that all five coefficients are the same number c (the reference's own
// benchmark setting, examples/jacobi/scripts/benchmark.jl:44-45).  Then every product c*x is the same float
// no matter which neighbour uses it, so a cell can carry p = fl(c*x) through the generations instead of x:
//     out = ((((p_N + p_W) + p_S) + p_E) + p_C)          same additions, same order, same values
//     p_out = fl(c * out)                                  one multiplication per cell instead of five
// Results are bit-identical to Jacobi5General (kernels.hpp:267-271); the work per cell-update drops from
// 9 to 5 floating-point operations.  Grids enter and leave as ordinary values: the first pipeline level of
// the first launch of a run multiplies its (raw) inputs itself, the last level of the last launch leaves
// its sum un-multiplied.  Which launch a kernel is for is a compile-time property (FirstLaunch /
// LastLaunch), the level inside the launch comes from the sweep (at_level), so no level carries a
// run-time mode.  Needs halo_value = +0 and c > 0 (then c*halo = halo bit for bit); the runtime falls
// back to Jacobi5General otherwise.
//
// The form is only valid if c*sum is ROUNDED before the next level adds it, and if the first level's products are
// rounded before they are added.  `#pragma clang fp contract(off)` says so where the translation unit's default is
// to contract and honours pragmas (hipcc's default, -ffp-contract=fast-honor-pragmas).  A unit built with
// -ffp-contract=fast disregards the pragma: instantiate the form's kernels only in units built without contraction.
// libststhip.so is built with -ffp-contract=off, where the pragma changes nothing, and the template layer uses the
// library's kernels for that reason (and to keep applications' compile times where they were).
template <bool FirstLaunch, bool LastLaunch> struct Jacobi5Uniform : public BaseTransitionFunction {
    using Cell = float;
    struct Block {
        float c;
    };

    float c;

    static Jacobi5Uniform from_params(Block const &b) {
        Jacobi5Uniform j;
        j.c = b.c;
        return j;
    }

    // level = 0 .. levels-1 inside one launch
    template <int level, int levels> STST_HD float at_level(Stencil<float, 1> const &s) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        constexpr bool raw_inputs = FirstLaunch && level == 0;
        constexpr bool raw_output = LastLaunch && level == levels - 1;
        float n = s[-1][0], w = s[0][-1], so = s[1][0], e = s[0][1], x = s[0][0];
        if constexpr (raw_inputs) {
            n = c * n;
            w = c * w;
            so = c * so;
            e = c * e;
            x = c * x;
        }
        const float sum = n + w + so + e + x;
        if constexpr (raw_output)
            return sum;
        else
            return c * sum;
    }

#if defined(__clang__)
    // The same level for a lane's whole row of four cells at once (the sweep's row-form hook, Sweep.hpp: check-free
    // waves with four cells per lane).  The rows arrive in LANE ORDER (c0, c2, c1, c3): the register pairs A = (c0, c2)
    // and B = (c1, c3) are then each other's west and east neighbours, so twelve of a row's sixteen additions and
    // its four multiplications are packed instructions (v_pk_add_f32 / v_pk_mul_f32: two operations per issue slot).
    // Per cell these are at_level's operations on at_level's values in at_level's order, ((((n + w) + s) + e) + x) and c * sum,
    // every one rounded on its own: bit for bit the same results (tests/test_packed_rows_cpu.py).
    // `sh.west(v)` / `sh.east(v)`: v as held by the lane to the west / east.
    typedef float Pair __attribute__((ext_vector_type(2)));
    // The four additions that take ONE neighbour-lane operand stay plain: left alone the compiler packs them as well
    // and builds their operand pairs with moves (57 v_mov per batch of the headline kernel instead of 8); a value
    // that has passed through an empty asm statement is opaque to that, and the lane shift still folds onto the add.
    STST_HD static float plain(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(v));
#endif
        return v;
    }
    template <int level, int levels, typename Shifts>
    STST_HD void row_at_level(Shifts sh, float const (&north)[4], float const (&centre)[4], float const (&south)[4],
                              float (&out)[4]) const {
#pragma clang fp contract(off)
        constexpr bool raw_inputs = FirstLaunch && level == 0;
        constexpr bool raw_output = LastLaunch && level == levels - 1;
        Pair nA = {north[0], north[1]}, nB = {north[2], north[3]};
        Pair mA = {centre[0], centre[1]}, mB = {centre[2], centre[3]};
        Pair sA = {south[0], south[1]}, sB = {south[2], south[3]};
        float wl = sh.west(centre[3]); // c3 of the lane to the west
        float er = sh.east(centre[0]); // c0 of the lane to the east
        if constexpr (raw_inputs) {
            nA = c * nA;
            nB = c * nB;
            mA = c * mA;
            mB = c * mB;
            sA = c * sA;
            sB = c * sB;
            wl = c * wl;
            er = c * er;
        }
        Pair tA;
        tA.x = plain(nA.x + wl);   // c0: n + w, west is the neighbour lane's c3
        tA.y = plain(nA.y + mB.x); // c2: n + w, west is c1
        tA = ((tA + sA) + mB) + mA; // east of (c0, c2) is (c1, c3)
        Pair tB = (nB + mA) + sB;   // west of (c1, c3) is (c0, c2)
        Pair uB;
        uB.x = plain(tB.x + mA.y); // c1: + e, east is c2
        uB.y = plain(tB.y + er);   // c3: + e, east is the neighbour lane's c0
        uB = uB + mB;
        if constexpr (!raw_output) {
            tA = c * tA;
            uB = c * uB;
        }
        out[0] = tA.x;
        out[1] = tA.y;
        out[2] = uB.x;
        out[3] = uB.y;
    }
#endif

    // one generation on its own is the original expression (first and last level at once)
    STST_HD float operator()(Stencil<float, 1> const &s) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        return c * s[-1][0] + c * s[0][-1] + c * s[1][0] + c * s[0][1] + c * s[0][0];
    }
};

} // namespace apps

namespace hip {
template <typename F, bool SOA> struct SweepTuning;
// With 5 flops per cell the kernel is HBM bound at 8 generations per launch; 12 generations per launch on 3 cells per
// lane was the optimum of the independent-wave sweep (profiles/r01_tune_jacobi_uniform.txt).  Round 3: four stages
// per column strip leave room for 4 cells per lane at five to six waves per SIMD -- 16384^2: 5690 -> 6000 Gcell/s as
// single launches, 2048 x 16384 (the strip of an 8-GPU run): 3190 -> 4090, 1000 x 1500: 570 -> 710 at T = 12 -- and,
// with stage 0's loads pinned, for 16 generations per launch (four levels per stage, launch depths 16, 8, 4, 2, 1; a
// quarter fewer HBM bytes per generation: the timed path ran at 0.69 of the HBM peak at T = 12): two strips 5730 ->
// 5920, 2048-row strip 3950 -> 4130 (profiles/r03_tune_staged.txt).
template <bool FirstLaunch, bool LastLaunch>
struct SweepTuning<apps::Jacobi5Uniform<FirstLaunch, LastLaunch>, false> {
    static constexpr int cells_per_lane = 4;
    static constexpr int max_generations = 16;
    static constexpr int prefetch_rows = 4;
    static constexpr bool interior_variant = true;
    static constexpr int min_waves_per_simd = 1;
    static constexpr int stages = 4;
    // two row strips side by side: 16 chunks of ~500 rows per strip, no tapered end (6375 -> 6470)
    static constexpr int tail_permille_beside = 200;
    static constexpr bool taper_beside = false;
};
} // namespace hip
} // namespace stencil

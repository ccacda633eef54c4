// Declared linear five-point functors through stencil::hip::StencilUpdate (hip/LinearForm.hpp): which form of the
// sweep runs for which functor, parameters and halo, and that the cells are the cpu backend's bit for bit whichever
// form runs.  The functors are user code: plain C++, no HIP annotations (built with --hipstdpar).
//
//   linear_form_test                 every case of the plain build
//   linear_form_test knob            the routed case alone, prints "form: <name>" (run with STSTHIP_LINEAR_FORM=0)
//   linear_form_test dump <file>     the routed case alone, prints "form: <name>" and writes the cells to <file>
//   linear_form_test dump-tiny <file>  the same on data around the subnormal threshold
//
// Built three times (Makefile): with -ffp-contract=off; as linear_form_test_fma with -ffp-contract=fast, where the
// functor is compiled into fused multiply-adds, is no longer its declared expression, and must not be rerouted; and as
// linear_form_test_ftz with -fgpu-flush-denormals-to-zero, whose kernels flush fp32 subnormals where the library's
// keep them, and which must not be rerouted either (only its knob and dump modes are run: the cpu backend it would
// be compared with does not flush).
#include "../cpp/mini_test.hpp"
#include <StencilStream/BaseTransitionFunction.hpp>
#include <StencilStream/cpu/StencilUpdate.hpp>
#include <StencilStream/hip/StencilUpdate.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

using namespace stencil;

// the declared expression, written out
struct UserCross5 : public BaseTransitionFunction {
    using Cell = float;
    float coef[5];
    float operator()(Stencil<float, 1> const &s) const {
        return coef[0] * s[-1][0] + coef[1] * s[0][-1] + coef[2] * s[1][0] + coef[3] * s[0][1] + coef[4] * s[0][0];
    }
};
// the same function without a declaration
struct Undeclared5 : public BaseTransitionFunction {
    using Cell = float;
    float coef[5];
    float operator()(Stencil<float, 1> const &s) const {
        return coef[0] * s[-1][0] + coef[1] * s[0][-1] + coef[2] * s[1][0] + coef[3] * s[0][1] + coef[4] * s[0][0];
    }
};
// declares the linear form but multiplies the sum: other roundings
struct Liar5 : public BaseTransitionFunction {
    using Cell = float;
    float c;
    float operator()(Stencil<float, 1> const &s) const {
        return (s[-1][0] + s[0][-1] + s[1][0] + s[0][1] + s[0][0]) * c;
    }
};
// declares the linear form but clamps it: the same on every cell below the clamp
struct Clamped5 : public BaseTransitionFunction {
    using Cell = float;
    float coef[5];
    float operator()(Stencil<float, 1> const &s) const {
        return fminf(coef[0] * s[-1][0] + coef[1] * s[0][-1] + coef[2] * s[1][0] + coef[3] * s[0][1] + coef[4] * s[0][0],
                     0.9f);
    }
};

namespace stencil {
namespace hip {
template <> struct LinearCross5<UserCross5> {
    static void coefficients(UserCross5 const &f, float (&c)[5]) {
        for (int i = 0; i < 5; i++)
            c[i] = f.coef[i];
    }
};
template <> struct LinearCross5<Liar5> {
    static void coefficients(Liar5 const &f, float (&c)[5]) {
        for (int i = 0; i < 5; i++)
            c[i] = f.c;
    }
};
template <> struct LinearCross5<Clamped5> {
    static void coefficients(Clamped5 const &f, float (&c)[5]) {
        for (int i = 0; i < 5; i++)
            c[i] = f.coef[i];
    }
};
} // namespace hip
} // namespace stencil

// The three functors that must keep their general sweep are swept two generations deep on one shape only: which
// form runs and what the cells are does not depend on the pipeline's shape, and this file compiles in a fraction of
// the time.  UserCross5 keeps the default shape, as an application's functor would.
namespace stencil {
namespace hip {
template <typename F> struct ShallowTuning {
    static constexpr int cells_per_lane = 4;
    static constexpr int max_generations = 2;
    static constexpr int prefetch_rows = 4;
    static constexpr bool interior_variant = false;
    static constexpr int min_waves_per_simd = 1;
    static constexpr bool narrow_form = false;
};
template <> struct SweepTuning<Undeclared5, false> : ShallowTuning<Undeclared5> {};
template <> struct SweepTuning<Liar5, false> : ShallowTuning<Liar5> {};
template <> struct SweepTuning<Clamped5, false> : ShallowTuning<Clamped5> {};
} // namespace hip
} // namespace stencil

static_assert(hip::internal::DeclaresLinearCross5<UserCross5>);
static_assert(!hip::internal::DeclaresLinearCross5<Undeclared5>);

using Cells = std::vector<float>;

// seeded values in [0, 1), or of both signs in (-1, 1)
static Cells random_cells(std::size_t h, std::size_t w, bool both_signs, std::uint64_t seed) {
    Cells cells(h * w);
    std::uint64_t state = seed * 0x9E3779B97F4A7C15ull + 1;
    for (float &v : cells) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const float unit = float(std::uint32_t(state >> 40)) / float(1u << 24);
        v = both_signs ? 2.0f * unit - 1.0f : unit;
    }
    return cells;
}

// random sign and mantissa, exponents 2^-150 .. 2^-120 around the smallest normal 2^-126: subnormals and normals side
// by side, in the data and in what a few generations of an averaging stencil make of them
static Cells tiny_cells(std::size_t h, std::size_t w, std::uint64_t seed) {
    Cells cells(h * w);
    std::uint64_t state = seed * 0x9E3779B97F4A7C15ull + 1;
    for (float &v : cells) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const float mantissa = 1.0f + float(std::uint32_t(state >> 40)) / float(1u << 24);
        const int exponent = -150 + int((state >> 20) % 31u);
        v = std::ldexp((state >> 10) & 1u ? -mantissa : mantissa, exponent);
    }
    return cells;
}

// values in (-1, 1) with a few planted cells: a NaN in the first corner, in the last column and on either side of the
// first strip seam, a +inf with a -inf as its right neighbour (a NaN after one generation) in the last corner, in the
// first row and across the seam, subnormals in the other corners, in the first column and right of the seam, a run of
// -0.0 along the first row across column 64.  Without a seam
// (`strip` = 0 or not less than the width) column 64 or the middle column stands in for it.
static Cells planted_cells(std::size_t h, std::size_t w, std::uint64_t seed, std::size_t strip) {
    Cells cells = random_cells(h, w, true, seed);
    const std::size_t seam = strip > 0 && strip < w ? strip : (w > 65 ? 64 : w / 2);
    auto at = [&](std::size_t r, std::size_t c) -> float & { return cells[r * w + c]; };
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float subnormal = std::numeric_limits<float>::denorm_min() * 77.0f;
    for (std::size_t c = 1; c < std::min<std::size_t>(w / 2, 70); c++)
        at(0, c) = -0.0f;
    at(0, w - 1) = subnormal, at(h - 1, 0) = -subnormal;
    if (h >= 8 && w >= 8) {
        at(h / 2, seam - 1) = nan, at(3 * h / 4, seam) = nan, at(2 * h / 3, w - 1) = nan;
        at(h / 4, seam) = subnormal, at(h / 2, 0) = -subnormal;
        at(h / 3, seam - 1) = inf, at(h / 3, seam) = -inf;
        at(0, w / 2) = inf, at(0, w / 2 + 1) = -inf;
    }
    at(0, 0) = nan;
    at(h - 1, w - 2) = inf, at(h - 1, w - 1) = -inf;
    return cells;
}

template <typename Grid> static Grid grid_of(Cells const &cells, std::size_t h, std::size_t w) {
    Grid grid(h, w);
    {
        typename Grid::template GridAccessor<sycl::access::mode::read_write> ac(grid);
        for (std::size_t r = 0; r < h; r++)
            for (std::size_t c = 0; c < w; c++)
                ac[r][c] = cells[r * w + c];
    }
    return grid;
}
template <typename Grid> static Cells cells_of(Grid &grid, std::size_t h, std::size_t w) {
    Cells cells(h * w);
    typename Grid::template GridAccessor<sycl::access::mode::read> ac(grid);
    for (std::size_t r = 0; r < h; r++)
        for (std::size_t c = 0; c < w; c++)
            cells[r * w + c] = ac[r][c];
    return cells;
}
static bool same_bits(Cells const &a, Cells const &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

// The rule for data with non-finite cells: NaNs in exactly the same cells (which NaN an operation returns differs
// between x86 and the GPU), every other cell -- +-inf and +-0 included -- the same bits.  No tolerance.
static bool same_cells(Cells const &a, Cells const &b) {
    if (a.size() != b.size())
        return false;
    for (std::size_t i = 0; i < a.size(); i++)
        if (std::isnan(a[i]) != std::isnan(b[i]) || (!std::isnan(a[i]) && std::memcmp(&a[i], &b[i], sizeof(float)) != 0))
            return false;
    return true;
}
struct Shares {
    double subnormal = 0, nan = 0, finite_nonzero = 0;
};
static Shares shares_of(Cells const &cells) {
    Shares s;
    for (float v : cells) {
        s.subnormal += std::fpclassify(v) == FP_SUBNORMAL;
        s.nan += std::isnan(v);
        s.finite_nonzero += std::isfinite(v) && v != 0.0f;
    }
    const double n = double(cells.size());
    return {s.subnormal / n, s.nan / n, s.finite_nonzero / n};
}

// the cpu backend on the same functor
template <typename F>
static Cells on_cpu(F const &f, float halo, Cells const &cells, std::size_t h, std::size_t w, std::size_t offset,
                    std::size_t n) {
    cpu::StencilUpdate<F> update({.transition_function = f, .halo_value = halo, .iteration_offset = offset,
                                  .n_iterations = n, .blocking = true});
    cpu::Grid<float> grid = grid_of<cpu::Grid<float>>(cells, h, w);
    cpu::Grid<float> out = update(grid);
    return cells_of(out, h, w);
}
template <typename F> static Cells on_hip(hip::StencilUpdate<F> &update, Cells const &cells, std::size_t h, std::size_t w) {
    hip::Grid<float> grid = grid_of<hip::Grid<float>>(cells, h, w);
    hip::Grid<float> out = update(grid);
    return cells_of(out, h, w);
}

// one update on both backends: the form that ran and whether the cells agree
template <typename F>
static void expect(const char *what, F const &f, float halo, std::size_t h, std::size_t w, std::size_t n, bool both_signs,
                   hip::SweepForm form) {
    const Cells cells = random_cells(h, w, both_signs, h * 1000003 + w * 101 + n);
    hip::StencilUpdate<F> update({.transition_function = f, .halo_value = halo, .n_iterations = n, .blocking = true});
    const bool general_before = update.get_sweep_form() == hip::SweepForm::general;
    const Cells got = on_hip(update, cells, h, w);
    const Cells want = on_cpu(f, halo, cells, h, w, 0, n);
    const bool right_form = update.get_sweep_form() == form, right_cells = same_bits(got, want);
    if (!right_form || !right_cells)
        std::fprintf(stderr, "%s %zu x %zu, %zu generations, %s: form %s (expected %s), cells %s\n", what, h, w, n,
                     both_signs ? "both signs" : "[0, 1)", to_string(update.get_sweep_form()), to_string(form),
                     right_cells ? "equal" : "DIFFER from the cpu backend");
    REQUIRE(general_before);
    REQUIRE(right_form);
    REQUIRE(right_cells);
}

// the same on tiny or planted data, by the rule of same_cells; the cpu backend's result must hold the cells the data is
// there for (at least 1 % subnormals or NaNs, at most half NaNs, at least 10 % finite and not zero)
template <typename F>
static void expect_special(const char *what, F const &f, std::size_t h, std::size_t w, std::size_t n, bool planted,
                           hip::SweepForm form) {
    hip::StencilUpdate<F> update({.transition_function = f, .halo_value = 0.0f, .n_iterations = n, .blocking = true});
    std::size_t strip = hip::StencilUpdate<F>::sweep_description().strip_width;
    ststhip_app_info info;
    if (form == hip::SweepForm::jacobi5_uniform && ststhip_app_find("jacobi5uniform", &info) == STSTHIP_OK)
        strip = info.strip_width;
    const std::uint64_t seed = h * 1000003 + w * 101 + n;
    const Cells cells = planted ? planted_cells(h, w, seed, strip) : tiny_cells(h, w, seed);
    const Cells got = on_hip(update, cells, h, w);
    const Cells want = on_cpu(f, 0.0f, cells, h, w, 0, n);
    const Shares shares = shares_of(want);
    const bool right_form = update.get_sweep_form() == form, right_cells = same_cells(got, want);
    const bool telling = (planted ? shares.nan : shares.subnormal) >= 0.01 && shares.nan <= 0.5 && shares.finite_nonzero >= 0.1;
    if (!right_form || !right_cells || !telling)
        std::fprintf(stderr, "%s %zu x %zu, %zu generations, %s data (%.1f %% subnormal, %.1f %% NaN, %.1f %% finite and not "
                             "zero): form %s (expected %s), cells %s\n",
                     what, h, w, n, planted ? "planted" : "tiny", 100 * shares.subnormal, 100 * shares.nan,
                     100 * shares.finite_nonzero, to_string(update.get_sweep_form()), to_string(form),
                     right_cells ? "equal" : "DIFFER from the cpu backend");
    REQUIRE(right_form);
    REQUIRE(right_cells);
    REQUIRE(telling);
}

static const UserCross5 uniform_cross{.coef = {0.2f, 0.2f, 0.2f, 0.2f, 0.2f}};
static const UserCross5 distinct_cross{.coef = {0.2f, 0.21f, 0.19f, 0.22f, 0.18f}};

static void test_routed() {
    // ragged last strips, several strips across, and grids smaller than a stencil; 1, 2 and 16 generations are the only
    // launch of their call, 17 a first and a last one, 37 has middle launches between them
    const std::size_t shapes[4][2] = {{300, 700}, {130, 257}, {3, 5}, {1, 1}};
    for (auto const &shape : shapes)
        for (std::size_t n : {1, 2, 16, 17, 37})
            for (bool both_signs : {false, true})
                expect("UserCross5 0.2 x 5", uniform_cross, 0.0f, shape[0], shape[1], n, both_signs,
                       hip::SweepForm::jacobi5_uniform);
    // subnormals, signed zeros, infinities and NaNs: the products the form carries go subnormal or infinite exactly
    // where the declared expression does
    for (std::size_t s = 0; s < 2; s++)
        for (std::size_t n : {17, 37})
            for (bool planted : {false, true})
                expect_special("UserCross5 0.2 x 5", uniform_cross, shapes[s][0], shapes[s][1], n, planted,
                               hip::SweepForm::jacobi5_uniform);
}

static void test_not_routed() {
    const auto general = hip::SweepForm::general;
    expect("UserCross5 distinct", distinct_cross, 0.0f, 130, 257, 17, false, general);
    expect("UserCross5 -0.2 x 5", UserCross5{.coef = {-0.2f, -0.2f, -0.2f, -0.2f, -0.2f}}, 0.0f, 130, 257, 17, true, general);
    expect("UserCross5 halo 0.25", uniform_cross, 0.25f, 130, 257, 17, false, general);
    expect("UserCross5 halo -0", uniform_cross, -0.0f, 130, 257, 17, true, general);
    expect("Liar5", Liar5{.c = 0.2f}, 0.0f, 130, 257, 17, false, general);
    expect("Clamped5", Clamped5{.coef = {0.2f, 0.2f, 0.2f, 0.2f, 0.2f}}, 0.0f, 130, 257, 17, false, general);
    // (a clamp that bites: cells above 0.9 exist after one generation of 0.3 x 5 on [0, 1))
    expect("Clamped5 0.3 x 5", Clamped5{.coef = {0.3f, 0.3f, 0.3f, 0.3f, 0.3f}}, 0.0f, 130, 257, 17, false, general);
    expect("Undeclared5", Undeclared5{.coef = {0.2f, 0.2f, 0.2f, 0.2f, 0.2f}}, 0.0f, 130, 257, 17, false, general);
    for (std::size_t n : {17, 37})
        for (bool planted : {false, true}) {
            expect_special("UserCross5 distinct", distinct_cross, 130, 257, n, planted, general);
            expect_special("UserCross5 distinct", distinct_cross, 300, 700, n, planted, general);
        }
}

// 20 generations, then 17 more from generation 20 on the same object: one call of 37
static void test_resume() {
    const std::size_t h = 300, w = 700;
    const Cells cells = random_cells(h, w, true, 20);
    hip::StencilUpdate<UserCross5> update({.transition_function = uniform_cross, .halo_value = 0.0f, .n_iterations = 20,
                                           .blocking = true});
    const Cells first = on_hip(update, cells, h, w);
    REQUIRE(update.get_sweep_form() == hip::SweepForm::jacobi5_uniform);
    update.get_params().iteration_offset = 20;
    update.get_params().n_iterations = 17;
    const Cells second = on_hip(update, first, h, w);
    REQUIRE(update.get_sweep_form() == hip::SweepForm::jacobi5_uniform);
    hip::StencilUpdate<UserCross5> whole({.transition_function = uniform_cross, .halo_value = 0.0f, .n_iterations = 37,
                                          .blocking = true});
    const Cells at_once = on_hip(whole, cells, h, w);
    REQUIRE(whole.get_sweep_form() == hip::SweepForm::jacobi5_uniform);
    REQUIRE(same_bits(second, at_once));
    REQUIRE(same_bits(second, on_cpu(uniform_cross, 0.0f, cells, h, w, 0, 37)));
}

// coefficients and halo changed through get_params(): the form follows
static void test_parameter_change() {
    const std::size_t h = 130, w = 257, n = 17;
    const Cells cells = random_cells(h, w, true, 5);
    hip::StencilUpdate<UserCross5> update({.transition_function = uniform_cross, .halo_value = 0.0f, .n_iterations = n,
                                           .blocking = true});
    REQUIRE(same_bits(on_hip(update, cells, h, w), on_cpu(uniform_cross, 0.0f, cells, h, w, 0, n)));
    REQUIRE(update.get_sweep_form() == hip::SweepForm::jacobi5_uniform);
    update.get_params().transition_function = distinct_cross;
    REQUIRE(same_bits(on_hip(update, cells, h, w), on_cpu(distinct_cross, 0.0f, cells, h, w, 0, n)));
    REQUIRE(update.get_sweep_form() == hip::SweepForm::general);
    update.get_params().transition_function = uniform_cross;
    REQUIRE(same_bits(on_hip(update, cells, h, w), on_cpu(uniform_cross, 0.0f, cells, h, w, 0, n)));
    REQUIRE(update.get_sweep_form() == hip::SweepForm::jacobi5_uniform);
    update.get_params().halo_value = 0.25f;
    REQUIRE(same_bits(on_hip(update, cells, h, w), on_cpu(uniform_cross, 0.25f, cells, h, w, 0, n)));
    REQUIRE(update.get_sweep_form() == hip::SweepForm::general);
}

// the routed case on its own: 300 x 700, 37 generations, both signs or tiny data
static int routed_case_alone(const char *path, bool tiny = false) {
    const std::size_t h = 300, w = 700;
    const Cells cells = tiny ? tiny_cells(h, w, 37) : random_cells(h, w, true, 37);
    hip::StencilUpdate<UserCross5> update({.transition_function = uniform_cross, .halo_value = 0.0f, .n_iterations = 37,
                                           .blocking = true});
    const Cells got = on_hip(update, cells, h, w);
    std::printf("form: %s\n", to_string(update.get_sweep_form()));
    if (path) {
        std::FILE *out = std::fopen(path, "wb");
        if (!out || std::fwrite(got.data(), sizeof(float), got.size(), out) != got.size())
            return 2;
        std::fclose(out);
    }
    return 0;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "all";
    if (mode == "knob")
        return routed_case_alone(nullptr);
    if (mode == "dump" && argc > 2)
        return routed_case_alone(argv[2]);
    if (mode == "dump-tiny" && argc > 2)
        return routed_case_alone(argv[2], true);
    if (mode != "all") {
        std::fprintf(stderr, "usage: %s [all | knob | dump <file> | dump-tiny <file>]\n", argv[0]);
        return 2;
    }
    test_routed();
    test_not_routed();
    test_resume();
    test_parameter_change();
    return finish("linear_form_test");
}

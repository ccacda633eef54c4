// stencil::hip::norms / stencil::hip::distance (hip/Reduce.hpp) against a host loop with the same definitions, on a
// Grid<float> and on a grid of two-field struct cells, and the "run until converged" loop of the documentation on
// stencil::hip against the same loop on stencil::cpu with a host scan.
#include "../cpp/mini_test.hpp"
#include <StencilStream/BaseTransitionFunction.hpp>
#include <StencilStream/cpu/StencilUpdate.hpp>
#include <StencilStream/hip/Reduce.hpp>
#include <StencilStream/hip/StencilUpdate.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

using namespace stencil;

struct Cross5 : public BaseTransitionFunction {
    using Cell = float;
    float c;
    float operator()(Stencil<float, 1> const &s) const {
        return c * s[-1][0] + c * s[0][-1] + c * s[1][0] + c * s[0][1] + c * s[0][0];
    }
};
// two generations per launch on one pipeline shape: what is tested here does not depend on the shape, and the file
// compiles in a fraction of the time
namespace stencil {
namespace hip {
template <> struct SweepTuning<Cross5, false> {
    static constexpr int cells_per_lane = 4;
    static constexpr int max_generations = 2;
    static constexpr int prefetch_rows = 4;
    static constexpr bool interior_variant = false;
    static constexpr int min_waves_per_simd = 1;
    static constexpr bool narrow_form = false;
};
} // namespace hip
} // namespace stencil

// a float beside a double: stride 16, members at 0 and 8
struct Pair {
    float t;
    double p;
};
static_assert(sizeof(Pair) == 16 && offsetof(Pair, p) == 8);

static std::uint64_t g_state = 0x5EED;
static double unit() { // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return double(std::uint32_t(g_state >> 40)) / double(1u << 24);
}
// both signs, magnitudes 2^-20 .. 2^20
static double wide() { return (unit() < 0.5 ? -1.0 : 1.0) * std::ldexp(0.5 + 0.5 * unit(), int(unit() * 41.0) - 20); }

// The definitions of ststhip.h on the host.  The sums are kept in long double: with its 64 bits of mantissa on x86 their
// own error, about n * 2^-64 * sum |v|, is far below the bound asserted: near-exact, not exact (and an ordinary sum
// where long double is double, for which the bound below still holds: both sums are then within half of it).
struct HostNorms {
    std::uint64_t n_cells = 0, n_nonfinite = 0;
    double max_abs = -std::numeric_limits<double>::infinity();
    long double sum = 0, sum_abs = 0, sum_sq = 0;
    void take(double v) {
        n_cells++;
        if (!std::isfinite(v)) {
            n_nonfinite++;
            return;
        }
        max_abs = std::fabs(v) > max_abs ? std::fabs(v) : max_abs;
        sum += v;
        sum_abs += std::fabs(v);
        sum_sq += (long double)v * v;
    }
};

// equal counts and maximum; the sums within the bound of n additions in any order (gamma_n, one more rounding for a
// square, a factor two of slack): n * 2^-52 * sum |v| and (n + 1) * 2^-52 * sum v^2
static void expect(const char *what, hip::Norms const &got, HostNorms const &want) {
    const long double eps = std::ldexp(1.0L, -52), n = (long double)want.n_cells;
    const bool counts = got.n_cells == want.n_cells && got.n_nonfinite == want.n_nonfinite;
    const bool maximum = std::memcmp(&got.max_abs, &want.max_abs, sizeof(double)) == 0;
    const bool sums = std::fabs((long double)got.sum - want.sum) <= n * eps * want.sum_abs &&
                      std::fabs((long double)got.sum_abs - want.sum_abs) <= n * eps * want.sum_abs &&
                      std::fabs((long double)got.sum_sq - want.sum_sq) <= (n + 1) * eps * want.sum_sq;
    if (!counts || !maximum || !sums)
        std::fprintf(stderr, "%s: cells %llu / %llu, non-finite %llu / %llu, max %a / %a, sum %.17g / %.17Lg, "
                     "sum_abs %.17g / %.17Lg, sum_sq %.17g / %.17Lg\n", what, (unsigned long long)got.n_cells,
                     (unsigned long long)want.n_cells, (unsigned long long)got.n_nonfinite,
                     (unsigned long long)want.n_nonfinite, got.max_abs, want.max_abs, got.sum, want.sum, got.sum_abs,
                     want.sum_abs, got.sum_sq, want.sum_sq);
    REQUIRE(counts);
    REQUIRE(maximum);
    REQUIRE(sums);
}

template <typename Cell> static hip::Grid<Cell> grid_of(std::vector<Cell> const &cells, std::size_t h, std::size_t w) {
    hip::Grid<Cell> grid(h, w);
    {
        typename hip::Grid<Cell>::template GridAccessor<sycl::access::mode::read_write> ac(grid);
        for (std::size_t r = 0; r < h; r++)
            for (std::size_t c = 0; c < w; c++)
                ac[r][c] = cells[r * w + c];
    }
    return grid;
}

static void test_float_grid() {
    const std::size_t h = 130, w = 257;
    std::vector<float> a(h * w), b(h * w);
    for (std::size_t i = 0; i < h * w; i++) {
        a[i] = float(wide());
        b[i] = float(wide());
    }
    a[5 * w + 7] = std::numeric_limits<float>::quiet_NaN();
    a[100 * w + 256] = std::numeric_limits<float>::infinity();
    hip::Grid<float> ga = grid_of(a, h, w), gb = grid_of(b, h, w);

    HostNorms whole, inner, apart;
    for (std::size_t r = 0; r < h; r++)
        for (std::size_t c = 0; c < w; c++) {
            whole.take(double(a[r * w + c]));
            apart.take(double(a[r * w + c]) - double(b[r * w + c]));
            if (r >= 1 && r < 129 && c >= 1 && c < 256)
                inner.take(double(a[r * w + c]));
        }
    expect("Grid<float> norms", hip::norms(ga), whole);
    REQUIRE(whole.n_nonfinite == 2);
    expect("Grid<float> norms of a rectangle", hip::norms(ga, {hip::over<float>(1, 129, 1, 256)})[0], inner);
    expect("Grid<float> distance", hip::distance(ga, gb), apart);
    // a rectangle past the grid is clipped, an empty one counts nothing
    expect("Grid<float> clipped", hip::norms(ga, {hip::over<float>(h + 9, w + 9)})[0], whole);
    const hip::Norms none = hip::norms(ga, {hip::over<float>(7, 7, 0, w)})[0];
    REQUIRE(none.n_cells == 0 && none.sum == 0.0 && none.max_abs == -std::numeric_limits<double>::infinity());
    // a grid against itself
    const hip::Norms self = hip::distance(gb, gb);
    REQUIRE(self.n_cells == h * w && self.n_nonfinite == 0 && self.max_abs == 0.0 && self.sum_abs == 0.0);

    hip::Grid<float> other(h, w + 1);
    bool thrown = false;
    try {
        hip::distance(ga, other);
    } catch (std::range_error const &) {
        thrown = true;
    }
    REQUIRE(thrown);
    // max_abs as before, on the grid without non-finite cells (it skips NaN only)
    HostNorms of_b;
    for (float v : b)
        of_b.take(double(v));
    const std::vector<double> m = hip::max_abs(gb, {hip::over<float>(h, w)});
    REQUIRE(m.size() == 1 && m[0] == of_b.max_abs);
}

static void test_struct_cells() {
    const std::size_t h = 67, w = 1100; // more than one row segment of 1024 cells
    std::vector<Pair> a(h * w), b(h * w);
    for (std::size_t i = 0; i < h * w; i++) {
        a[i] = Pair{float(wide()), wide()};
        b[i] = Pair{float(wide()), wide()};
    }
    hip::Grid<Pair> ga = grid_of(a, h, w), gb = grid_of(b, h, w);
    HostNorms t, p, dt, dp;
    for (std::size_t r = 0; r < h; r++)
        for (std::size_t c = 0; c < w; c++) {
            Pair const &x = a[r * w + c], &y = b[r * w + c];
            t.take(double(x.t));
            dt.take(double(x.t) - double(y.t));
            if (r >= 3 && r < 60 && c >= 5 && c < 1099) {
                p.take(x.p);
                dp.take(x.p - y.p);
            }
        }
    const std::vector<hip::Norms> n = hip::norms(ga, {hip::over(&Pair::t, h, w), hip::over(&Pair::p, 3, 60, 5, 1099)});
    REQUIRE(n.size() == 2);
    expect("Pair::t norms", n[0], t);
    expect("Pair::p norms of a rectangle", n[1], p);
    const std::vector<hip::Norms> d = hip::distance(ga, gb, {hip::over(&Pair::t, h, w), hip::over(&Pair::p, 3, 60, 5, 1099)});
    expect("Pair::t distance", d[0], dt);
    expect("Pair::p distance of a rectangle", d[1], dp);
}

// The loop of the documentation: k generations per call, the distance of the two states, stop on max_abs < tolerance,
// stop loudly on a non-finite value.  On stencil::cpu the distance is a host scan.
static void test_run_until_converged() {
    const std::size_t h = 64, w = 64, k = 8;
    const double tolerance = 5e-3;
    const Cross5 f{.c = 0.2f};
    std::vector<float> start(h * w);
    for (float &v : start)
        v = float(unit());

    hip::StencilUpdate<Cross5> update({.transition_function = f, .halo_value = 0.0f, .n_iterations = k});
    hip::Grid<float> grid = grid_of(start, h, w);
    std::size_t calls = 0;
    bool diverged = false;
    for (;;) {
        hip::Grid<float> next = update(grid); // non-blocking: distance() sees the result through device_cells()
        const hip::Norms d = hip::distance(next, grid);
        grid = next;
        calls++;
        if (d.n_nonfinite > 0) {
            diverged = true;
            break;
        }
        if (d.max_abs < tolerance || calls >= 1000)
            break;
    }

    cpu::StencilUpdate<Cross5> cpu_update({.transition_function = f, .halo_value = 0.0f, .n_iterations = k, .blocking = true});
    cpu::Grid<float> cpu_grid(h, w);
    {
        cpu::Grid<float>::GridAccessor<sycl::access::mode::read_write> ac(cpu_grid);
        for (std::size_t r = 0; r < h; r++)
            for (std::size_t c = 0; c < w; c++)
                ac[r][c] = start[r * w + c];
    }
    std::size_t cpu_calls = 0;
    for (;;) {
        cpu::Grid<float> next = cpu_update(cpu_grid);
        double max_abs = -std::numeric_limits<double>::infinity();
        {
            cpu::Grid<float>::GridAccessor<sycl::access::mode::read> before(cpu_grid), after(next);
            for (std::size_t r = 0; r < h; r++)
                for (std::size_t c = 0; c < w; c++) {
                    const double v = double(after[r][c]) - double(before[r][c]);
                    max_abs = std::fabs(v) > max_abs ? std::fabs(v) : max_abs;
                }
        }
        cpu_grid = next;
        cpu_calls++;
        if (max_abs < tolerance || cpu_calls >= 1000)
            break;
    }

    std::printf("run until converged: %zu calls of %zu generations on stencil::hip, %zu on stencil::cpu\n", calls, k, cpu_calls);
    REQUIRE(!diverged);
    REQUIRE(calls == cpu_calls);
    REQUIRE(calls >= 24 && calls <= 60); // "a few dozen": the tolerance is chosen for it
    bool same = true;
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read> got(grid);
        cpu::Grid<float>::GridAccessor<sycl::access::mode::read> want(cpu_grid);
        for (std::size_t r = 0; r < h; r++)
            for (std::size_t c = 0; c < w; c++) {
                const float x = got[r][c], y = want[r][c];
                same = same && std::memcmp(&x, &y, sizeof(float)) == 0;
            }
    }
    REQUIRE(same);
}

int main() {
    test_float_grid();
    test_struct_cells();
    test_run_until_converged();
    return finish("grid_norms_test");
}

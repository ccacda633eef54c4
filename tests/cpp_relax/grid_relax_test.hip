// stencil::hip::relax and sor (hip/Relax.hpp) against the same half-sweeps in plain host C++ (this file is built with
// -ffp-contract=off, so the host model rounds every product and every sum once): a Grid<float> as a whole and on a
// rectangle with parity 1, a member of struct cells with another member as right-hand side, doubles;
// std::range_error and std::invalid_argument; and the validity-flag protocol between relax and the GridAccessor.
#include "../cpp/mini_test.hpp"
#include <StencilStream/hip/Relax.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

using namespace stencil;

struct Pair {
    float t;
    float k;
};
// a float, a double and a float: stride 24, members at 0, 8 and 16
struct Tri {
    float a;
    double b;
    float c;
};
static_assert(sizeof(Tri) == 24 && offsetof(Tri, b) == 8 && offsetof(Tri, c) == 16);

static std::uint64_t g_state = 0x4E1A7;
static std::uint32_t bits() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return std::uint32_t(g_state >> 32);
}
static float unit() { return float(bits() >> 8) / float(1u << 24) - 0.5f; }

// NaNs in the same places, every other value equal as bits
template <typename T> static bool same(T x, T y) {
    if (std::isnan(x) || std::isnan(y))
        return std::isnan(x) && std::isnan(y);
    return std::memcmp(&x, &y, sizeof(T)) == 0;
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
template <typename Cell> static std::vector<Cell> cells_of(hip::Grid<Cell> &grid) {
    typename hip::Grid<Cell>::template GridAccessor<sycl::access::mode::read> ac(grid);
    const std::size_t h = grid.get_grid_height(), w = grid.get_grid_width();
    std::vector<Cell> out(h * w);
    for (std::size_t r = 0; r < h; r++)
        for (std::size_t c = 0; c < w; c++)
            out[r * w + c] = ac[r][c];
    return out;
}

// ---- the host model: half-sweeps in place over a rectangle, one rounding per product and per sum ----
// u(r, c): a reference to the relaxed element; f(r, c): the right-hand side's value (used where has_rhs).
template <typename T, typename U, typename F>
static void model(U &&u, F &&f, std::size_t h, std::size_t w, hip::Rect rect, hip::Cross5 k, T halo, unsigned first_colour,
                  unsigned half_sweeps, bool has_rhs, double rhs_coef, unsigned parity) {
    const T wn = T(k.n), ww = T(k.w), wc = T(k.c), we = T(k.e), ws = T(k.s), coef = T(rhs_coef);
    for (unsigned sweep = 0; sweep < half_sweeps; sweep++)
        for (std::size_t r = rect.row_begin; r < rect.row_end; r++)
            for (std::size_t c = rect.col_begin; c < rect.col_end; c++) {
                if (((r + c + parity) & 1) != ((first_colour + sweep) & 1))
                    continue;
                const T n = r == 0 ? halo : u(r - 1, c), west = c == 0 ? halo : u(r, c - 1);
                const T e = c + 1 == w ? halo : u(r, c + 1), s = r + 1 == h ? halo : u(r + 1, c);
                T acc = wn * n;
                acc = acc + ww * west;
                acc = acc + wc * u(r, c);
                acc = acc + we * e;
                acc = acc + ws * s;
                if (has_rhs)
                    acc = acc + coef * f(r, c);
                u(r, c) = acc; // in place: the neighbours have the other colour
            }
}

constexpr std::size_t H = 38, W = 300; // wider than a wave's span of four floats per lane
static const hip::Cross5 cross{-0.23, 0.41, -0.53, 0.67, -0.83};

static void test_sor() {
    const hip::Cross5 k = hip::sor(1.5);
    REQUIRE(k.n == 0.375 && k.w == 0.375 && k.c == -0.5 && k.e == 0.375 && k.s == 0.375);
    const hip::Cross5 gs = hip::sor(1.0);
    REQUIRE(gs.n == 0.25 && gs.c == 0.0);
}

static void test_planes() {
    std::vector<float> u(H * W), f(H * W);
    for (std::size_t i = 0; i < H * W; i++)
        u[i] = unit(), f[i] = unit();
    hip::Grid<float> gu = grid_of(u, H, W), gf = grid_of(f, H, W);
    auto at = [&](std::size_t r, std::size_t c) -> float & { return u[r * W + c]; };
    auto rhs = [&](std::size_t r, std::size_t c) { return f[r * W + c]; };
    const hip::Rect whole{0, H, 0, W};
    auto agree = [&] {
        std::vector<float> got = cells_of(gu);
        bool ok = true;
        for (std::size_t i = 0; i < H * W; i++)
            ok = ok && same(got[i], u[i]);
        return ok;
    };
    // the whole grid: every border reads the halo; three half-sweeps, the odd colour first
    hip::relax(hip::field(gu), whole, cross, -2.5f, 1, 3);
    model<float>(at, rhs, H, W, whole, cross, -2.5f, 1, 3, false, 0.0, 0);
    REQUIRE(agree());
    // SOR with a right-hand side: two sweeps
    hip::relax(hip::field(gu), whole, hip::sor(1.5), 0.0f, 0, 4, 1.5 * 0.25 / 4096.0, hip::field(gf));
    model<float>(at, rhs, H, W, whole, hip::sor(1.5), 0.0f, 0, 4, true, 1.5 * 0.25 / 4096.0, 0);
    REQUIRE(agree());
    // an inner rectangle with parity 1: its neighbours outside are cells of the grid and keep their values
    const hip::Rect inner{1, H - 2, 3, W - 1};
    const float nan = std::numeric_limits<float>::quiet_NaN();
    hip::relax(hip::field(gu), inner, cross, nan, 0, 2, 0.25, hip::field(gf), 1);
    model<float>(at, rhs, H, W, inner, cross, nan, 0, 2, true, 0.25, 1);
    REQUIRE(agree());
    // the defaults: a zero halo, the even colour first, one sweep
    hip::relax(hip::field(gu), whole, cross);
    model<float>(at, rhs, H, W, whole, cross, 0.0f, 0, 2, false, 0.0, 0);
    REQUIRE(agree());
    // the right-hand side is untouched
    std::vector<float> still = cells_of(gf);
    REQUIRE(std::memcmp(still.data(), f.data(), f.size() * sizeof(float)) == 0);
}

static void test_members() {
    std::vector<Tri> tri(H * W);
    std::vector<Pair> pair(H * W);
    for (std::size_t i = 0; i < H * W; i++) {
        tri[i] = Tri{unit(), double(unit()), unit()};
        pair[i] = Pair{unit(), unit()};
    }
    hip::Grid<Tri> gt = grid_of(tri, H, W);
    hip::Grid<Pair> gp = grid_of(pair, H, W);
    const hip::Rect whole{0, H, 0, W}, part{2, H, 0, W - 5};
    // a member of Pair cells, the right-hand side the other member of the same cells
    hip::relax(hip::field(gp, &Pair::t), whole, hip::sor(1.25), 0.5f, 0, 5, -2.0, hip::field(gp, &Pair::k));
    // the double member of Tri cells on a rectangle, parity 1, no right-hand side; then a float member with a
    // right-hand side from the other cell type
    hip::relax(hip::field(gt, &Tri::b), part, cross, 7.0, 1, 2);
    hip::relax(hip::field(gt, &Tri::a), part, cross, -1.0f, 0, 3, 1.0 / 3.0, hip::field(gp, &Pair::k), 1);
    model<float>([&](std::size_t r, std::size_t c) -> float & { return pair[r * W + c].t; },
                 [&](std::size_t r, std::size_t c) { return pair[r * W + c].k; }, H, W, whole, hip::sor(1.25), 0.5f, 0, 5, true, -2.0, 0);
    model<double>([&](std::size_t r, std::size_t c) -> double & { return tri[r * W + c].b; },
                  [&](std::size_t, std::size_t) { return 0.0; }, H, W, part, cross, 7.0, 1, 2, false, 0.0, 0);
    model<float>([&](std::size_t r, std::size_t c) -> float & { return tri[r * W + c].a; },
                 [&](std::size_t r, std::size_t c) { return pair[r * W + c].k; }, H, W, part, cross, -1.0f, 0, 3, true, 1.0 / 3.0, 1);
    std::vector<Tri> got_tri = cells_of(gt);
    std::vector<Pair> got_pair = cells_of(gp);
    bool ok = true;
    for (std::size_t i = 0; i < H * W; i++)
        ok = ok && same(got_tri[i].a, tri[i].a) && same(got_tri[i].b, tri[i].b) && same(got_tri[i].c, tri[i].c) &&
             same(got_pair[i].t, pair[i].t) && same(got_pair[i].k, pair[i].k);
    REQUIRE(ok);
}

template <typename E, typename F> static bool throws(F &&call) {
    try {
        call();
    } catch (E const &) {
        return true;
    } catch (...) {
        return false;
    }
    return false;
}

static void test_errors() {
    hip::Grid<float> a(8, 12), f(8, 12), small(4, 6);
    hip::Grid<double> d(8, 12);
    const hip::Rect whole{0, 8, 0, 12};
    REQUIRE(throws<std::range_error>([&] { hip::relax(hip::field(a), {0, 9, 0, 12}, cross); }));
    REQUIRE(throws<std::range_error>([&] { hip::relax(hip::field(a), {0, 8, 3, 13}, cross); }));
    REQUIRE(throws<std::range_error>([&] { hip::relax(hip::field(a), {5, 4, 0, 12}, cross); }));
    REQUIRE(throws<std::range_error>([&] { hip::relax(hip::field(a), whole, cross, 0.0f, 0, 2, 1.0, hip::field(small)); }));
    // element types: erased fields are checked when the call is made
    const hip::AnyField fa = hip::field(a), fd = hip::field(d);
    REQUIRE(throws<std::invalid_argument>([&] { hip::relax(fa, whole, cross, 0.0, 0, 2, 1.0, fd); }));
    // colours, parities, counts and weights
    REQUIRE(throws<std::invalid_argument>([&] { hip::relax(hip::field(a), whole, cross, 0.0f, 2, 2); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::relax(hip::field(a), whole, cross, 0.0f, 0, 0); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::relax(hip::field(a), whole, cross, 0.0f, 0, 1025); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::relax(hip::field(a), whole, cross, 0.0f, 0, 2, 1.0, hip::field(f), 2); }));
    const hip::Cross5 infinite{0.25, 0.25, std::numeric_limits<double>::infinity(), 0.25, 0.25};
    REQUIRE(throws<std::invalid_argument>([&] { hip::relax(hip::field(a), whole, infinite); }));
    // an empty rectangle is fine, anywhere inside
    hip::relax(hip::field(a), {8, 8, 3, 3}, cross);
    hip::relax(hip::field(a), {2, 5, 12, 12}, cross, 0.0f, 0, 2, 1.0, hip::field(f));
    // what the library refuses arrives as an exception too: the relaxed field as its own right-hand side
    REQUIRE(throws<std::exception>([&] { hip::relax(hip::field(a), whole, cross, 0.0f, 0, 2, 1.0, hip::field(a)); }));
    hip::Grid<float> alias = a; // (handles share cells)
    REQUIRE(throws<std::exception>([&] { hip::relax(hip::field(a), {1, 7, 1, 11}, cross, 0.0f, 0, 2, 1.0, hip::field(alias)); }));
}

// host-mirror validity: write through an accessor, relax, read through an accessor
static void test_flag_protocol() {
    hip::Grid<float> u(16, 24), f(16, 24);
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> au(u), af(f);
        for (std::size_t r = 0; r < 16; r++)
            for (std::size_t c = 0; c < 24; c++) {
                au[r][c] = float(r);
                af[r][c] = float(c);
            }
    }
    const hip::Cross5 sum{1.0, 1.0, 0.0, 1.0, 1.0}; // N + W + E + S
    hip::relax(hip::field(u), {0, 16, 0, 24}, sum, 0.0f, 0, 1, 2.0, hip::field(f)); // uploads both mirrors first
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> au(u); // downloads: the mirror no longer counted
        REQUIRE(au[5][7] == 4.0f * 5.0f + 2.0f * 7.0f); // an even cell
        REQUIRE(au[5][8] == 5.0f);                       // an odd cell keeps its value
        REQUIRE(au[0][0] == 0.0f + 0.0f + 0.0f + 1.0f);  // north and west are halo
        au[5][8] = 100.0f;                               // the host writes again ...
    }
    hip::relax(hip::field(u), {0, 16, 0, 24}, sum, 0.0f, 0, 1); // ... and the write counts
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read> au(u);
        // u(5, 7) = u(4, 7) + u(5, 6) + u(5, 8) + u(6, 7), all odd cells
        REQUIRE(au[5][7] == 4.0f + 5.0f + 100.0f + 6.0f);
    }
    std::printf("flag protocol: accessor writes reach relax, its results reach the accessor\n");
}

int main() {
    test_sor();
    test_planes();
    test_members();
    test_errors();
    test_flag_protocol();
    return finish("grid_relax_test");
}

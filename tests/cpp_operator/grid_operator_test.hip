// stencil::hip::apply (hip/Operator.hpp) against the same formula in plain host C++ (this file is built with
// -ffp-contract=off, so the host model rounds every product and every sum once): a Grid<float>, members of struct cells
// of two cell types, doubles; std::range_error and std::invalid_argument; and the validity-flag protocol between apply
// and the GridAccessor.
#include "../cpp/mini_test.hpp"
#include <StencilStream/hip/Operator.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

using namespace stencil;

// a float, a double and a float: stride 24, members at 0, 8 and 16
struct Tri {
    float a;
    double b;
    float c;
};
static_assert(sizeof(Tri) == 24 && offsetof(Tri, b) == 8 && offsetof(Tri, c) == 16);
struct Pair {
    float t;
    float k;
};

static std::uint64_t g_state = 0x57E9C11;
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
static std::vector<float> random_floats(std::size_t n) {
    std::vector<float> v(n);
    for (float &x : v)
        x = unit();
    return v;
}

// ---- the host model: the taps in row-major order, one rounding per product and per sum ----
// s(r, c): the source cell, any r and c inside the grid; weight: row-major, converted once; cross: five taps only.
template <typename T, typename S>
static T model(S &&s, std::size_t h, std::size_t w, bool cross, const double (&weight)[9], T halo, std::size_t r, std::size_t c) {
    bool first = true;
    T acc = T();
    for (int a = -1; a <= 1; a++)
        for (int b = -1; b <= 1; b++) {
            if (cross && a != 0 && b != 0)
                continue;
            const long rr = long(r) + a, cc = long(c) + b;
            const T value = rr < 0 || cc < 0 || rr >= long(h) || cc >= long(w) ? halo : s(std::size_t(rr), std::size_t(cc));
            const T product = T(weight[3 * (a + 1) + (b + 1)]) * value;
            acc = first ? product : acc + product;
            first = false;
        }
    return acc;
}

constexpr std::size_t H = 38, W = 300; // wider than a wave's span of four floats per lane
static const double nine[9] = {0.11, -0.23, 0.37, 0.41, -0.53, 0.67, 0.71, -0.83, 0.97};
static const hip::Box9 box{{{0.11, -0.23, 0.37}, {0.41, -0.53, 0.67}, {0.71, -0.83, 0.97}}};
static const hip::Cross5 cross{-0.23, 0.41, -0.53, 0.67, -0.83};
static const double cross_nine[9] = {0.0, -0.23, 0.0, 0.41, -0.53, 0.67, 0.0, -0.83, 0.0};

static void test_planes() {
    std::vector<float> u = random_floats(H * W), f = random_floats(H * W), z = random_floats(H * W);
    hip::Grid<float> gu = grid_of(u, H, W), gf = grid_of(f, H, W), gz = grid_of(z, H, W);
    auto s = [&](std::size_t r, std::size_t c) { return u[r * W + c]; };
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // the whole grid: every border reads the halo
    for (float halo : {0.0f, -2.5f, nan}) {
        hip::apply(hip::field(gz), {0, H, 0, W}, box, hip::field(gu), halo);
        std::vector<float> got = cells_of(gz);
        bool ok = true;
        for (std::size_t r = 0; r < H; r++)
            for (std::size_t c = 0; c < W; c++)
                ok = ok && same(got[r * W + c], model<float>(s, H, W, false, nine, halo, r, c));
        REQUIRE(ok);
    }
    // an inner rectangle of a cross with a right-hand side, in place on the right-hand side; the rest keeps its values
    const hip::Rect inner{1, H - 2, 3, W - 1};
    hip::apply(hip::field(gf), inner, cross, hip::field(gu), 1.5f, 0.25, hip::field(gf));
    std::vector<float> got = cells_of(gf);
    bool ok = true;
    for (std::size_t r = 0; r < H; r++)
        for (std::size_t c = 0; c < W; c++) {
            const bool in = r >= inner.row_begin && r < inner.row_end && c >= inner.col_begin && c < inner.col_end;
            float want = f[r * W + c];
            if (in)
                want = model<float>(s, H, W, true, cross_nine, 1.5f, r, c) + 0.25f * f[r * W + c];
            ok = ok && same(got[r * W + c], want);
        }
    REQUIRE(ok);
    // the default halo is a zero
    hip::apply(hip::field(gz), {0, H, 0, W}, cross, hip::field(gu));
    got = cells_of(gz);
    ok = true;
    for (std::size_t r = 0; r < H; r++)
        for (std::size_t c = 0; c < W; c++)
            ok = ok && same(got[r * W + c], model<float>(s, H, W, true, cross_nine, 0.0f, r, c));
    REQUIRE(ok);
    // the source is untouched
    std::vector<float> still = cells_of(gu);
    REQUIRE(std::memcmp(still.data(), u.data(), u.size() * sizeof(float)) == 0);
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
    const hip::Rect whole{0, H, 0, W};
    // a member of Tri cells from another member of the same cells, the right-hand side a member of Pair cells
    hip::apply(hip::field(gt, &Tri::a), whole, box, hip::field(gt, &Tri::c), 0.5f, -2.0, hip::field(gp, &Pair::k));
    // the double member from a plane of doubles, the right-hand side the member itself
    std::vector<double> d(H * W);
    for (double &x : d)
        x = double(unit()) * 1.0e-3;
    hip::Grid<double> gd = grid_of(d, H, W);
    hip::apply(hip::field(gt, &Tri::b), {2, H, 0, W - 5}, cross, hip::field(gd), 7.0, 1.0 / 3.0, hip::field(gt, &Tri::b));
    // a member of Pair cells from the other member of the same cells
    hip::apply(hip::field(gp, &Pair::t), {0, H - 1, 1, W}, cross, hip::field(gp, &Pair::k), -1.0f);
    std::vector<Tri> got_tri = cells_of(gt);
    std::vector<Pair> got_pair = cells_of(gp);
    auto sc = [&](std::size_t r, std::size_t c) { return tri[r * W + c].c; };
    auto sd = [&](std::size_t r, std::size_t c) { return d[r * W + c]; };
    auto sk = [&](std::size_t r, std::size_t c) { return pair[r * W + c].k; };
    bool ok = true;
    for (std::size_t r = 0; r < H; r++)
        for (std::size_t c = 0; c < W; c++) {
            const std::size_t i = r * W + c;
            const float a = model<float>(sc, H, W, false, nine, 0.5f, r, c) + -2.0f * pair[i].k;
            double b = tri[i].b;
            if (r >= 2 && c < W - 5)
                b = model<double>(sd, H, W, true, cross_nine, 7.0, r, c) + (1.0 / 3.0) * tri[i].b;
            float t = pair[i].t;
            if (r < H - 1 && c >= 1)
                t = model<float>(sk, H, W, true, cross_nine, -1.0f, r, c);
            ok = ok && same(got_tri[i].a, a) && same(got_tri[i].b, b) && same(got_tri[i].c, tri[i].c) && same(got_pair[i].t, t) &&
                 same(got_pair[i].k, pair[i].k);
        }
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
    hip::Grid<float> a(8, 12), b(8, 12), f(8, 12), small(4, 6);
    hip::Grid<double> d(8, 12);
    hip::Grid<Tri> t(8, 12);
    const hip::Rect whole{0, 8, 0, 12};
    REQUIRE(throws<std::range_error>([&] { hip::apply(hip::field(a), {0, 9, 0, 12}, cross, hip::field(b)); }));
    REQUIRE(throws<std::range_error>([&] { hip::apply(hip::field(a), {0, 8, 3, 13}, box, hip::field(b)); }));
    REQUIRE(throws<std::range_error>([&] { hip::apply(hip::field(a), {5, 4, 0, 12}, cross, hip::field(b)); }));
    REQUIRE(throws<std::range_error>([&] { hip::apply(hip::field(a), whole, cross, hip::field(small)); }));
    REQUIRE(throws<std::range_error>([&] { hip::apply(hip::field(a), whole, cross, hip::field(b), 0.0f, 1.0, hip::field(small)); }));
    // element types: erased fields are checked when the call is made
    const hip::AnyField fa = hip::field(a), fb = hip::field(b), fd = hip::field(d);
    REQUIRE(throws<std::invalid_argument>([&] { hip::apply(fa, whole, STSTHIP_STENCIL_BOX9, nine, fd); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::apply(fd, whole, STSTHIP_STENCIL_BOX9, nine, hip::field(t, &Tri::c)); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::apply(fa, whole, STSTHIP_STENCIL_BOX9, nine, fb, 0.0, 1.0, fd); }));
    // a cross has no corners
    REQUIRE(throws<std::invalid_argument>([&] { hip::apply(fa, whole, STSTHIP_STENCIL_CROSS5, nine, fb); }));
    const double corner[9] = {0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1e-300};
    REQUIRE(throws<std::invalid_argument>([&] { hip::apply(fa, whole, STSTHIP_STENCIL_CROSS5, corner, fb); }));
    const double infinite[9] = {0.0, 1.0, 0.0, 1.0, std::numeric_limits<double>::infinity(), 1.0, 0.0, 1.0, 0.0};
    REQUIRE(throws<std::invalid_argument>([&] { hip::apply(fa, whole, STSTHIP_STENCIL_CROSS5, infinite, fb); }));
    // an empty rectangle is fine, anywhere inside
    hip::apply(hip::field(a), {8, 8, 3, 3}, cross, hip::field(b));
    hip::apply(hip::field(a), {2, 5, 12, 12}, box, hip::field(b), 0.0f, 1.0, hip::field(f));
    // what the library refuses arrives as an exception too: a stencil in place
    REQUIRE(throws<std::exception>([&] { hip::apply(hip::field(a), whole, cross, hip::field(a)); }));
    hip::Grid<float> alias = a; // (handles share cells)
    REQUIRE(throws<std::exception>([&] { hip::apply(hip::field(a), {1, 7, 1, 11}, box, hip::field(alias)); }));
}

// host-mirror validity: write through an accessor, apply, read through an accessor
static void test_flag_protocol() {
    hip::Grid<float> u(16, 24), v(16, 24), f(16, 24);
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> au(u), af(f);
        for (std::size_t r = 0; r < 16; r++)
            for (std::size_t c = 0; c < 24; c++) {
                au[r][c] = float(r);
                af[r][c] = float(c);
            }
    }
    const hip::Cross5 sum{1.0, 1.0, 0.0, 1.0, 1.0}; // N + W + E + S
    hip::apply(hip::field(v), {0, 16, 0, 24}, sum, hip::field(u), 0.0f, 2.0, hip::field(f)); // uploads both mirrors first
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> av(v); // downloads: the mirror no longer counted
        REQUIRE(av[5][7] == 4.0f * 5.0f + 2.0f * 7.0f);
        REQUIRE(av[0][0] == 0.0f + 0.0f + 0.0f + 1.0f);          // north and west are halo
        REQUIRE(av[15][23] == 14.0f + 15.0f + 2.0f * 23.0f);     // east and south are halo
        av[3][5] = 100.0f; // the host writes again ...
    }
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> au(u); // (a source's mirror stays valid)
        REQUIRE(au[2][7] == 2.0f);
        au[2][7] = -1.0f;
    }
    hip::Grid<float> alias = v; // handles share cells
    hip::apply(hip::field(f), {0, 16, 0, 24}, sum, hip::field(alias), 0.0f, 1.0, hip::field(u)); // ... and both writes count
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read> af(f);
        // f(3, 4) = v(2, 4) + v(3, 3) + v(3, 5) + v(4, 4) + u(3, 4)
        REQUIRE(af[3][4] == (4.0f * 2.0f + 8.0f) + (4.0f * 3.0f + 6.0f) + 100.0f + (4.0f * 4.0f + 8.0f) + 3.0f);
        // f(2, 7) = v(1, 7) + v(2, 6) + v(2, 8) + v(3, 7) + u(2, 7), and u(2, 7) is the host's -1
        REQUIRE(af[2][7] == (4.0f + 14.0f) + (8.0f + 12.0f) + (8.0f + 16.0f) + (12.0f + 14.0f) - 1.0f);
    }
    std::printf("flag protocol: accessor writes reach apply, its results reach the accessor\n");
}

int main() {
    test_planes();
    test_members();
    test_errors();
    test_flag_protocol();
    return finish("grid_operator_test");
}

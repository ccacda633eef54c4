// stencil::hip::combine / restrict_mean / prolong_bilinear (hip/Algebra.hpp) against the same formulas in plain host
// C++ (this file is built with -ffp-contract=off, so the host model rounds every product and every sum once): a
// Grid<float>, members of struct cells of another cell type, doubles; std::range_error and std::invalid_argument; and
// the validity-flag protocol between these calls and the GridAccessor.
#include "../cpp/mini_test.hpp"
#include <StencilStream/hip/Algebra.hpp>

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

static std::uint64_t g_state = 0xA16EB;
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

// ---- the host models, formula by formula ----
template <typename T> static T restrict_model(std::vector<T> const &s, std::size_t w, std::size_t r, std::size_t c) {
    return ((s[2 * r * w + 2 * c] + s[2 * r * w + 2 * c + 1]) + (s[(2 * r + 1) * w + 2 * c] + s[(2 * r + 1) * w + 2 * c + 1])) * T(0.25);
}
// fine cell (fr, fc) of the prolongation of the h x w grid `c`
template <typename T>
static T prolong_model(std::vector<T> const &c, std::size_t h, std::size_t w, T halo, std::size_t fr, std::size_t fc) {
    const long i = long(fr / 2), j = long(fc / 2);
    const long i_far = fr % 2 == 0 ? i - 1 : i + 1, j_far = fc % 2 == 0 ? j - 1 : j + 1;
    auto at = [&](long r, long q) { return r < 0 || q < 0 || r >= long(h) || q >= long(w) ? halo : c[std::size_t(r) * w + std::size_t(q)]; };
    auto along = [&](long r) { return T(0.75) * at(r, j) + T(0.25) * at(r, j_far); };
    return T(0.75) * along(i) + T(0.25) * along(i_far);
}

constexpr std::size_t H = 38, W = 70;

static void test_combine() {
    // planes of floats: three terms over an inner rectangle, the rest keeps its values
    std::vector<float> x = random_floats(H * W), y = random_floats(H * W), z = random_floats(H * W);
    hip::Grid<float> gx = grid_of(x, H, W), gy = grid_of(y, H, W), gz = grid_of(z, H, W);
    const hip::Rect inner{1, H - 2, 3, W - 1};
    const float c0 = float(0.1), c1 = float(-1.0), c2 = float(3.0e30);
    hip::combine(hip::field(gz), inner, {hip::term(0.1, gx), hip::term(-1.0, gy), hip::term(3.0e30, gz)});
    std::vector<float> got = cells_of(gz);
    bool ok = true;
    for (std::size_t r = 0; r < H; r++)
        for (std::size_t c = 0; c < W; c++) {
            const std::size_t i = r * W + c;
            const bool in = r >= inner.row_begin && r < inner.row_end && c >= inner.col_begin && c < inner.col_end;
            float want = z[i];
            if (in) {
                want = c0 * x[i];
                want = want + c1 * y[i];
                want = want + c2 * z[i];
            }
            ok = ok && same(got[i], want);
        }
    REQUIRE(ok);

    // members: a member of Tri cells from a member of Pair cells and another member of the same Tri cells, in place
    std::vector<Tri> tri(H * W);
    std::vector<Pair> pair(H * W);
    for (std::size_t i = 0; i < H * W; i++) {
        tri[i] = Tri{unit(), double(unit()), unit()};
        pair[i] = Pair{unit(), unit()};
    }
    hip::Grid<Tri> gt = grid_of(tri, H, W);
    hip::Grid<Pair> gp = grid_of(pair, H, W);
    const hip::Rect whole{0, H, 0, W};
    hip::combine(hip::field(gt, &Tri::a), whole, {hip::term(0.5, gt, &Tri::a), hip::term(2.0, gp, &Pair::k), hip::term(-0.3, gt, &Tri::c)});
    hip::combine(hip::field(gt, &Tri::b), whole, {hip::term(1.0 / 3.0, gt, &Tri::b)});
    std::vector<Tri> got_tri = cells_of(gt);
    ok = true;
    for (std::size_t i = 0; i < H * W; i++) {
        float a = 0.5f * tri[i].a;
        a = a + 2.0f * pair[i].k;
        a = a + float(-0.3) * tri[i].c;
        const double b = (1.0 / 3.0) * tri[i].b;
        ok = ok && same(got_tri[i].a, a) && same(got_tri[i].b, b) && same(got_tri[i].c, tri[i].c);
    }
    REQUIRE(ok);
    // the sources are untouched
    std::vector<Pair> got_pair = cells_of(gp);
    REQUIRE(std::memcmp(got_pair.data(), pair.data(), pair.size() * sizeof(Pair)) == 0);
}

static void test_resample() {
    const std::size_t h = 19, w = 35; // coarse
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> fine = random_floats(4 * h * w);
    hip::Grid<float> gf = grid_of(fine, 2 * h, 2 * w);
    hip::Grid<float> gc(h, w);
    hip::restrict_mean(hip::field(gc), {0, h, 0, w}, hip::field(gf));
    std::vector<float> coarse = cells_of(gc);
    bool ok = true;
    for (std::size_t r = 0; r < h; r++)
        for (std::size_t c = 0; c < w; c++)
            ok = ok && same(coarse[r * w + c], restrict_model(fine, 2 * w, r, c));
    REQUIRE(ok);

    for (float halo : {0.0f, -2.5f, nan}) {
        hip::Grid<float> back(2 * h, 2 * w);
        hip::prolong_bilinear(hip::field(back), 0, 0, hip::field(gc), {0, h, 0, w}, halo);
        std::vector<float> got = cells_of(back);
        ok = true;
        for (std::size_t r = 0; r < 2 * h; r++)
            for (std::size_t c = 0; c < 2 * w; c++)
                ok = ok && same(got[r * 2 * w + c], prolong_model(coarse, h, w, halo, r, c));
        REQUIRE(ok);
    }

    // a member of struct cells (doubles) into a plane of doubles and back into an inner rectangle of the member
    std::vector<Tri> tri(4 * h * w);
    for (Tri &t : tri)
        t = Tri{unit(), double(unit()) * 1.0e-3, unit()};
    hip::Grid<Tri> gt = grid_of(tri, 2 * h, 2 * w);
    hip::Grid<double> gd(h, w);
    hip::restrict_mean(hip::field(gd), {2, h, 1, w - 1}, hip::field(gt, &Tri::b), 3, 1); // odd source row and column
    std::vector<double> got_d = cells_of(gd);
    ok = true;
    for (std::size_t r = 0; r < h; r++)
        for (std::size_t c = 0; c < w; c++) {
            double want = 0.0; // (a fresh grid)
            if (r >= 2 && c >= 1 && c < w - 1) {
                auto s = [&](std::size_t a, std::size_t b) { return tri[(3 + 2 * (r - 2) + a) * 2 * w + 1 + 2 * (c - 1) + b].b; };
                want = ((s(0, 0) + s(0, 1)) + (s(1, 0) + s(1, 1))) * 0.25;
            }
            ok = ok && same(got_d[r * w + c], want);
        }
    REQUIRE(ok);
    hip::prolong_bilinear(hip::field(gt, &Tri::b), 4, 6, hip::field(gd), {2, 9, 3, 11}, 7.0);
    std::vector<Tri> got_t = cells_of(gt);
    ok = true;
    for (std::size_t r = 0; r < 2 * h; r++)
        for (std::size_t c = 0; c < 2 * w; c++) {
            Tri want = tri[r * 2 * w + c];
            if (r >= 4 && r < 4 + 14 && c >= 6 && c < 6 + 16) // coarse cell (2 + (r-4)/2, 3 + (c-6)/2), parity of r-4 / c-6
                want.b = prolong_model(got_d, h, w, 7.0, 2 * 2 + (r - 4), 2 * 3 + (c - 6));
            ok = ok && same(got_t[r * 2 * w + c].a, want.a) && same(got_t[r * 2 * w + c].b, want.b) &&
                 same(got_t[r * 2 * w + c].c, want.c);
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
    hip::Grid<float> a(8, 12), b(8, 12), small(4, 6), coarse(4, 6);
    hip::Grid<double> d(8, 12);
    hip::Grid<Tri> t(8, 12);
    const hip::Rect whole{0, 8, 0, 12};
    REQUIRE(throws<std::range_error>([&] { hip::combine(hip::field(a), {0, 9, 0, 12}, {hip::term(1.0, b)}); }));
    REQUIRE(throws<std::range_error>([&] { hip::combine(hip::field(a), {0, 8, 3, 13}, {hip::term(1.0, b)}); }));
    REQUIRE(throws<std::range_error>([&] { hip::combine(hip::field(a), {5, 4, 0, 12}, {hip::term(1.0, b)}); }));
    REQUIRE(throws<std::range_error>([&] { hip::combine(hip::field(a), whole, {hip::term(1.0, small)}); }));
    REQUIRE(throws<std::range_error>([&] { hip::restrict_mean(hip::field(coarse), {0, 5, 0, 6}, hip::field(a)); }));
    REQUIRE(throws<std::range_error>([&] { hip::restrict_mean(hip::field(coarse), {0, 4, 0, 6}, hip::field(a), 1, 0); }));
    REQUIRE(throws<std::range_error>([&] { hip::prolong_bilinear(hip::field(a), 0, 2, hip::field(coarse), {0, 4, 0, 6}); }));
    REQUIRE(throws<std::range_error>([&] { hip::prolong_bilinear(hip::field(a), 0, 0, hip::field(coarse), {0, 4, 2, 7}); }));
    // element types: erased fields are checked when the call is made
    const hip::AnyField fa = hip::field(a), fd = hip::field(d);
    REQUIRE(throws<std::invalid_argument>([&] { hip::combine(fa, whole, {hip::AnyTerm{1.0, fd}}); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::combine(fd, whole, {hip::AnyTerm{1.0, hip::field(t, &Tri::c)}}); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::combine(fa, whole, std::vector<hip::AnyTerm>{}); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::combine(fa, whole, std::vector<hip::AnyTerm>(5, hip::AnyTerm{1.0, fa})); }));
    // an empty rectangle is fine, anywhere inside
    hip::combine(hip::field(a), {8, 8, 3, 3}, {hip::term(1.0, b)});
    hip::restrict_mean(hip::field(coarse), {4, 4, 0, 6}, hip::field(a), 8, 0);
    // what the library refuses arrives as an exception too: a term that overlaps the destination a column further
    REQUIRE(throws<std::exception>([&] {
        hip::AnyField shifted = hip::field(a);
        auto base = shifted.for_reading;
        shifted.for_reading = [base] { ststhip_grid_view v = base(); v.base = static_cast<char *>(v.base) + 4; v.width -= 1; return v; };
        shifted.width -= 1;
        hip::combine(fa, {0, 8, 0, 11}, {hip::AnyTerm{1.0, shifted}});
    }));
}

// host-mirror validity: write through an accessor, combine, read through an accessor
static void test_flag_protocol() {
    hip::Grid<float> u(16, 24), v(16, 24);
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> au(u), av(v);
        for (std::size_t r = 0; r < 16; r++)
            for (std::size_t c = 0; c < 24; c++) {
                au[r][c] = float(r);
                av[r][c] = float(c);
            }
    }
    hip::combine(hip::field(u), {0, 16, 0, 24}, {hip::term(2.0, u), hip::term(1.0, v)}); // uploads both mirrors first
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> au(u); // downloads: the mirror no longer counted
        bool ok = true;
        for (std::size_t r = 0; r < 16; r++)
            for (std::size_t c = 0; c < 24; c++)
                ok = ok && au[r][c] == 2.0f * float(r) + float(c);
        REQUIRE(ok);
        au[3][5] = 100.0f; // the host writes again ...
    }
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> av(v); // (a source's mirror stays valid)
        REQUIRE(av[2][7] == 7.0f);
        av[2][7] = -1.0f;
    }
    hip::Grid<float> alias = u; // handles share cells
    hip::combine(hip::field(alias), {0, 16, 0, 24}, {hip::term(1.0, u), hip::term(1.0, v)}); // ... and both writes count
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read> au(u);
        REQUIRE(au[3][5] == 105.0f);
        REQUIRE(au[2][7] == 2.0f * 2.0f + 7.0f - 1.0f);
        REQUIRE(au[15][23] == 30.0f + 23.0f + 23.0f);
    }
    // a transfer's destination follows the same rule
    hip::Grid<float> coarse(8, 12);
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> ac(coarse);
        ac[0][0] = 9.0f; // a valid mirror the restriction must not leave in charge
    }
    hip::restrict_mean(hip::field(coarse), {0, 8, 0, 12}, hip::field(v));
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read> ac(coarse);
        REQUIRE(ac[0][0] == ((0.0f + 1.0f) + (0.0f + 1.0f)) * 0.25f);
        REQUIRE(ac[1][3] == ((6.0f + -1.0f) + (6.0f + 7.0f)) * 0.25f); // v[2][7] = -1 is in there
    }
    std::printf("flag protocol: accessor writes reach the combine, its results reach the accessor\n");
}

int main() {
    test_combine();
    test_resample();
    test_errors();
    test_flag_protocol();
    return finish("grid_algebra_test");
}

// stencil::hip::diffuse, jacobi_step and diagonal_solve (hip/Diffusion.hpp) against the same formula in plain host C++
// (this file is built with -ffp-contract=off, so the host model rounds every product, sum, difference and quotient
// once): planes of floats and of doubles as a whole and on a rectangle, members of struct cells with the faces and the
// right-hand side as other members; std::range_error and std::invalid_argument; and the validity-flag protocol between
// the calls and the GridAccessor.
#include "../cpp/mini_test.hpp"
#include <StencilStream/hip/Diffusion.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

using namespace stencil;

// five floats and padding: stride 32
struct Five {
    float u, kx, ky, f, out;
    float pad[3];
};
static_assert(sizeof(Five) == 32);
// a float and three doubles: stride 32, members at 0, 8, 16 and 24
struct Wide {
    float a;
    double kx, ky, v;
};
static_assert(sizeof(Wide) == 32 && offsetof(Wide, kx) == 8 && offsetof(Wide, v) == 24);

static std::uint64_t g_state = 0xD1FF;
static std::uint32_t bits() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return std::uint32_t(g_state >> 32);
}
static float unit() { return float(bits() >> 8) / float(1u << 24) - 0.5f; }
static float face() { return 0.25f + float(bits() >> 8) / float(1u << 24) * ((bits() & 1) ? 1000.0f : 1.0f); }

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

// ---- the host model: the formula of ststhip.h over a rectangle, one rounding per operation ----
enum Mode { APPLY, JACOBI, SOLVE_DIAG };
struct Scalars {
    double sigma, scale, omega, rhs_coef;
};
// out(r, c): a reference to the destination; u, kx, ky, f: values.  The destination is no source here.
template <typename T, typename Out, typename U, typename KX, typename KY, typename F>
static void model(Mode mode, Out &&out, U &&u, KX &&kx, KY &&ky, F &&f, std::size_t h, std::size_t w, hip::Rect rect, Scalars k,
                  T halo, T outside, bool has_rhs) {
    const T sigma = T(k.sigma), scale = T(k.scale), omega = T(k.omega), coef = T(k.rhs_coef);
    for (std::size_t r = rect.row_begin; r < rect.row_end; r++)
        for (std::size_t c = rect.col_begin; c < rect.col_end; c++) {
            const T kn = r == 0 ? outside : ky(r - 1, c), kw = c == 0 ? outside : kx(r, c - 1);
            const T ke = kx(r, c), ks = ky(r, c);
            T centre = T(), acc = T();
            if (mode != SOLVE_DIAG) {
                centre = u(r, c);
                const T n = r == 0 ? halo : u(r - 1, c), west = c == 0 ? halo : u(r, c - 1);
                const T e = c + 1 == w ? halo : u(r, c + 1), s = r + 1 == h ? halo : u(r + 1, c);
                acc = kn * (centre - n);
                acc = acc + kw * (centre - west);
                acc = acc + ke * (centre - e);
                acc = acc + ks * (centre - s);
            }
            T d = kn + kw;
            d = d + ke;
            d = d + ks;
            d = scale * d;
            d = sigma + d;
            if (mode == APPLY) {
                T y = sigma * centre;
                y = y + scale * acc;
                if (has_rhs)
                    y = y + coef * f(r, c);
                out(r, c) = y;
            } else if (mode == JACOBI) {
                T t = sigma * centre;
                t = t + scale * acc;
                T res = coef * f(r, c);
                res = res - t;
                out(r, c) = centre + omega * (res / d);
            } else {
                out(r, c) = (coef * f(r, c)) / d;
            }
        }
}

constexpr std::size_t H = 38, W = 300; // wider than a wave's span of four floats per lane

template <typename T> static void test_planes() {
    std::vector<T> u(H * W), kx(H * W), ky(H * W), f(H * W), out(H * W);
    for (std::size_t i = 0; i < H * W; i++)
        u[i] = unit(), kx[i] = face(), ky[i] = face(), f[i] = unit(), out[i] = unit();
    hip::Grid<T> gu = grid_of(u, H, W), gkx = grid_of(kx, H, W), gky = grid_of(ky, H, W), gf = grid_of(f, H, W),
                 gout = grid_of(out, H, W);
    auto at = [](std::vector<T> &v) { return [&v](std::size_t r, std::size_t c) -> T & { return v[r * W + c]; }; };
    const hip::Rect whole{0, H, 0, W}, inner{1, H - 2, 3, W - 1};
    const hip::Faces<T> faces{hip::field(gkx), hip::field(gky), T(1.5)};
    auto agree = [&] {
        std::vector<T> got = cells_of(gout);
        bool ok = true;
        for (std::size_t i = 0; i < H * W; i++)
            ok = ok && same(got[i], out[i]);
        return ok;
    };
    // the whole grid: every border reads the halo and the outside face
    hip::diffuse(hip::field(gout), whole, faces, 0.3, 0.7, hip::field(gu), T(-2.5));
    model<T>(APPLY, at(out), at(u), at(kx), at(ky), at(f), H, W, whole, {0.3, 0.7, 0.0, 0.0}, T(-2.5), T(1.5), false);
    REQUIRE(agree());
    // a residual r = f - A u on an inner rectangle: its neighbours outside are cells of the grid
    const T nan = std::numeric_limits<T>::quiet_NaN();
    hip::diffuse(hip::field(gout), inner, faces, 0.0, -1.0, hip::field(gu), nan, 1.0, hip::field(gf));
    model<T>(APPLY, at(out), at(u), at(kx), at(ky), at(f), H, W, inner, {0.0, -1.0, 0.0, 1.0}, nan, T(1.5), true);
    REQUIRE(agree());
    // the default halo
    hip::diffuse(hip::field(gout), whole, faces, 1.0, 0.125, hip::field(gu));
    model<T>(APPLY, at(out), at(u), at(kx), at(ky), at(f), H, W, whole, {1.0, 0.125, 0.0, 0.0}, T(0), T(1.5), false);
    REQUIRE(agree());
    // a damped Jacobi step, and the right-hand side being the destination itself
    hip::jacobi_step(hip::field(gout), whole, faces, 0.1, 1.0 / 3.0, hip::field(gu), T(0.5), 0.8, -0.3, hip::field(gf));
    model<T>(JACOBI, at(out), at(u), at(kx), at(ky), at(f), H, W, whole, {0.1, 1.0 / 3.0, 0.8, -0.3}, T(0.5), T(1.5), true);
    REQUIRE(agree());
    hip::jacobi_step(hip::field(gout), inner, faces, 0.1, 1.0, hip::field(gu), T(0.5), 0.8, 2.0, hip::field(gout));
    model<T>(JACOBI, at(out), at(u), at(kx), at(ky), at(out), H, W, inner, {0.1, 1.0, 0.8, 2.0}, T(0.5), T(1.5), true);
    REQUIRE(agree());
    // the diagonal solve
    hip::diagonal_solve(hip::field(gout), whole, faces, 0.0, 1.0, 1.0, hip::field(gf));
    model<T>(SOLVE_DIAG, at(out), at(u), at(kx), at(ky), at(f), H, W, whole, {0.0, 1.0, 0.0, 1.0}, T(0), T(1.5), true);
    REQUIRE(agree());
    // the sources are untouched
    std::vector<T> still = cells_of(gu);
    REQUIRE(std::memcmp(still.data(), u.data(), u.size() * sizeof(T)) == 0);
    still = cells_of(gkx);
    REQUIRE(std::memcmp(still.data(), kx.data(), kx.size() * sizeof(T)) == 0);
    still = cells_of(gky);
    REQUIRE(std::memcmp(still.data(), ky.data(), ky.size() * sizeof(T)) == 0);
}

static void test_members() {
    std::vector<Five> five(H * W);
    std::vector<Wide> wide(H * W);
    for (std::size_t i = 0; i < H * W; i++) {
        five[i] = Five{unit(), face(), face(), unit(), unit(), {unit(), unit(), unit()}};
        wide[i] = Wide{unit(), double(face()), double(face()), double(unit())};
    }
    hip::Grid<Five> g5 = grid_of(five, H, W);
    hip::Grid<Wide> gw = grid_of(wide, H, W);
    std::vector<double> plane(H * W);
    for (double &x : plane)
        x = double(unit());
    hip::Grid<double> gp = grid_of(plane, H, W);
    const hip::Rect whole{0, H, 0, W}, part{2, H, 0, W - 5};
    auto m5 = [&](float Five::*member) { return [&five, member](std::size_t r, std::size_t c) -> float & { return five[r * W + c].*member; }; };
    auto mw = [&](double Wide::*member) { return [&wide, member](std::size_t r, std::size_t c) -> double & { return wide[r * W + c].*member; }; };
    auto pl = [&](std::size_t r, std::size_t c) -> double & { return plane[r * W + c]; };
    // five members of one cell
    const hip::Faces<float> f5{hip::field(g5, &Five::kx), hip::field(g5, &Five::ky), 2.0f};
    hip::jacobi_step(hip::field(g5, &Five::out), whole, f5, 0.25, 0.5, hip::field(g5, &Five::u), -1.0f, 0.8, 1.0, hip::field(g5, &Five::f));
    model<float>(JACOBI, m5(&Five::out), m5(&Five::u), m5(&Five::kx), m5(&Five::ky), m5(&Five::f), H, W, whole,
                 {0.25, 0.5, 0.8, 1.0}, -1.0f, 2.0f, true);
    hip::diagonal_solve(hip::field(g5, &Five::u), part, f5, 0.25, 0.5, -2.0, hip::field(g5, &Five::out));
    model<float>(SOLVE_DIAG, m5(&Five::u), m5(&Five::u), m5(&Five::kx), m5(&Five::ky), m5(&Five::out), H, W, part,
                 {0.25, 0.5, 0.0, -2.0}, 0.0f, 2.0f, true);
    // doubles: the faces are members, the source a plane, the destination a member; then into the plane
    const hip::Faces<double> fw{hip::field(gw, &Wide::kx), hip::field(gw, &Wide::ky), 0.0};
    hip::diffuse(hip::field(gw, &Wide::v), part, fw, 0.5, 1.0 / 3.0, hip::field(gp), 7.0, 0.25, hip::field(gw, &Wide::v));
    {
        std::vector<double> before(H * W);
        for (std::size_t i = 0; i < H * W; i++)
            before[i] = wide[i].v;
        model<double>(APPLY, mw(&Wide::v), pl, mw(&Wide::kx), mw(&Wide::ky),
                      [&](std::size_t r, std::size_t c) { return before[r * W + c]; }, H, W, part, {0.5, 1.0 / 3.0, 0.0, 0.25}, 7.0, 0.0,
                      true);
    }
    hip::diffuse(hip::field(gp), whole, fw, 0.0, 1.0, hip::field(gw, &Wide::v));
    model<double>(APPLY, pl, mw(&Wide::v), mw(&Wide::kx), mw(&Wide::ky), pl, H, W, whole, {0.0, 1.0, 0.0, 0.0}, 0.0, 0.0, false);
    std::vector<Five> got5 = cells_of(g5);
    std::vector<Wide> gotw = cells_of(gw);
    std::vector<double> gotp = cells_of(gp);
    bool ok = true;
    for (std::size_t i = 0; i < H * W; i++)
        ok = ok && same(got5[i].u, five[i].u) && same(got5[i].kx, five[i].kx) && same(got5[i].ky, five[i].ky) &&
             same(got5[i].f, five[i].f) && same(got5[i].out, five[i].out) && same(got5[i].pad[0], five[i].pad[0]) &&
             same(got5[i].pad[2], five[i].pad[2]) && same(gotw[i].a, wide[i].a) && same(gotw[i].kx, wide[i].kx) &&
             same(gotw[i].ky, wide[i].ky) && same(gotw[i].v, wide[i].v) && same(gotp[i], plane[i]);
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
    hip::Grid<float> a(8, 12), u(8, 12), kx(8, 12), ky(8, 12), f(8, 12), small(4, 6);
    hip::Grid<double> d(8, 12);
    const hip::Rect whole{0, 8, 0, 12};
    const hip::Faces<float> faces{hip::field(kx), hip::field(ky), 1.0f};
    const hip::Faces<float> short_faces{hip::field(kx), hip::field(small), 1.0f};
    REQUIRE(throws<std::range_error>([&] { hip::diffuse(hip::field(a), {0, 9, 0, 12}, faces, 0.0, 1.0, hip::field(u)); }));
    REQUIRE(throws<std::range_error>([&] { hip::diffuse(hip::field(a), {0, 8, 3, 13}, faces, 0.0, 1.0, hip::field(u)); }));
    REQUIRE(throws<std::range_error>([&] { hip::diffuse(hip::field(a), {5, 4, 0, 12}, faces, 0.0, 1.0, hip::field(u)); }));
    REQUIRE(throws<std::range_error>([&] { hip::diffuse(hip::field(a), whole, faces, 0.0, 1.0, hip::field(small)); }));
    REQUIRE(throws<std::range_error>([&] { hip::diffuse(hip::field(a), whole, short_faces, 0.0, 1.0, hip::field(u)); }));
    REQUIRE(throws<std::range_error>([&] { hip::diagonal_solve(hip::field(a), whole, faces, 0.0, 1.0, 1.0, hip::field(small)); }));
    // element types: erased fields are checked when the call is made
    const hip::AnyField fa = hip::field(a), fu = hip::field(u), fd = hip::field(d);
    const hip::AnyFaces any{hip::field(kx), hip::field(ky), 1.0}, mixed{hip::field(kx), fd, 1.0};
    REQUIRE(throws<std::invalid_argument>([&] { hip::diffuse(fa, whole, any, 0.0, 1.0, fd); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::diffuse(fa, whole, mixed, 0.0, 1.0, fu); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::jacobi_step(fa, whole, any, 0.0, 1.0, fu, 0.0, 0.8, 1.0, fd); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::diagonal_solve(fa, whole, any, 0.0, 1.0, 1.0, fd); }));
    // scalars
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    REQUIRE(throws<std::invalid_argument>([&] { hip::diffuse(hip::field(a), whole, faces, inf, 1.0, hip::field(u)); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::diffuse(hip::field(a), whole, faces, 0.0, nan, hip::field(u)); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::diffuse(hip::field(a), whole, faces, 0.0, 1.0, hip::field(u), 0.0f, inf, hip::field(f)); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::jacobi_step(hip::field(a), whole, faces, 0.0, 1.0, hip::field(u), 0.0f, nan, 1.0, hip::field(f)); }));
    REQUIRE(throws<std::invalid_argument>([&] { hip::diagonal_solve(hip::field(a), whole, faces, 0.0, 1.0, nan, hip::field(f)); }));
    // an empty rectangle is fine, anywhere inside
    hip::diffuse(hip::field(a), {8, 8, 3, 3}, faces, 0.0, 1.0, hip::field(u));
    hip::jacobi_step(hip::field(a), {2, 5, 12, 12}, faces, 0.0, 1.0, hip::field(u), 0.0f, 0.8, 1.0, hip::field(f));
    // what the library refuses arrives as an exception too: the source, or a face field, as the destination
    REQUIRE(throws<std::exception>([&] { hip::diffuse(hip::field(a), whole, faces, 0.0, 1.0, hip::field(a)); }));
    REQUIRE(throws<std::exception>([&] { hip::diffuse(hip::field(kx), whole, faces, 0.0, 1.0, hip::field(u)); }));
    hip::Grid<float> alias = a; // (handles share cells)
    REQUIRE(throws<std::exception>([&] { hip::diffuse(hip::field(a), {1, 7, 1, 11}, faces, 0.0, 1.0, hip::field(alias)); }));
}

// host-mirror validity: write through an accessor, compute, read through an accessor
static void test_flag_protocol() {
    hip::Grid<float> u(16, 24), kx(16, 24), ky(16, 24), out(16, 24);
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> au(u), ax(kx), ay(ky);
        for (std::size_t r = 0; r < 16; r++)
            for (std::size_t c = 0; c < 24; c++) {
                au[r][c] = float(r * c);
                ax[r][c] = 1.0f;
                ay[r][c] = 2.0f;
            }
    }
    const hip::Faces<float> faces{hip::field(kx), hip::field(ky), 4.0f};
    hip::diffuse(hip::field(out), {0, 16, 0, 24}, faces, 0.0, 1.0, hip::field(u), 0.0f); // uploads the three mirrors first
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> ao(out), ax(kx); // downloads
        // (5, 7): 2 (35 - 28) + 1 (35 - 30) + 1 (35 - 40) + 2 (35 - 42)
        REQUIRE(ao[5][7] == 0.0f);
        // (0, 0): u = 0 and all four neighbours are 0
        REQUIRE(ao[0][0] == 0.0f);
        // (1, 1): 2 (1 - 0) + 1 (1 - 0) + 1 (1 - 2) + 2 (1 - 2)
        REQUIRE(ao[1][1] == 0.0f);
        // (15, 23): south and east are the halo 0: 2 (345 - 322) + 1 (345 - 330) + 1 * 345 + 2 * 345
        REQUIRE(ao[15][23] == 46.0f + 15.0f + 345.0f + 690.0f);
        ax[5][7] = 11.0f; // the host writes again ...
    }
    hip::diffuse(hip::field(out), {0, 16, 0, 24}, faces, 0.0, 1.0, hip::field(u), 0.0f); // ... and the write counts
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read> ao(out);
        REQUIRE(ao[5][7] == 10.0f * (35.0f - 40.0f)); // the east face of (5, 7) grew by 10
        REQUIRE(ao[5][8] == 10.0f * (40.0f - 35.0f)); // ... which is the west face of (5, 8)
    }
    hip::diagonal_solve(hip::field(u), {0, 16, 0, 24}, faces, 0.0, 1.0, 6.0, hip::field(out));
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read> au(u);
        REQUIRE(au[5][7] == 6.0f * -50.0f / (2.0f + 1.0f + 11.0f + 2.0f));
        REQUIRE(au[0][0] == 0.0f); // d = 4 + 4 + 1 + 2
    }
    std::printf("flag protocol: accessor writes reach the operator, its results reach the accessor\n");
}

int main() {
    test_planes<float>();
    test_planes<double>();
    test_members();
    test_errors();
    test_flag_protocol();
    return finish("grid_diffusion_test");
}

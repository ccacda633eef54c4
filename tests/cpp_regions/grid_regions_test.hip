// stencil::hip::read / write / fill / copy (hip/Region.hpp) against host loops on a Grid<float> and on a grid of
// three-member struct cells, the validity-flag protocol between them and the GridAccessor, and a five-point functor
// with a source injected between two StencilUpdate calls against stencil::cpu doing the same through accessors.
#include "../cpp/mini_test.hpp"
#include <StencilStream/BaseTransitionFunction.hpp>
#include <StencilStream/cpu/StencilUpdate.hpp>
#include <StencilStream/hip/Region.hpp>
#include <StencilStream/hip/StencilUpdate.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

using namespace stencil;

// a float, a double and an int: stride 24, members at 0, 8 and 16, four bytes of padding nobody names
struct Tri {
    float a;
    double b;
    std::int32_t c;
};
static_assert(sizeof(Tri) == 24 && offsetof(Tri, b) == 8 && offsetof(Tri, c) == 16);

// a heat cell: the temperature diffuses, the conductivity stays
struct Heat {
    float t;
    float k;
};
struct Diffuse : public BaseTransitionFunction {
    using Cell = Heat;
    float c;
    Heat operator()(Stencil<Heat, 1> const &s) const {
        return Heat{c * s[-1][0].t + c * s[0][-1].t + c * s[1][0].t + c * s[0][1].t + s[0][0].k * s[0][0].t, s[0][0].k};
    }
};
// two generations per launch on one pipeline shape: what is tested here does not depend on the shape, and the file
// compiles in a fraction of the time
namespace stencil {
namespace hip {
template <> struct SweepTuning<Diffuse, false> {
    static constexpr int cells_per_lane = 2;
    static constexpr int max_generations = 2;
    static constexpr int prefetch_rows = 4;
    static constexpr bool interior_variant = false;
    static constexpr int min_waves_per_simd = 1;
    static constexpr bool narrow_form = false;
};
} // namespace hip
} // namespace stencil

static std::uint64_t g_state = 0x5EED;
static std::uint32_t bits() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return std::uint32_t(g_state >> 32);
}
static float unit() { return float(bits() >> 8) / float(1u << 24); }

template <typename T> static bool same_bytes(T const &x, T const &y) { return std::memcmp(&x, &y, sizeof(T)) == 0; }
static bool same(Tri const &x, Tri const &y) { return same_bytes(x.a, y.a) && same_bytes(x.b, y.b) && x.c == y.c; }
static bool same(float x, float y) { return same_bytes(x, y); }

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
// the grid equals the host's model of it, cell by cell
template <typename Cell> static bool holds(hip::Grid<Cell> &grid, std::vector<Cell> const &model) {
    typename hip::Grid<Cell>::template GridAccessor<sycl::access::mode::read> ac(grid);
    const std::size_t h = grid.get_grid_height(), w = grid.get_grid_width();
    bool all = true;
    for (std::size_t r = 0; r < h; r++)
        for (std::size_t c = 0; c < w; c++)
            all = all && same(ac[r][c], model[r * w + c]);
    return all;
}

constexpr std::size_t H = 61, W = 67;

static void test_float_grid() {
    std::vector<float> model(H * W);
    for (float &v : model)
        v = unit();
    hip::Grid<float> grid = grid_of(model, H, W);

    // read: a rectangle, the whole grid, a decimated rectangle that ends in the last row and column
    const hip::Rect inner{3, 58, 5, 66};
    std::vector<float> got = hip::read(grid, inner);
    REQUIRE(got.size() == 55 * 61);
    bool ok = true;
    for (std::size_t r = 0; r < 55; r++)
        for (std::size_t c = 0; c < 61; c++)
            ok = ok && same(got[r * 61 + c], model[(3 + r) * W + 5 + c]);
    REQUIRE(ok);
    got = hip::read(grid, {0, H, 0, W});
    REQUIRE(got.size() == H * W && std::memcmp(got.data(), model.data(), H * W * sizeof(float)) == 0);
    got = hip::read(grid, {1, H, 2, W}, {7, 3}); // rows 1, 8, .. 57: 9; columns 2, 5, .. 65: 22
    REQUIRE(got.size() == 9 * 22);
    ok = got.size() == 9 * 22;
    for (std::size_t r = 0; ok && r < 9; r++)
        for (std::size_t c = 0; c < 22; c++)
            ok = ok && same(got[r * 22 + c], model[(1 + 7 * r) * W + 2 + 3 * c]);
    REQUIRE(ok);

    // write
    std::vector<float> patch(4 * 9);
    for (float &v : patch)
        v = -unit();
    hip::write(grid, {57, 61, 58, 67}, patch.data());
    for (std::size_t r = 0; r < 4; r++)
        for (std::size_t c = 0; c < 9; c++)
            model[(57 + r) * W + 58 + c] = patch[r * 9 + c];
    REQUIRE(holds(grid, model));

    // fill: the bits of -0.0 arrive as they are
    hip::fill(grid, {10, 13, 20, 23}, -0.0f);
    for (std::size_t r = 10; r < 13; r++)
        for (std::size_t c = 20; c < 23; c++)
            model[r * W + c] = -0.0f;
    REQUIRE(holds(grid, model));

    // copy: between two grids with a step, and inside one grid between disjoint rectangles
    std::vector<float> other_model(H * W);
    for (float &v : other_model)
        v = 2.0f + unit();
    hip::Grid<float> other = grid_of(other_model, H, W);
    hip::copy(other, 4, 6, grid, {0, 60, 1, 67}, {2, 3}); // 30 x 22
    for (std::size_t r = 0; r < 30; r++)
        for (std::size_t c = 0; c < 22; c++)
            other_model[(4 + r) * W + 6 + c] = model[(2 * r) * W + 1 + 3 * c];
    REQUIRE(holds(other, other_model));
    REQUIRE(holds(grid, model));
    hip::copy(grid, 40, 0, grid, {0, 20, 30, 67});
    for (std::size_t r = 0; r < 20; r++)
        for (std::size_t c = 0; c < 37; c++)
            model[(40 + r) * W + c] = model[r * W + 30 + c];
    REQUIRE(holds(grid, model));

    // nothing is clipped
    auto throws = [&](auto &&call) {
        try {
            call();
        } catch (std::range_error const &) {
            return true;
        }
        return false;
    };
    REQUIRE(throws([&] { hip::read(grid, {0, H + 1, 0, W}); }));
    REQUIRE(throws([&] { hip::read(grid, {0, H, 5, W + 1}); }));
    REQUIRE(throws([&] { hip::read(grid, {7, 6, 0, W}); }));
    REQUIRE(throws([&] { hip::write(grid, {60, 62, 0, 1}, patch.data()); }));
    REQUIRE(throws([&] { hip::fill(grid, {0, 1, 66, 68}, 1.0f); }));
    REQUIRE(throws([&] { hip::copy(other, 60, 0, grid, {0, 2, 0, 2}); }));
    REQUIRE(throws([&] { hip::copy(other, 0, 0, grid, {0, H + 1, 0, 2}); }));
    REQUIRE(holds(grid, model));
    // an empty rectangle is no error and no work
    REQUIRE(hip::read(grid, {5, 5, 0, W}).empty());
}

static void test_struct_cells() {
    std::vector<Tri> model(H * W);
    for (Tri &v : model)
        v = Tri{unit(), double(unit()) * 1e3, std::int32_t(bits())};
    hip::Grid<Tri> grid = grid_of(model, H, W);

    // read: whole cells and every member
    std::vector<Tri> cells = hip::read(grid, {2, 61, 0, 66}, {3, 5}); // 20 x 14
    REQUIRE(cells.size() == 20 * 14);
    bool ok = cells.size() == 20 * 14;
    for (std::size_t r = 0; ok && r < 20; r++)
        for (std::size_t c = 0; c < 14; c++)
            ok = ok && same(cells[r * 14 + c], model[(2 + 3 * r) * W + 5 * c]);
    REQUIRE(ok);
    std::vector<float> a = hip::read(grid, &Tri::a, {0, H, 0, W});
    std::vector<double> b = hip::read(grid, &Tri::b, {1, 60, 3, 67});
    std::vector<std::int32_t> c32 = hip::read(grid, &Tri::c, {0, H, 0, W}, {2, 2}); // 31 x 34
    REQUIRE(a.size() == H * W && b.size() == 59 * 64 && c32.size() == 31 * 34);
    ok = a.size() == H * W && b.size() == 59 * 64 && c32.size() == 31 * 34;
    for (std::size_t r = 0; ok && r < H; r++)
        for (std::size_t c = 0; c < W; c++) {
            ok = ok && same_bytes(a[r * W + c], model[r * W + c].a);
            if (r >= 1 && r < 60 && c >= 3)
                ok = ok && same_bytes(b[(r - 1) * 64 + c - 3], model[r * W + c].b);
            if (r % 2 == 0 && c % 2 == 0)
                ok = ok && c32[(r / 2) * 34 + c / 2] == model[r * W + c].c;
        }
    REQUIRE(ok);

    // write a member: the other members keep their bytes
    std::vector<double> patch(5 * 7);
    for (double &v : patch)
        v = -double(unit());
    hip::write(grid, &Tri::b, {56, 61, 60, 67}, patch.data());
    for (std::size_t r = 0; r < 5; r++)
        for (std::size_t c = 0; c < 7; c++)
            model[(56 + r) * W + 60 + c].b = patch[r * 7 + c];
    REQUIRE(holds(grid, model));
    // write whole cells
    std::vector<Tri> block(3 * 4);
    for (Tri &v : block)
        v = Tri{-unit(), -1.0, -7};
    hip::write(grid, {0, 3, 63, 67}, block.data());
    for (std::size_t r = 0; r < 3; r++)
        for (std::size_t c = 0; c < 4; c++)
            model[r * W + 63 + c] = block[r * 4 + c];
    REQUIRE(holds(grid, model));

    // fill a member and a cell
    hip::fill(grid, &Tri::c, {0, H, 11, 12}, std::int32_t(-42));
    for (std::size_t r = 0; r < H; r++)
        model[r * W + 11].c = -42;
    const Tri mark{1.5f, -0.0, 9};
    hip::fill(grid, {30, 33, 30, 33}, mark);
    for (std::size_t r = 30; r < 33; r++)
        for (std::size_t c = 30; c < 33; c++)
            model[r * W + c] = mark;
    REQUIRE(holds(grid, model));

    // copy into a second grid
    hip::Grid<Tri> other(H, W);
    std::vector<Tri> other_model(H * W, Tri{});
    hip::copy(other, 1, 2, grid, {0, 60, 0, 65});
    for (std::size_t r = 0; r < 60; r++)
        for (std::size_t c = 0; c < 65; c++)
            other_model[(1 + r) * W + 2 + c] = model[r * W + c];
    REQUIRE(holds(other, other_model));
}

// what the validity flags promise
static void test_flag_protocol() {
    std::vector<float> model(H * W, 1.0f);
    hip::Grid<float> grid = grid_of(model, H, W);
    REQUIRE(hip::read(grid, {0, 1, 0, 1})[0] == 1.0f); // (the cells are in HBM now)
    // a write through a GridAccessor is seen by read
    {
        hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> ac(grid);
        ac[7][9] = 5.0f;
    }
    model[7 * W + 9] = 5.0f;
    REQUIRE(hip::read(grid, {7, 8, 9, 10})[0] == 5.0f);
    // a fill is seen by a following GridAccessor
    hip::fill(grid, {20, 22, 0, W}, 3.0f);
    for (std::size_t c = 0; c < 2 * W; c++)
        model[20 * W + c] = 3.0f;
    REQUIRE(holds(grid, model));
    // a fill is seen through a second handle of the same grid, and a fill through that one through the first
    hip::Grid<float> handle = grid;
    hip::fill(grid, {40, 41, 3, 6}, 4.0f);
    for (std::size_t c = 3; c < 6; c++)
        model[40 * W + c] = 4.0f;
    REQUIRE(holds(handle, model));
    hip::fill(handle, {41, 42, 3, 6}, 6.0f);
    for (std::size_t c = 3; c < 6; c++)
        model[41 * W + c] = 6.0f;
    REQUIRE(hip::read(grid, {41, 42, 3, 4})[0] == 6.0f);
    REQUIRE(holds(grid, model));
    // a fill of a grid that was never on the device starts from its value-initialised cells
    hip::Grid<float> fresh(8, 8);
    hip::fill(fresh, {1, 2, 1, 2}, 2.0f);
    std::vector<float> fresh_model(64, 0.0f);
    fresh_model[9] = 2.0f;
    REQUIRE(holds(fresh, fresh_model));
}

// 8 generations, a 3 x 3 source, 8 more, one member of every second cell: stencil::hip with fill and read against
// stencil::cpu through accessors, bit for bit
static void test_source_between_two_updates() {
    const std::size_t h = 64, w = 64, k = 8;
    const Diffuse f{.c = 0.15f};
    std::vector<Heat> start(h * w);
    for (Heat &v : start)
        v = Heat{unit(), 0.2f + 0.2f * unit()};
    const Heat halo{0.0f, 0.0f};

    hip::StencilUpdate<Diffuse> update({.transition_function = f, .halo_value = halo, .n_iterations = k});
    hip::Grid<Heat> grid = grid_of(start, h, w);
    grid = update(grid); // non-blocking: the fill is queued behind it
    hip::fill(grid, &Heat::t, {30, 33, 40, 43}, 100.0f);
    grid = update(grid);
    const std::vector<float> got = hip::read(grid, &Heat::t, {0, h, 0, w}, {2, 2});

    cpu::StencilUpdate<Diffuse> cpu_update({.transition_function = f, .halo_value = halo, .n_iterations = k, .blocking = true});
    cpu::Grid<Heat> cpu_grid(h, w);
    {
        cpu::Grid<Heat>::GridAccessor<sycl::access::mode::read_write> ac(cpu_grid);
        for (std::size_t r = 0; r < h; r++)
            for (std::size_t c = 0; c < w; c++)
                ac[r][c] = start[r * w + c];
    }
    cpu_grid = cpu_update(cpu_grid);
    {
        cpu::Grid<Heat>::GridAccessor<sycl::access::mode::read_write> ac(cpu_grid);
        for (std::size_t r = 30; r < 33; r++)
            for (std::size_t c = 40; c < 43; c++)
                ac[r][c].t = 100.0f;
    }
    cpu_grid = cpu_update(cpu_grid);

    REQUIRE(got.size() == 32 * 32);
    bool all = got.size() == 32 * 32, moved = false;
    {
        cpu::Grid<Heat>::GridAccessor<sycl::access::mode::read> want(cpu_grid);
        for (std::size_t r = 0; all && r < 32; r++)
            for (std::size_t c = 0; c < 32; c++) {
                const float x = want[2 * r][2 * c].t;
                all = all && same_bytes(got[r * 32 + c], x);
                moved = moved || x > 1.0f; // (the source is there: nothing else exceeds 1)
            }
    }
    REQUIRE(all);
    REQUIRE(moved);
    std::printf("source between two updates: %zu + %zu generations, 32 x 32 values of one member equal\n", k, k);
}

int main() {
    test_float_grid();
    test_struct_cells();
    test_flag_protocol();
    test_source_between_two_updates();
    return finish("grid_regions_test");
}

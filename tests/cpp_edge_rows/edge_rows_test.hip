// Which waves call a transition function's row form (include/StencilStream/hip/internal/Sweep.hpp: row form, edge
// waves).  The canary is a radius-1 function of one float whose per-cell path is honest and whose row_at_level is the
// same level plus a constant no honest result comes near: a cell carries the constant iff the wave that produced it
// called the row form.  ONE launch on a 71 x 701 grid in row chunks of sixteen rows, at depth 1 (independent waves) and
// at the compiled depth 4 (four stages of one level):
//   Canary                        every cell of the grid carries the constant, in edge units and check-free units alike;
//   Canary, row_form_edges=false  exactly the cells of the edge units do not.
// The units' rectangles are predicted here from Sweep::entry's condition for the check-free code.
// Run by tests/test_edge_rows_cpp_gpu.py.
#include <StencilStream/BaseTransitionFunction.hpp>
#include <StencilStream/hip/StencilUpdate.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace {

constexpr float mark = 1024.0f;
constexpr int chunk = 16;

template <int V> struct Canary : public stencil::BaseTransitionFunction {
    using Cell = float;

    // a weighted mean: values that start in [0, 1) stay there
    STST_HD static float mean(float n, float w, float c, float e, float s) {
        return 0.5f * c + 0.125f * (n + w) + 0.125f * (e + s);
    }
    STST_HD float operator()(stencil::Stencil<float, 1> const &s) const {
        return mean(s[-1][0], s[0][-1], s[0][0], s[0][1], s[1][0]);
    }
    // rows in lane order (c0, c2, c1, c3)
    template <int level, int levels, typename Shifts>
    STST_HD void row_at_level(Shifts sh, float const (&north)[4], float const (&centre)[4], float const (&south)[4],
                              float (&out)[4]) const {
        const float west = sh.west(centre[3]), east = sh.east(centre[0]);
        out[0] = mark + mean(north[0], west, centre[0], centre[2], south[0]);      // c0: west is the neighbour lane's c3
        out[2] = mark + mean(north[2], centre[0], centre[2], centre[1], south[2]); // c1
        out[1] = mark + mean(north[1], centre[2], centre[1], centre[3], south[1]); // c2
        out[3] = mark + mean(north[3], centre[1], centre[3], east, south[3]);      // c3: east is the neighbour lane's c0
    }
};

} // namespace

namespace stencil::hip {
template <int V, bool SOA> struct SweepTuning<Canary<V>, SOA> {
    static constexpr int cells_per_lane = 4;
    static constexpr int max_generations = 4;
    static constexpr int prefetch_rows = 4;
    static constexpr bool interior_variant = true;
    static constexpr int min_waves_per_simd = 1;
    static constexpr int stages = 4;
    static constexpr bool narrow_form = false;
    static constexpr bool row_form_edges = (V == 0);
};
} // namespace stencil::hip

namespace {

namespace hi = stencil::hip::internal;

// One launch of depth N; returns the number of cells that are not what the prediction says.
template <int V, int N> long run(std::size_t h, std::size_t w) {
    using F = Canary<V>;
    using SW = hi::SweepOf<F, false, N>;
    static_assert(hi::has_row_form<F>() && SW::ROW_FORM && SW::EDGE_ROW_FORM == (V == 0) && SW::OW == 256 - 2 * SW::GX);
    std::mt19937 rng(0xed6e + N);
    std::uniform_real_distribution<float> uniform(0.0f, 1.0f);
    stencil::hip::Grid<float> grid(h, w);
    {
        stencil::hip::Grid<float>::GridAccessor<sycl::access::mode::read_write> ac(grid);
        for (std::size_t r = 0; r < h; r++)
            for (std::size_t c = 0; c < w; c++)
                ac[r][c] = uniform(rng);
    }
    stencil::hip::StencilUpdate<F> update({.transition_function = F{}, .halo_value = 0.0f, .n_iterations = std::size_t(N), .blocking = true});
    stencil::hip::Grid<float> out = update(grid);

    // the cells check-free units produce (Sweep::entry: the footprint -- 64 lanes of columns, the chunk's rows and the
    // depth on either side -- lies inside the grid, and starts at a positive column)
    std::vector<char> check_free(h * w, 0);
    long units = 0, edge_units = 0;
    const int n_strips = (int(w) + SW::OW - 1) / SW::OW, n_chunks = (int(h) + chunk - 1) / chunk;
    for (int strip = 0; strip < n_strips; strip++)
        for (int k = 0; k < n_chunks; k++) {
            const int ya = k * chunk, yb = std::min(ya + chunk, int(h));
            const int xw0 = strip * SW::OW - SW::GX;
            if (!(xw0 > 0 && xw0 + SW::LW <= int(w) && ya - SW::G >= 0 && yb + SW::G <= int(h))) {
                edge_units++;
                continue;
            }
            units++;
            for (int r = ya; r < yb; r++)
                for (int x = strip * SW::OW; x < std::min((strip + 1) * SW::OW, int(w)); x++)
                    check_free[std::size_t(r) * w + std::size_t(x)] = 1;
        }
    long wrong = 0, marked = 0;
    {
        stencil::hip::Grid<float>::GridAccessor<sycl::access::mode::read> ac(out);
        for (std::size_t r = 0; r < h; r++)
            for (std::size_t c = 0; c < w; c++) {
                const float v = ac[r][c];
                const bool carries = v >= mark, honest = v >= 0.0f && v < 1.0f;
                const bool want = V == 0 || check_free[r * w + c];
                marked += carries;
                if ((want ? !carries : !honest) && wrong++ < 5)
                    std::printf("  variant %d depth %d: cell (%zu, %zu) = %g, row form %s\n", V, N, r, c, double(v),
                                want ? "expected" : "not expected");
            }
    }
    std::printf("edge_rows_test: row_form_edges=%d depth %d: %ld check-free and %ld edge units, %ld of %zu cells carry the mark, "
                "%ld wrong\n", int(V == 0), N, units, edge_units, marked, h * w, wrong);
    // a plan without both kinds of units has not tested what this is for
    if (units == 0 || edge_units == 0)
        wrong++;
    return wrong;
}

} // namespace

int main() {
    // the plan the prediction is written for: row chunks of sixteen rows, one tier
    setenv("STSTHIP_CHUNK_ROWS", "16", 1);
    setenv("STSTHIP_TAPER", "", 1);
    for (const char *knob : {"STSTHIP_LAST_CHUNK_EARLY", "STSTHIP_XCD_REMAP", "STSTHIP_NARROW_BAND_ROWS", "STSTHIP_MAX_GENERATIONS",
                             "STSTHIP_VIRTUAL_STRIPS", "STSTHIP_TAIL_PERMILLE"})
        unsetenv(knob);
    ststhip_reload_options();
    if (hi::options().chunk_rows != chunk || hi::options().n_taper != 0) {
        std::printf("edge_rows_test: the plan is not chunks of %d rows\n", chunk);
        return 2;
    }
    long failures = 0;
    failures += run<0, 1>(71, 701);
    failures += run<1, 1>(71, 701);
    failures += run<0, 4>(71, 701);
    failures += run<1, 4>(71, 701);
    std::printf("edge_rows_test: %ld failures\n", failures);
    return failures ? 1 : 0;
}

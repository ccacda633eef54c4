// Host test of the packed row form of the uniform Jacobi kernel (include/StencilStream/hip/forms/Jacobi5Uniform.hpp):
// row_at_level on rows in lane order (c0, c2, c1, c3) against at_level cell by cell, bit for bit, for the four launch
// variants and the levels that differ (first, middle, last, only level of a launch).  A row is `lanes` lanes of four
// cells with one more cell on either side; a lane's shifts hand it the neighbouring lanes' cells (the outer cells for
// the first and the last lane), as the sweep's DPP shifts do.  Values: random, with subnormals, +-0, +-inf, NaN and
// numbers near the overflow threshold planted in most rows.  NaNs are compared by position (tests/special_values.py:
// which NaN an operation makes is the machine's business), everything else by its bits.
// Built with the ROCm installation's clang and -ffp-contract=off (Makefile); run by tests/test_packed_rows_cpu.py.
#include <StencilStream/hip/forms/Jacobi5Uniform.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

namespace {

constexpr int lanes = 5;
constexpr int width = 4 * lanes + 2; // column 0 and column width-1: the cells beyond the row's lanes

struct HostShifts {
    float from_west, from_east;
    float west(float) const { return from_west; }
    float east(float) const { return from_east; }
};

std::uint32_t bits(float v) {
    std::uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

float special(std::mt19937 &rng) {
    const float least = std::numeric_limits<float>::denorm_min();
    const float inf = std::numeric_limits<float>::infinity();
    switch (rng() % 12) {
    case 0: return least * float(1 + rng() % 1000);
    case 1: return -least * float(1 + rng() % 1000);
    case 2: return std::numeric_limits<float>::min() * 0.75f; // a large subnormal
    case 3: return 0.0f;
    case 4: return -0.0f;
    case 5: return inf;
    case 6: return -inf;
    case 7: return std::numeric_limits<float>::quiet_NaN();
    case 8: return std::numeric_limits<float>::max() * 0.3f; // sums of these overflow
    case 9: return -std::numeric_limits<float>::max() * 0.3f;
    case 10: return std::numeric_limits<float>::min() * 3.0f; // c * this is subnormal
    default: return -std::numeric_limits<float>::min() * 1.5f;
    }
}

void to_lane_order(const float *cells, float (&row)[4]) {
    row[0] = cells[0];
    row[1] = cells[2];
    row[2] = cells[1];
    row[3] = cells[3];
}

template <bool First, bool Last, int level, int levels>
long check(int n_rows, unsigned seed, float c, long &n_special_results) {
    using F = stencil::apps::Jacobi5Uniform<First, Last>;
    using St = stencil::Stencil<float, 1>;
    typename F::Block block{c};
    const F f = F::from_params(block);
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> uniform(-1.0f, 1.0f);
    long failures = 0;
    for (int r = 0; r < n_rows; r++) {
        float grid[3][width];
        for (auto &row : grid)
            for (float &v : row)
                v = uniform(rng);
        if (r % 4 != 0) // three rows in four carry special values, a few or many
            for (int n = 1 + int(rng() % (r % 4 == 1 ? 3 : 24)); n > 0; n--)
                grid[rng() % 3][rng() % width] = special(rng);
        for (int lane = 0; lane < lanes; lane++) {
            const int x = 1 + 4 * lane; // column of the lane's c0
            float north[4], centre[4], south[4], out[4];
            to_lane_order(&grid[0][x], north);
            to_lane_order(&grid[1][x], centre);
            to_lane_order(&grid[2][x], south);
            // the lane to the west holds column x-1 as its c3, the lane to the east column x+4 as its c0
            const HostShifts sh{grid[1][x - 1], grid[1][x + 4]};
            f.template row_at_level<level, levels>(sh, north, centre, south, out);
            const float got[4] = {out[0], out[2], out[1], out[3]}; // back from lane order
            for (int k = 0; k < 4; k++) {
                St st(sycl::id<2>(7, std::size_t(x + k)), sycl::range<2>(64, 1024), 0, 0, std::monostate{});
                for (int rr = 0; rr < 3; rr++)
                    for (int cc = 0; cc < 3; cc++)
                        st[sycl::id<2>(rr, cc)] = grid[rr][x + k - 1 + cc];
                const float want = f.template at_level<level, levels>(st);
                const bool same = (std::isnan(got[k]) && std::isnan(want)) ||
                                  (!std::isnan(got[k]) && !std::isnan(want) && bits(got[k]) == bits(want));
                if (!std::isnormal(want))
                    n_special_results++;
                if (!same && failures++ < 10)
                    std::printf("  first=%d last=%d level %d of %d, row %d lane %d cell %d: got %a (%#x), want %a (%#x)\n",
                                int(First), int(Last), level, levels, r, lane, k, got[k], bits(got[k]), want, bits(want));
            }
        }
    }
    return failures;
}

template <bool First, bool Last> long check_variant(int n_rows) {
    long failures = 0, n_special = 0;
    unsigned seed = 0x5eed0000u + unsigned(First) * 2 + unsigned(Last);
    for (float c : {0.2f, 0.25f, 1.0f / 3.0f}) {
        failures += check<First, Last, 0, 1>(n_rows, seed++, c, n_special); // the only level of a launch
        failures += check<First, Last, 0, 4>(n_rows, seed++, c, n_special); // first
        failures += check<First, Last, 2, 4>(n_rows, seed++, c, n_special); // middle
        failures += check<First, Last, 3, 4>(n_rows, seed++, c, n_special); // last
    }
    std::printf("packed_rows_test: first=%d last=%d: %d rows of %d lanes per level and coefficient, %ld results that are "
                "zero, subnormal or not finite, %ld failures\n",
                int(First), int(Last), n_rows, lanes, n_special, failures);
    // a run in which nothing special came out has not tested what it is for
    if (n_special < n_rows)
        failures++;
    return failures;
}

} // namespace

int main(int argc, char **argv) {
    const char *variant = argc > 1 ? argv[1] : "all";
    const int n_rows = argc > 2 ? std::atoi(argv[2]) : 20000;
    const bool all = std::strcmp(variant, "all") == 0;
    long failures = 0;
    bool known = all;
    if (all || std::strcmp(variant, "middle") == 0)
        failures += check_variant<false, false>(n_rows), known = true;
    if (all || std::strcmp(variant, "first") == 0)
        failures += check_variant<true, false>(n_rows), known = true;
    if (all || std::strcmp(variant, "last") == 0)
        failures += check_variant<false, true>(n_rows), known = true;
    if (all || std::strcmp(variant, "only") == 0)
        failures += check_variant<true, true>(n_rows), known = true;
    if (!known) {
        std::printf("usage: packed_rows_test [all|middle|first|last|only] [rows]\n");
        return 2;
    }
    std::printf("packed_rows_test: %ld failures\n", failures);
    return failures ? 1 : 0;
}

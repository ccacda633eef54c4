// What a transition function may add to the plain protocol (interior(), at_level<level, levels>(),
// constant_fields, halo_columns_per_generation, an explicit SweepTuning, state of its own, the strategies for the
// time-dependent values), on hash functors in the scheme of shape_cases.hpp: swept by stencil::hip::StencilUpdate,
// compared with stencil::cpu::StencilUpdate field by field.  A hook that is used where its promise does not hold, or a
// hint that is honoured where it must not be, can only produce a wrong number: every functor here reads and writes
// what the plain ones do.
//
// The file is included by the HIP binaries shape_test_e ... (the functors, their tunings, the static asserts and the
// canary's driver) and by the host-only shape_host_test (the functors alone).  Every functor that is not about the
// rule's own shape or a stated explicit one carries a shallow explicit tuning (four generations at the most, no narrow
// form): the sweeps of a functor are compiled per depth, stage and code path.
#pragma once
#include "shape_cases.hpp"

#include <bit>

namespace shapes {

// A value that is never the right one: floating-point fields hold integers below 2^20, so the successor modulo 2^20
// differs from the value whatever the hash gave.
constexpr float wrong(float right) { return float((u32(right) + 1u) & 0xFFFFFu); }

// Is the cell within `radius` of an edge of the grid?
template <typename S> constexpr bool on_rim(S const &s, std::size_t radius) {
    return s.id[0] < radius || s.id[1] < radius || s.id[0] + radius >= s.grid_range[0] || s.id[1] + radius >= s.grid_range[1];
}

// ------------------------------------------------------------------ read policies
// Sub-iteration 0 reads the centre and every neighbour with a column offset <= 0, sub-iteration 1 the centre and every
// neighbour with a column offset >= 0; rows are unrestricted.  Over a generation a cell's dependency cone grows by
// R columns per side, not by 2 R.  COPIED_FROM: fields from this index on are copied from the centre cell.
template <int COPIED_FROM = 8> struct OneWayReads {
    template <int D, int NS> static constexpr bool reads(int o, int, u32 subiteration) {
        static_assert(NS == 2);
        const int dc = o % D - D / 2;
        return subiteration == 0 ? dc <= 0 : dc >= 0;
    }
    static constexpr bool copied(int f) { return f >= COPIED_FROM; }
};
// both sides in both sub-iterations
struct AllReads {
    template <int D, int NS> static constexpr bool reads(int, int, u32) { return true; }
    static constexpr bool copied(int) { return false; }
};

struct Medium { // FDTD's combination in small: a field that evolves and one that is only carried along
    float value;
    u32 material;
    static constexpr auto fields = std::make_tuple(&Medium::value, &Medium::material);
};

// ------------------------------------------------------------------ the hooks
// interior() returns something else than operator(): after ONE launch the cells that differ from the cpu backend are
// the output rectangles of the units that ran the check-free code (run_canary below).
struct Canary : Hash<float, 1, 1> {
    using Base = Hash<float, 1, 1>;
    constexpr Canary(u32 seed) : Base{seed} {}
    Cell interior(stencil::Stencil<float, 1, std::monostate> const &s) const { return wrong(Base::operator()(s)); }
};

// interior() is right exactly where the sweep may call it: for cells that are not on the rim of the grid
struct Rim : Hash<float, 1, 1> {
    using Base = Hash<float, 1, 1>;
    constexpr Rim(u32 seed) : Base{seed} {}
    Cell interior(stencil::Stencil<float, 1, std::monostate> const &s) const {
        const float right = Base::operator()(s);
        return on_rim(s, 1) ? wrong(right) : right;
    }
};

// at_level<level, levels>() is right exactly when the sweep names the level it is computing: the level's sub-iteration
// is the stencil's, the level lies inside the launch, and the launch is whole generations
struct Levels : Hash<float, 1, 2> {
    using Base = Hash<float, 1, 2>;
    constexpr Levels(u32 seed) : Base{seed} {}
    template <int level, int levels> Cell at_level(stencil::Stencil<float, 1, std::monostate> const &s) const {
        const float right = Base::operator()(s);
        const bool named = std::size_t(level % 2) == s.subiteration && level < levels && levels % 2 == 0 && level >= 0;
        return named ? right : wrong(right);
    }
};

struct ColumnHint {
    static constexpr std::size_t halo_columns_per_generation = 1;
};
struct NoHint {};

// one-way reads, with and without the hint they allow (the twin without is never swept: its strip width is what the
// hint is measured against)
template <typename Hint> struct OneWayOf : Hash<float, 1, 2, std::monostate, OneWayReads<>>, Hint {
    using Base = Hash<float, 1, 2, std::monostate, OneWayReads<>>;
    constexpr OneWayOf(u32 seed) : Base{seed} {}
};
using OneWay = OneWayOf<ColumnHint>;

// the same on two planes, the second one declared constant: from the third pass of a call on its stores are left out
template <typename Hint> struct OneWayPlanesOf : Hash<Medium, 1, 2, std::monostate, OneWayReads<1>>, Hint {
    using Base = Hash<Medium, 1, 2, std::monostate, OneWayReads<1>>;
    static constexpr auto constant_fields = std::make_tuple(&Medium::material);
    constexpr OneWayPlanesOf(u32 seed) : Base{seed} {}
};
using OneWayPlanes = OneWayPlanesOf<ColumnHint>;

// the hint against the check-free promise: one cell per lane, so the column halo is exactly the hint's and the cells
// that reach the output come within one column of the footprint's edge -- up to its last column in the first
// sub-iteration, which reads west only: a check-free footprint that ended at the grid's east edge handed interior() the
// grid's last column (Sweep::hinted_interior keeps such units a column away since)
template <typename Hint> struct OneWayRimOf : Hash<float, 1, 2, std::monostate, OneWayReads<>>, Hint {
    using Base = Hash<float, 1, 2, std::monostate, OneWayReads<>>;
    constexpr OneWayRimOf(u32 seed) : Base{seed} {}
    Cell interior(stencil::Stencil<float, 1, std::monostate> const &s) const {
        const float right = Base::operator()(s);
        return on_rim(s, 1) ? wrong(right) : right;
    }
};
using OneWayRim = OneWayRimOf<ColumnHint>;

// declares the hint and reads both sides all the same: wherever a strip seam lies inside the grid the result is wrong
struct Liar : Hash<float, 1, 2, std::monostate, AllReads>, ColumnHint {
    using Base = Hash<float, 1, 2, std::monostate, AllReads>;
    constexpr Liar(u32 seed) : Base{seed} {}
};

// ------------------------------------------------------------------ explicit tunings
struct Lone8 : Hash<float, 1, 1> { // no `stages`: independent waves at depths 8, 4, 2, 1
    constexpr Lone8(u32 seed) : Hash<float, 1, 1>{seed} {}
};
struct Twelve : Hash<float, 1, 1> { // depth 12 on four stages, 6 and 3 on three, 1 on one
    constexpr Twelve(u32 seed) : Hash<float, 1, 1>{seed} {}
};
struct Batch8 : Hash<float, 1, 1> { // batches of eight rows, every toggle the rule would set false
    constexpr Batch8(u32 seed) : Hash<float, 1, 1>{seed} {}
};
struct FatOn : Hash<Octo, 1, 1> { // a fat cell with every toggle the rule would leave off
    constexpr FatOn(u32 seed) : Hash<Octo, 1, 1>{seed} {}
};

// ------------------------------------------------------------------ the function object's own state
// The state is folded into the seed of the hash (every byte under a multiplier of its own, so a lost or misplaced byte
// changes cells), the table by an index taken from the centre cell at run time.
template <u32 SEED> struct NoState {
    constexpr NoState(u32) {}
    constexpr u32 fold(u32) const { return SEED; }
};
struct Bytes7 {
    std::uint8_t b[7];
    constexpr Bytes7(u32 seed) : b{} {
        for (u32 i = 0; i < 7; i++)
            b[i] = std::uint8_t(finalize(seed + i * odd(810u)) >> 24);
    }
    constexpr u32 fold(u32) const {
        u32 h = 0;
        for (u32 i = 0; i < 7; i++)
            h += u32(b[i]) * odd(820u + i);
        return h;
    }
};
struct DoubleAndWords {
    double d;
    u32 a, b;
    constexpr DoubleAndWords(u32 seed)
        : d(double(finalize(seed)) * 4294967296.0 + double(finalize(seed + 1u))), a(finalize(seed + 2u)), b(finalize(seed + 3u)) {}
    constexpr u32 fold(u32) const {
        const std::uint64_t bits = std::bit_cast<std::uint64_t>(d);
        return u32(bits) * odd(830u) + u32(bits >> 32) * odd(831u) + a * odd(832u) + b * odd(833u);
    }
};
template <int N, bool INDEXED = false> struct Words {
    u32 w[N];
    constexpr Words(u32 seed) : w{} {
        for (u32 i = 0; i < u32(N); i++)
            w[i] = finalize(seed + i * odd(811u));
    }
    constexpr u32 fold(u32 centre) const {
        if constexpr (INDEXED) {
            return w[centre & u32(N - 1)];
        } else {
            u32 h = 0;
            for (u32 i = 0; i < u32(N); i++)
                h += w[i] * odd(840u + i);
            return h;
        }
    }
};
static_assert(sizeof(Bytes7) == 7 && sizeof(DoubleAndWords) == 16 && alignof(DoubleAndWords) == 8 && sizeof(Words<9>) == 36 &&
              sizeof(Words<10>) == 40 && sizeof(Words<16, true>) == 64);

template <typename State> struct Stateful : State {
    using Cell = float;
    using TimeDependentValue = std::monostate;
    static constexpr std::size_t stencil_radius = 1;
    static constexpr std::size_t n_subiterations = 1;

    constexpr Stateful(u32 seed) : State(seed) {}
    std::monostate get_time_dependent_value(std::size_t) const { return {}; }

    template <typename Neighbour> float evaluate(Context const &c, Neighbour &&at) const {
        return Hash<float, 1, 1>{this->fold(to_word(at(0, 0)))}.evaluate(c, at);
    }
    float operator()(stencil::Stencil<float, 1, std::monostate> const &s) const {
        return Hash<float, 1, 1>{this->fold(to_word(s[0][0]))}(s);
    }
};
using Stateless = Stateful<NoState<0x5005u>>;
using State7 = Stateful<Bytes7>;
using State16 = Stateful<DoubleAndWords>;
using State36 = Stateful<Words<9>>;
using State40 = Stateful<Words<10>>;
using StateTable = Stateful<Words<16, true>>;
static_assert(std::is_empty_v<Stateless> && sizeof(State7) == 7 && sizeof(State16) == 16 && sizeof(State36) == 36 &&
              sizeof(State40) == 40 && sizeof(StateTable) == 64);

} // namespace shapes

#ifdef __HIPCC__
// ====================================================================== the HIP side
namespace shapes {

// the members of an explicit tuning (`stages` apart: a tuning without it is a case)
template <int K, int T, int P> struct ShapeWithoutStages {
    static constexpr int cells_per_lane = K;
    static constexpr int max_generations = T;
    static constexpr int prefetch_rows = P;
    static constexpr bool interior_variant = true;
    static constexpr int min_waves_per_simd = 1;
    static constexpr bool narrow_form = false;
};
template <int K, int T, int P, int STAGES> struct Shape : ShapeWithoutStages<K, T, P> {
    static constexpr int stages = STAGES;
};

} // namespace shapes

namespace stencil::hip {
// four cells per lane, four generations on four stages
template <bool SOA> struct SweepTuning<shapes::Canary, SOA> : shapes::Shape<4, 4, 4, 4> {};
template <bool SOA> struct SweepTuning<shapes::Rim, SOA> : shapes::Shape<4, 4, 4, 4> {};
template <bool SOA> struct SweepTuning<shapes::Levels, SOA> : shapes::Shape<4, 4, 4, 4> {}; // two levels per stage
template <typename Hint, bool SOA> struct SweepTuning<shapes::OneWayOf<Hint>, SOA> : shapes::Shape<4, 4, 4, 4> {};
template <typename Hint, bool SOA> struct SweepTuning<shapes::OneWayPlanesOf<Hint>, SOA> : shapes::Shape<2, 4, 4, 4> {};
template <typename Hint, bool SOA> struct SweepTuning<shapes::OneWayRimOf<Hint>, SOA> : shapes::Shape<1, 4, 4, 4> {};
template <bool SOA> struct SweepTuning<shapes::Liar, SOA> : shapes::Shape<1, 2, 4, 4> {};
template <typename State, bool SOA> struct SweepTuning<shapes::Stateful<State>, SOA> : shapes::Shape<4, 4, 4, 4> {};

template <bool SOA> struct SweepTuning<shapes::Lone8, SOA> : shapes::ShapeWithoutStages<4, 8, 4> {};
template <bool SOA> struct SweepTuning<shapes::Twelve, SOA> : shapes::Shape<2, 12, 4, 4> {};
template <bool SOA> struct SweepTuning<shapes::Batch8, SOA> : shapes::Shape<4, 8, 8, 4> {
    static constexpr bool interior_variant = false;
    static constexpr bool pinned_loads = false, pinned_stores = false, scalar_function = false, trapezoid_fill = false,
                          streaming_stores = false;
};
template <bool SOA> struct SweepTuning<shapes::FatOn, SOA> : shapes::Shape<1, 4, 4, 4> {
    static constexpr bool trapezoid_fill = true, pinned_loads = true, pinned_stores = true, streaming_stores = true;
};
} // namespace stencil::hip

namespace shapes {

template <typename F, bool SOA, int T = SweepTuning<F, SOA>::max_generations> constexpr int levels_per_stage() {
    return hi::SweepOf<F, SOA, T>::L;
}
template <typename F, bool SOA, int T = SweepTuning<F, SOA>::max_generations> constexpr int waves_per_strip() {
    return hi::SweepOf<F, SOA, T>::W;
}

//                       F      planes  K  T  P  stages narrow
static_assert(has_shape<Canary, false, 4, 4, 4, 4, false>() && hi::SweepOf<Canary, false>::OW == 248);
static_assert(has_shape<Rim, false, 4, 4, 4, 4, false>() && hi::SweepOf<Rim, false>::OW == 248);
static_assert(has_shape<Levels, false, 4, 4, 4, 4, false>() && hi::SweepOf<Levels, false>::OW == 240 &&
              levels_per_stage<Levels, false>() == 2);
// the hint widens the strips: a column halo of T instead of 2 T, rounded to whole lanes
static_assert(has_shape<OneWay, false, 4, 4, 4, 4, false>() && hi::SweepOf<OneWay, false>::OW == 248 &&
              hi::SweepOf<OneWayOf<NoHint>, false>::OW == 240);
static_assert(has_shape<OneWayPlanes, true, 2, 4, 4, 4, false>() && on_planes<OneWayPlanes, true>() &&
              hi::SweepOf<OneWayPlanes, true>::OW == 120 && hi::SweepOf<OneWayPlanesOf<NoHint>, true>::OW == 112 &&
              hi::constant_plane_mask<OneWayPlanes>() == 2u);
static_assert(has_shape<OneWayRim, false, 1, 4, 4, 4, false>() && hi::SweepOf<OneWayRim, false>::OW == 56 &&
              hi::SweepOf<OneWayRim, false>::GX == 4 && hi::SweepOf<OneWayRimOf<NoHint>, false>::OW == 48);
// ... and the liar's are two columns short of what it reads on either side
static_assert(has_shape<Liar, false, 1, 2, 4, 4, false>() && hi::SweepOf<Liar, false>::OW == 60 &&
              hi::SweepOf<Liar, false>::GX == 2 && hi::SweepOf<Liar, false>::G == 4);

// no `stages` member: independent waves at every depth, four units per workgroup
template <typename Tuning> constexpr bool names_stages = requires { Tuning::stages; };
static_assert(!names_stages<SweepTuning<Lone8, false>> && names_stages<SweepTuning<Twelve, false>> && SweepTuning<Lone8, false>::max_generations == 8 &&
              SweepTuning<Lone8, false>::cells_per_lane == 4 && !hi::has_narrow_form<Lone8, false>() &&
              waves_per_strip<Lone8, false>() == 1 && hi::SweepOf<Lone8, false>::units_per_block == 4 &&
              hi::SweepOf<Lone8, false>::OW == 240);
// 12 levels on four stages, 6 and 3 on three, 1 on one
static_assert(has_shape<Twelve, false, 2, 12, 4, 4, false>() && hi::SweepOf<Twelve, false>::OW == 104 &&
              waves_per_strip<Twelve, false, 12>() == 4 && waves_per_strip<Twelve, false, 6>() == 3 &&
              waves_per_strip<Twelve, false, 3>() == 3 && waves_per_strip<Twelve, false, 1>() == 1);
static_assert(has_shape<Batch8, false, 4, 8, 8, 4, false>() && hi::SweepOf<Batch8, false>::LDS_WORDS * 4 == 48 * 1024 &&
              !hi::pinned_loads_for<Batch8, false>() && !hi::pinned_stores_for<Batch8, false>() &&
              !hi::scalar_function_for<Batch8, false>() && !hi::trapezoid_fill_for<Batch8, false>() &&
              !hi::streaming_stores_for<Batch8, false>() && !SweepTuning<Batch8, false>::interior_variant);
// (the rule: a 32-byte cell gets none of the four)
static_assert(has_shape<FatOn, false, 1, 4, 4, 4, false>() && hi::SweepOf<FatOn, false>::LDS_WORDS * 4 == 48 * 1024 &&
              hi::trapezoid_fill_for<FatOn, false>() && hi::pinned_loads_for<FatOn, false>() &&
              hi::pinned_stores_for<FatOn, false>() && hi::streaming_stores_for<FatOn, false>() &&
              !hi::trapezoid_fill_for<Octo1, false>() && !hi::pinned_loads_for<Octo1, false>() &&
              !hi::pinned_stores_for<Octo1, false>() && !hi::streaming_stores_for<Octo1, false>());

// which state travels in scalar registers (staged sweeps: all of these are)
static_assert(has_shape<State36, false, 4, 4, 4, 4, false>() && waves_per_strip<State36, false>() == 4);
static_assert(!hi::scalar_function_for<Stateless, false>() && !hi::scalar_function_for<State7, false>() &&
              hi::scalar_function_for<State16, false>() && hi::scalar_function_for<State36, false>() &&
              !hi::scalar_function_for<State40, false>() && !hi::scalar_function_for<StateTable, false>());

// ------------------------------------------------------------------ the canary's driver
// ONE launch of Canary's compiled depth `n` on an h x w grid: the cells that differ from the cpu backend must be exactly
// the output rectangles of the units Sweep::entry() gives the check-free code -- restated here for row chunks of eight
// rows and one tier (the chunks-of-8-rows environment: pick_chunk_rows returns 8, and a quarter of that is below the
// taper's four rows), whole rows, no column range.  Returns the number of check-free units.
template <int N, typename Functor> std::size_t run_canary_grid(Case<Functor, false> &c, std::size_t h, std::size_t w) {
    using SW = hi::SweepOf<Functor, false, N>;
    constexpr int chunk = 8;
    auto grids = c.make_grids(h, w);
    c.update.get_params().n_iterations = c.reference.get_params().n_iterations = std::size_t(N);
    c.update.get_params().iteration_offset = c.reference.get_params().iteration_offset = 0;
    stencil::hip::Grid<float> out = c.update(grids.device);
    stencil::cpu::Grid<float> want = c.reference(grids.host);

    std::vector<char> expected(h * w, 0);
    std::size_t units = 0;
    const int n_strips = (int(w) + SW::OW - 1) / SW::OW, n_chunks = (int(h) + chunk - 1) / chunk;
    for (int strip = 0; strip < n_strips; strip++)
        for (int k = 0; k < n_chunks; k++) {
            const int ya = k * chunk, yb = std::min(ya + chunk, int(h));
            const int xw0 = strip * SW::OW - SW::GX;
            const bool check_free = xw0 > 0 && xw0 + SW::LW <= int(w) && ya - SW::G >= 0 && yb + SW::G <= int(h);
            if (!check_free)
                continue;
            units++;
            for (int r = ya; r < yb; r++)
                for (int x = strip * SW::OW; x < (strip + 1) * SW::OW; x++)
                    expected[std::size_t(r) * w + std::size_t(x)] = 1;
        }
    std::size_t differing = 0, unexpected = 0, first_row = 0, first_column = 0;
    {
        typename stencil::hip::Grid<float>::template GridAccessor<sycl::access::mode::read> ac(out);
        typename stencil::cpu::Grid<float>::template GridAccessor<sycl::access::mode::read> wc(want);
        for (std::size_t r = 0; r < h; r++)
            for (std::size_t x = 0; x < w; x++) {
                const bool differs = !(ac[r][x] == wc[r][x]);
                differing += differs ? 1 : 0;
                if (differs != bool(expected[r * w + x]) && unexpected++ == 0)
                    first_row = r, first_column = x;
            }
    }
    if (unexpected != 0)
        std::fprintf(stderr,
                     "MISMATCH canary: %zu x %zu, depth %d: %zu cells are not where the check-free units are, first at "
                     "(row %zu, column %zu)\n", h, w, N, unexpected, first_row, first_column);
    REQUIRE(unexpected == 0);
    REQUIRE(differing == units * std::size_t(chunk) * std::size_t(SW::OW));
    return units;
}

// The six extents of Case::run's check-free grids, every width at every height, at the compiled depth T; and at depth 1
// (independent waves, a warm-up of one row) the predicted set alone.  Needs row chunks of eight rows; says so and
// checks nothing otherwise.
// (a template, like run_liar: the units that do not call it instantiate none of its kernels)
template <typename Functor = Canary> void run_canary(u32 seed) {
    using C = Case<Functor, false>;
    if (hi::options().chunk_rows != 8 || hi::options().n_taper > 0 || hi::options().xcd_remap) {
        std::printf("canary: not run (row chunks of eight rows only)\n");
        return;
    }
    C c("Canary", seed);
    REQUIRE(int(C::Update::sweep_description().max_generations) == C::T);
    static_assert(std::is_same_v<Functor, Canary>);
    const std::size_t a = std::size_t((C::G + 7) / 8 * 8);
    const std::size_t widths[3] = {std::size_t(2 * C::OW + C::GX - 1), std::size_t(2 * C::OW + C::GX), std::size_t(3 * C::OW + C::GX + 1)};
    const std::size_t heights[3] = {a + 8 + C::G - 1, a + 8 + C::G, 4 * std::size_t(C::G) + 7};
    std::printf("canary: depth %d, units", C::T);
    for (std::size_t h : heights)
        for (std::size_t w : widths) {
            const std::size_t units = run_canary_grid<C::T>(c, h, w);
            // strip 1 just misses at the first width, no chunk qualifies at the first height
            REQUIRE((units == 0) == (w == widths[0] || h == heights[0]));
            std::printf(" %zux%zu:%zu", h, w, units);
            (void)run_canary_grid<1>(c, h, w);
        }
    std::printf("\n");
    std::fflush(stdout);
}

// The liar's result differs from the cpu backend where a strip seam lies inside the grid, and only there.
template <typename Functor = Liar> void run_liar(u32 seed) {
    using C = Case<Functor, false>;
    C c("Liar", seed);
    std::size_t differing[2];
    const std::size_t widths[2] = {std::size_t(C::OW), std::size_t(2 * C::OW + 3)};
    for (int i = 0; i < 2; i++) {
        const std::size_t h = std::size_t(C::G) + 1, w = widths[i];
        auto grids = c.make_grids(h, w);
        c.update.get_params().n_iterations = c.reference.get_params().n_iterations = std::size_t(C::T);
        stencil::hip::Grid<float> out = c.update(grids.device);
        stencil::cpu::Grid<float> want = c.reference(grids.host);
        typename stencil::hip::Grid<float>::template GridAccessor<sycl::access::mode::read> ac(out);
        typename stencil::cpu::Grid<float>::template GridAccessor<sycl::access::mode::read> wc(want);
        differing[i] = compare_fields<float>(
                           h, w, [&](std::size_t r, std::size_t x) { return ac[r][x]; },
                           [&](std::size_t r, std::size_t x) { return wc[r][x]; })
                           .count;
    }
    REQUIRE(differing[0] == 0);
    REQUIRE(differing[1] != 0);
    std::printf("liar: K=%d T=%d OW=%d depth=%u, cells that differ at width %zu: %zu, at width %zu: %zu\n", C::K, C::T, C::OW,
                unsigned(C::Update::sweep_description().max_generations), widths[0], differing[0], widths[1], differing[1]);
    std::fflush(stdout);
}

} // namespace shapes
#endif // __HIPCC__

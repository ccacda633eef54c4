// User functors of every pipeline shape SweepTuning's rule produces (hip/internal/Sweep.hpp), swept by
// stencil::hip::StencilUpdate and compared with stencil::cpu::StencilUpdate field by field.
//
// The functors are position-sensitive hashes: every output field is a wrap-around 32-bit hash of the cells of the
// (2R+1)^2 neighbourhood (a distinct odd multiplier per offset and field), of the cell's coordinates, the grid's extent,
// the generation, the sub-iteration and the time-dependent value.  A neighbour taken from the wrong lane, row, level or
// generation changes the cell.  Floating-point fields hold integers below 2^20, converted exactly both ways, so no result
// depends on rounding or on the order of operations; nothing calls libm.
//
// The file is included by the HIP binaries shape_test_a ... shape_test_d (the cells, the functors, the static asserts
// on their shapes and the driver), through hook_cases.hpp by shape_test_e ... shape_test_j (functors with the hooks,
// hints, tunings and states a transition function may add) and by the host-only shape_host_test (the cells and the
// functors alone, checked against a plain double loop).
#pragma once
#include "mini_test.hpp"
#include <StencilStream/Stencil.hpp>
#include <StencilStream/cpu/StencilUpdate.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <tuple>
#include <type_traits>
#include <variant>
#include <vector>

namespace shapes {

using u32 = std::uint32_t;

// ------------------------------------------------------------------ cells
struct Tri { // three floats: three-word LDS packets, AoS and on planes
    float a, b, c;
    static constexpr auto fields = std::make_tuple(&Tri::a, &Tri::b, &Tri::c);
};
struct Quad { // 16 bytes, four fields: a request for planes is swept as AoS (hip::SplitCellPolicy)
    float a, b;
    u32 c, d;
    static constexpr auto fields = std::make_tuple(&Quad::a, &Quad::b, &Quad::c, &Quad::d);
};
struct Octo { // 32 bytes: the row rings of four stages are exactly 48 KiB
    u32 a, b;
    float c, d;
    u32 e;
    float f;
    u32 g, h;
    static constexpr auto fields =
        std::make_tuple(&Octo::a, &Octo::b, &Octo::c, &Octo::d, &Octo::e, &Octo::f, &Octo::g, &Octo::h);
};
struct Penta { // five doubles: deeper than its window allows only through stages
    double a, b, c, d, e;
    static constexpr auto fields = std::make_tuple(&Penta::a, &Penta::b, &Penta::c, &Penta::d, &Penta::e);
};
struct Mixed { // plane elements of 1, 2 and 8 bytes; five padding bytes that scatter / gather never move
    std::uint8_t a;
    std::uint16_t b;
    double c;
    static constexpr auto fields = std::make_tuple(&Mixed::a, &Mixed::b, &Mixed::c);
};
static_assert(sizeof(Tri) == 12 && sizeof(Quad) == 16 && sizeof(Octo) == 32 && sizeof(Penta) == 40 && sizeof(Mixed) == 16);

// a time-dependent value that is a struct, not a scalar
struct Drive {
    u32 phase;
    float level;
};

// ------------------------------------------------------------------ fields as 32-bit words
template <typename Cell> constexpr int n_fields() {
    if constexpr (requires { Cell::fields; })
        return int(std::tuple_size_v<std::remove_cvref_t<decltype(Cell::fields)>>);
    else
        return 1;
}
template <int I, typename Cell> constexpr auto const &field(Cell const &cell) {
    if constexpr (requires { Cell::fields; }) {
        constexpr auto member = std::get<I>(Cell::fields);
        return cell.*member;
    } else {
        return cell;
    }
}
template <int I, typename Cell> constexpr auto &field(Cell &cell) {
    if constexpr (requires { Cell::fields; }) {
        constexpr auto member = std::get<I>(Cell::fields);
        return cell.*member;
    } else {
        return cell;
    }
}
// exact: integer fields as they are, floating-point fields hold integers below 2^20
template <typename T> constexpr u32 to_word(T value) { return u32(value); }
template <typename T> constexpr T from_hash(u32 hash) {
    if constexpr (std::is_floating_point_v<T>)
        return T(hash & 0xFFFFFu);
    else
        return T(hash >> (32 - 8 * int(sizeof(T)))); // the top bits: the best mixed ones
}
constexpr u32 golden = 0x9E3779B1u;
// the i-th odd multiplier: distinct for distinct i (multiplying by an odd number is a bijection modulo 2^32)
constexpr u32 odd(u32 i) { return golden * (2u * i + 1u); }
constexpr u32 finalize(u32 h) {
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    h *= 0x297A2D39u;
    h ^= h >> 15;
    return h;
}
// every field of a cell from one hash
template <typename Cell> constexpr Cell cell_from(u32 hash) {
    Cell cell{};
    stencil::internal::static_for<0, n_fields<Cell>()>([&](auto f) {
        using T = std::remove_cvref_t<decltype(field<f>(cell))>;
        field<f>(cell) = from_hash<T>(finalize(hash * odd(900u + u32(f)) + u32(f)));
    });
    return cell;
}
template <typename Cell> constexpr Cell initial_cell(u32 row, u32 column, u32 seed) {
    return cell_from<Cell>(seed + row * odd(800u) + column * odd(801u));
}
template <typename Cell> constexpr Cell halo_cell(u32 seed) { return cell_from<Cell>(seed * odd(802u) + 0xABCD1234u); }

constexpr u32 tdv_word(std::monostate) { return 0u; }
constexpr u32 tdv_word(Drive const &drive) { return drive.phase * odd(803u) + to_word(drive.level) * odd(804u); }

// What a cell update sees besides its neighbourhood.
struct Context {
    u32 row, column, height, width, iteration, subiteration, tdv;
};

// ------------------------------------------------------------------ what a sub-iteration reads
// Field f of the neighbour at offset o (row-major in the D x D neighbourhood) is read in sub-iteration (o + f) mod NS --
// every sub-iteration reads other fields and other neighbours, a generation reads them all; the centre cell is read
// whole every time.  No field is merely copied.
struct RotatingReads {
    template <int D, int NS> static constexpr bool reads(int o, int f, u32 subiteration) {
        return NS == 1 || o == (D * D) / 2 || u32(o + f) % u32(NS) == subiteration;
    }
    static constexpr bool copied(int) { return false; }
};

// ------------------------------------------------------------------ the functor
template <typename CellT, std::size_t R, std::size_t NS, typename TDVT = std::monostate, typename Reads = RotatingReads>
struct Hash {
    using Cell = CellT;
    using TimeDependentValue = TDVT;
    static constexpr std::size_t stencil_radius = R;
    static constexpr std::size_t n_subiterations = NS;
    static constexpr int D = 2 * int(R) + 1;
    static constexpr int NF = n_fields<CellT>();
    // multiplier o * 8 + f of a neighbour's field stays below the 700s of the context
    static_assert(NF <= 8 && D * D * 8 < 700);

    u32 seed;

    TDVT get_time_dependent_value(std::size_t i) const {
        if constexpr (std::is_same_v<TDVT, Drive>)
            return Drive{u32(i) * 2654435761u ^ seed, float((u32(i) * 7u + 3u) % 1000u)};
        else
            return TDVT{};
    }

    // what a sub-iteration reads is a policy (RotatingReads above; hook_cases.hpp has one-way ones)
    static constexpr bool reads(int o, int f, u32 subiteration) { return Reads::template reads<D, int(NS)>(o, f, subiteration); }

    // `at(dr, dc)`: the neighbour dr rows south and dc columns east of the cell
    template <typename Neighbour> Cell evaluate(Context const &c, Neighbour &&at) const {
        u32 hash = seed + c.row * odd(701u) + c.column * odd(702u) + c.height * odd(703u) +
                   c.width * odd(704u) + c.iteration * odd(705u) + c.subiteration * odd(706u) + c.tdv * odd(707u);
        stencil::internal::static_for<0, D * D>([&](auto o) {
            CellT const neighbour = at(int(o) / D - int(R), int(o) % D - int(R));
            stencil::internal::static_for<0, NF>([&](auto f) {
                if (reads(o, f, c.subiteration))
                    hash += to_word(field<f>(neighbour)) * odd(u32(o) * 8u + u32(f));
            });
        });
        CellT result = cell_from<CellT>(finalize(hash));
        // fields the policy says are only copied keep the centre cell's value
        stencil::internal::static_for<0, NF>([&](auto f) {
            if constexpr (Reads::copied(int(f)))
                field<f>(result) = field<f>(at(0, 0));
        });
        return result;
    }

    Cell operator()(stencil::Stencil<CellT, R, TDVT> const &s) const {
        const Context c{u32(s.id[0]),     u32(s.id[1]),        u32(s.grid_range[0]),           u32(s.grid_range[1]),
                        u32(s.iteration), u32(s.subiteration), tdv_word(s.time_dependent_value)};
        return evaluate(c, [&](int dr, int dc) { return s[dr][dc]; });
    }
};

// ------------------------------------------------------------------ the cases: one per shape
using U16 = Hash<std::uint16_t, 1, 1>;          // sub-word cell; compiled 16 deep, 8 by default
using F3 = Hash<float, 1, 3, Drive>;            // the relaxed depth 6 with its halvings 3 and 1; a struct as TDV
using D1 = Hash<double, 1, 1>;                  // one 8-byte field: two cells per lane, twelve generations
using Tri1 = Hash<Tri, 1, 1>;                   // three-word packets, AoS and on planes
using Quad1 = Hash<Quad, 1, 1>;                 // 16 bytes in four fields: swept as AoS whatever is asked
using Octo1 = Hash<Octo, 1, 1>;                 // rings exactly at the LDS limit
using Penta1 = Hash<Penta, 1, 1>;               // deeper through stages only
using Mixed2 = Hash<Mixed, 1, 2>;               // planes of 1, 2 and 8 bytes, two sub-iterations
using F2x2 = Hash<float, 2, 2>;                 // radius 2, two sub-iterations
using F3x1 = Hash<float, 3, 1>;                 // radius 3: 7 x 7 neighbourhood, K != R, P = 6
using D2x1 = Hash<double, 2, 1>;                // radius 2 on two cells per lane

// ------------------------------------------------------------------ comparing two grids field by field
struct Difference {
    std::size_t count = 0;
    std::size_t row = 0, column = 0;
    int field_index = 0;
    u32 got = 0, want = 0;
};
template <typename Cell, typename Got, typename Want>
Difference compare_fields(std::size_t height, std::size_t width, Got &&got, Want &&want) {
    Difference d;
    for (std::size_t r = 0; r < height; r++)
        for (std::size_t c = 0; c < width; c++) {
            Cell const x = got(r, c), y = want(r, c);
            bool differs = false;
            stencil::internal::static_for<0, n_fields<Cell>()>([&](auto f) {
                if (!(field<f>(x) == field<f>(y))) {
                    if (d.count == 0 && !differs) {
                        d.row = r, d.column = c, d.field_index = int(f);
                        d.got = to_word(field<f>(x)), d.want = to_word(field<f>(y));
                    }
                    differs = true;
                }
            });
            d.count += differs ? 1 : 0;
        }
    return d;
}

inline std::vector<std::size_t> unique_sorted(std::vector<std::size_t> values) {
    std::sort(values.begin(), values.end());
    values.erase(std::unique(values.begin(), values.end()), values.end());
    return values;
}

} // namespace shapes

#ifdef __HIPCC__
// ====================================================================== the HIP side
#include <StencilStream/hip/StencilUpdate.hpp>

namespace shapes {
using stencil::hip::SweepTuning;
namespace hi = stencil::hip::internal;

template <typename F, bool SOA, int K, int T, int P, int STAGES, bool NARROW> constexpr bool has_shape() {
    using S = SweepTuning<F, SOA>;
    return S::cells_per_lane == K && S::max_generations == T && S::prefetch_rows == P && S::stages == STAGES &&
           hi::has_narrow_form<F, SOA>() == NARROW;
}
template <typename F, bool SPLIT> constexpr bool on_planes() {
    return stencil::hip::StencilUpdate<F, SPLIT>::sweeps_on_planes;
}

// The shape each case stands for (the table of the coverage contract).  A change of the rule
// that moves a case fails here: give the shape another case before touching the numbers.
//                       F      planes  K  T   P  stages narrow
static_assert(has_shape<U16, false, 4, 16, 4, 4, true>() && hi::default_generations_for<U16, false>() == 8 &&
              hi::SweepOf<U16, false>::OW == 224);
static_assert(has_shape<F3, false, 4, 6, 2, 2, true>() && hi::SweepOf<F3, false>::OW == 216);
static_assert(has_shape<D1, false, 2, 12, 4, 4, true>() && hi::SweepOf<D1, false>::OW == 104);
static_assert(has_shape<Tri1, false, 1, 8, 4, 4, false>() && hi::SweepOf<Tri1, false>::OW == 48);
static_assert(has_shape<Tri1, true, 1, 8, 4, 4, false>() && hi::SweepOf<Tri1, true>::OW == 48 && on_planes<Tri1, true>());
static_assert(has_shape<Quad1, false, 1, 8, 4, 4, false>() && !on_planes<Quad1, true>());
static_assert(has_shape<Octo1, false, 1, 8, 4, 4, false>() && hi::SweepOf<Octo1, false>::OW == 48 &&
              hi::SweepOf<Octo1, false>::LDS_WORDS * 4 == 48 * 1024);
static_assert(has_shape<Penta1, false, 1, 8, 2, 4, false>() && hi::SweepOf<Penta1, false>::OW == 48);
static_assert(has_shape<Mixed2, true, 1, 8, 4, 4, false>() && hi::SweepOf<Mixed2, true>::OW == 32 && on_planes<Mixed2, true>());
static_assert(has_shape<F2x2, false, 4, 6, 4, 4, true>() && hi::SweepOf<F2x2, false>::OW == 208);
static_assert(has_shape<F3x1, false, 4, 1, 6, 1, false>() && hi::SweepOf<F3x1, false>::OW == 248);
static_assert(has_shape<D2x1, false, 2, 2, 4, 2, false>() && hi::SweepOf<D2x1, false>::OW == 120);

// ------------------------------------------------------------------ the driver
// `Strategy`: where the launches' time-dependent values come from (tdv/SinglePassStrategies.hpp)
template <typename F, bool SPLIT, typename Strategy = stencil::tdv::single_pass::PrecomputeOnHostStrategy> struct Case {
    using Cell = typename F::Cell;
    using Update = stencil::hip::StencilUpdate<F, SPLIT, Strategy>;
    using Reference = stencil::cpu::StencilUpdate<F>;
    static constexpr bool planes = Update::sweeps_on_planes;
    using Tuning = SweepTuning<F, planes>;
    static constexpr int K = Tuning::cells_per_lane, T = Tuning::max_generations;
    static constexpr int G = int(F::stencil_radius) * int(F::n_subiterations) * T;
    static constexpr int OW = hi::SweepOf<F, planes>::OW;
    static constexpr int GX = (hi::wave_size * K - OW) / 2; // the column halo, rounded to whole lanes
    static constexpr bool narrow = hi::has_narrow_form<F, planes>();
    static constexpr int OWn = [] {
        if constexpr (narrow)
            return hi::SweepOf<hi::NarrowForm<F>, planes>::OW;
        else
            return 0;
    }();

    const char *name;
    u32 seed;
    Update update;
    Reference reference;

    Case(const char *name, u32 seed)
        : name(name), seed(seed),
          update({.transition_function = F{seed}, .halo_value = halo_cell<Cell>(seed), .blocking = true}),
          reference({.transition_function = F{seed}, .halo_value = halo_cell<Cell>(seed), .blocking = true}) {}

    struct Pair {
        stencil::hip::Grid<Cell> device;
        stencil::cpu::Grid<Cell> host;
    };
    Pair make_grids(std::size_t h, std::size_t w) const {
        Pair grids{stencil::hip::Grid<Cell>(h, w), stencil::cpu::Grid<Cell>(h, w)};
        typename stencil::hip::Grid<Cell>::template GridAccessor<sycl::access::mode::read_write> ac(grids.device);
        typename stencil::cpu::Grid<Cell>::template GridAccessor<sycl::access::mode::read_write> hc(grids.host);
        for (std::size_t r = 0; r < h; r++)
            for (std::size_t c = 0; c < w; c++)
                hc[r][c] = ac[r][c] = initial_cell<Cell>(u32(r), u32(c), seed);
        return grids;
    }

    // n generations from `offset` on both backends; the results replace the grids when `resume`
    void advance(Pair &grids, std::size_t n, std::size_t offset, bool resume, const char *what) {
        update.get_params().n_iterations = reference.get_params().n_iterations = n;
        update.get_params().iteration_offset = reference.get_params().iteration_offset = offset;
        stencil::hip::Grid<Cell> out = update(grids.device);
        stencil::cpu::Grid<Cell> want = reference(grids.host);
        const std::size_t h = grids.host.get_grid_height(), w = grids.host.get_grid_width();
        Difference d;
        {
            typename stencil::hip::Grid<Cell>::template GridAccessor<sycl::access::mode::read> ac(out);
            typename stencil::cpu::Grid<Cell>::template GridAccessor<sycl::access::mode::read> wc(want);
            d = compare_fields<Cell>(
                h, w, [&](std::size_t r, std::size_t c) { return ac[r][c]; },
                [&](std::size_t r, std::size_t c) { return wc[r][c]; });
        }
        if (d.count != 0)
            std::fprintf(stderr,
                         "MISMATCH %s%s: %zu x %zu, n = %zu, offset = %zu, depth %u: %zu cells differ, first at (row %zu, "
                         "column %zu, field %d): got %u, want %u\n",
                         name, what, h, w, n, offset, unsigned(Update::sweep_description().max_generations), d.count, d.row,
                         d.column, d.field_index, unsigned(d.got), unsigned(d.want));
        REQUIRE(d.count == 0);
        if (resume) {
            grids.device = out;
            grids.host = want;
        }
    }

    // `more_generations`: run lengths of a case's own besides the ones every case sweeps
    void run(std::vector<std::size_t> more_generations = {}) {
        // the smallest grids at which a strip seam, a ragged last lane, a one-row grid and a launch of several row
        // chunks can each go wrong, all derived from the shape
        std::vector<std::size_t> widths = {1, 2, K + 1, OW - 1, OW, OW + 1, 2 * OW + 3};
        if constexpr (narrow)
            widths.insert(widths.end(), {OWn - 1, OWn, OWn + 1});
        widths = unique_sorted(widths);
        const std::size_t heights[4] = {1, 3, G + 1, 4 * G + 7};
        // every compiled depth and the mixes (T = 1: no generation at all is a case as well)
        more_generations.insert(more_generations.end(), {1, 2, 3, T - 1, T, T + 1, 2 * T + 3});
        const std::vector<std::size_t> generations = unique_sorted(more_generations);
        for (std::size_t i = 0; i < widths.size(); i++)
            for (std::size_t h : {heights[i % 4], heights[(i + 2) % 4]}) { // every width and every height occurs
                Pair grids = make_grids(h, widths[i]);
                for (std::size_t n : generations)
                    advance(grids, n, 0, false, "");
            }
        // Grids on which units of the wave grid run the check-free code (Sweep::entry(): a unit whose whole footprint
        // lies inside the grid).  The widest grid above, 2 OW + 3, is narrower than the first one where strip 1 has its
        // footprint inside, 2 OW + GX: its columns are [OW - GX, 2 OW + GX) and GX is 4 at the least.  So, per form: the
        // width at which strip 1 just misses, the one at which it just fits, and two check-free strips with a ragged
        // third; with the chunks of eight rows of the chunks-of-8-rows environment and a = ceil(G / 8) * 8, the chunk
        // [a, a + 8) is the first whose warm-up rows lie inside the grid, and it needs a + 8 + G rows: one row less
        // (no chunk qualifies), exactly that (one does), and 4 G + 7.  Every width meets the height at which one chunk
        // qualifies; the width that just fits meets the height that just misses, the two others 4 G + 7.
        auto check_free_widths = [](int ow, int gx) {
            return std::vector<std::size_t>{std::size_t(2 * ow + gx - 1), std::size_t(2 * ow + gx), std::size_t(3 * ow + gx + 1)};
        };
        std::vector<std::size_t> wide = check_free_widths(OW, GX);
        if constexpr (narrow) {
            const std::vector<std::size_t> more = check_free_widths(OWn, (hi::wave_size * hi::ceil_pow2(int(F::stencil_radius)) - OWn) / 2);
            wide.insert(wide.end(), more.begin(), more.end());
        }
        const std::size_t a = std::size_t((G + 7) / 8 * 8);
        const std::size_t tall[3] = {a + 8 + G - 1, a + 8 + G, 4 * std::size_t(G) + 7};
        for (std::size_t i = 0; i < wide.size(); i++)
            for (std::size_t h : {tall[1], i % 3 == 1 ? tall[0] : tall[2]}) {
                Pair grids = make_grids(h, wide[i]);
                for (std::size_t n : generations)
                    advance(grids, n, 0, false, " (check-free)");
            }
        {
            Pair grids = make_grids(G + 1, OW + 1);
            advance(grids, T + 1, 5, false, " (offset)");
        }
        {
            // a second call resumes where the first one stopped, through get_params()
            Pair grids = make_grids(4 * G + 7, OW + 1);
            advance(grids, T + 1, 0, true, " (first call)");
            advance(grids, 3, T + 1, true, " (resumed)");
        }
        std::printf("shape %s: K=%d T=%d P=%d stages=%d narrow=%d planes=%d OW=%d depth=%u\n", name, K, T,
                    Tuning::prefetch_rows, hi::stages_for<F, planes>(), int(narrow), int(planes), OW,
                    unsigned(Update::sweep_description().max_generations));
        std::fflush(stdout);
    }
};

template <typename F, bool SPLIT = false, typename Strategy = stencil::tdv::single_pass::PrecomputeOnHostStrategy>
void run_case(const char *name, u32 seed, std::vector<std::size_t> more_generations = {}) {
    Case<F, SPLIT, Strategy> c(name, seed);
    c.run(more_generations);
}

} // namespace shapes
#endif // __HIPCC__

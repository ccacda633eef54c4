// The functors of shape_cases.hpp through the drivers that cut a grid over several GPUs: stencil::hip::StripUpdate on
// 1, 2 and 3 ranks and stencil::hip::BlockUpdate on meshes 1 x 1 ... 3 x 3, the ranks as threads of this process
// (tests/cpp/mesh_harness.hpp), the owned cells assembled and compared field by field with stencil::cpu::StencilUpdate
// on the whole grid.  The second mode ("mesh", "substrips") of shape_test_a ... shape_test_d: StripUpdate<F> and
// BlockUpdate<F> launch through StencilUpdate<F>::launch_entry(), so they instantiate no kernel those binaries do not
// hold already.
//
// Every extent is derived from the sweep's description, as the drivers derive their ghost depth from it:
//     D   = alt_generations if non-zero and below max_generations, else max_generations
//     hpg = halo_depth_per_generation,   g = D * hpg,   m = launches per ghost exchange,   ghost = g * m
// Per axis that is cut over n ranks (an axis that is not takes the shape test's small extent, OW + 1 columns or
// G + 1 rows), by the value of STSTHIP_EXCHANGE_EVERY the process was started with:
//     1      "limit":  n * 2 * g -- every rank owns exactly two ghost depths: a middle strip is two bands and no
//                      interior, a block's left and right packed columns are adjacent
//            "ragged": E = max(2 * g, OW) + 1, n * E + (n - 1) -- the earlier ranks own one more than the last, the
//                      sweep's column-strip seams fall inside the blocks, packed ghost columns of 1- and 2-byte planes
//                      are no multiple of four bytes wide
//     unset  the rule's m (4 for strips, 2 for blocks): n * 4 * g * m, and ragged with E = max(4 * g * m, OW) + 1 --
//            thick enough that the rule keeps its m
//     2      n * 8 * g keeps m = 2; n * (8 * g - 1) must fall to m = 1
// Generations per run: 1; m * D + 1 (a full group whose last launch feeds the exchange, and one launch more);
// 2 * m * D + 3.  Strips of 3 and the meshes 2 x 2 and 3 x 3 run all three at every extent (the thick grids of the two
// other intervals: the longest at the first extent only), the other decompositions one each in rotation.  Every run
// asserts from the drivers' counters that the interval it meant to test was in effect: n_exchanges == the sum over its
// calls of ceil(passes / m).
#pragma once
#include "shape_cases.hpp"

#ifdef __HIPCC__
#include "mesh_harness.hpp"
#include <StencilStream/hip/BlockUpdate.hpp>
#include <StencilStream/hip/StripUpdate.hpp>

#include <array>
#include <chrono>
#include <cstring>
#include <map>
#include <string>
#include <thread>

namespace shapes {

// the launches a driver plans for n generations: the deepest compiled depth, halved until it is no deeper than D and
// than what is left (ststhip.h, ststhip_strip_advance)
inline std::vector<std::size_t> planned_passes(std::size_t n, std::size_t max_generations, std::size_t D) {
    std::vector<std::size_t> passes;
    while (n > 0) {
        std::size_t t = max_generations;
        while (t > 1 && (t > n || t > D))
            t /= 2;
        passes.push_back(t);
        n -= t;
    }
    return passes;
}

enum class Interval { every_launch, rule, two };
inline Interval interval_from_environment() {
    const char *text = std::getenv("STSTHIP_EXCHANGE_EVERY");
    if (!text || std::strcmp(text, "") == 0 || std::strcmp(text, "0") == 0)
        return Interval::rule;
    if (std::strcmp(text, "1") == 0)
        return Interval::every_launch;
    if (std::strcmp(text, "2") == 0)
        return Interval::two;
    std::fprintf(stderr, "the mesh mode knows STSTHIP_EXCHANGE_EVERY unset, 1 and 2, not %s\n", text);
    std::exit(2);
}
inline const char *name_of(Interval interval) {
    return interval == Interval::every_launch ? "1" : interval == Interval::rule ? "rule" : "2";
}

struct Decomposition {
    bool strips;
    int rows, cols; // strips: rows ranks, one column of them
    int ranks() const { return rows * cols; }
    std::string name() const {
        return strips ? "strips" + std::to_string(rows) : "mesh" + std::to_string(rows) + "x" + std::to_string(cols);
    }
};
struct Call {
    std::size_t n, offset;
};

template <typename F, bool SPLIT> struct MeshCase {
    using Cell = typename F::Cell;
    using Update = stencil::hip::StencilUpdate<F, SPLIT>;
    using Strip = stencil::hip::StripUpdate<F, SPLIT>;
    using Block = stencil::hip::BlockUpdate<F, SPLIT>;
    using Reference = stencil::cpu::StencilUpdate<F>;
    static constexpr bool planes = Update::sweeps_on_planes;
    static constexpr int T = SweepTuning<F, planes>::max_generations;
    static constexpr int G = int(F::stencil_radius) * int(F::n_subiterations) * T;
    static constexpr int OW = hi::SweepOf<F, planes>::OW;
    static constexpr std::size_t unbounded = ~std::size_t(0);

    const char *name;
    u32 seed;
    Interval interval;
    ststhip_sweep_desc desc;
    std::size_t D, hpg, g;
    std::map<std::array<std::size_t, 4>, std::vector<Cell>> references; // (rows, columns, generations, offset)
    std::string extents_report, exchanges_report;
    std::size_t n_runs = 0;
    double slowest_run = 0.0, reference_seconds = 0.0;
    std::string slowest_name;

    MeshCase(const char *name, u32 seed)
        : name(name), seed(seed), interval(interval_from_environment()) {
        stencil::hip::internal::ensure_runtime(sycl::device().hip_index());
        desc = Update::sweep_description_with_host_values(); // as StripUpdate and BlockUpdate hand it to the drivers
        D = desc.alt_generations != 0 && desc.alt_generations < desc.max_generations ? desc.alt_generations
                                                                                   : desc.max_generations;
        hpg = desc.halo_depth_per_generation;
        g = D * hpg;
    }

    typename Update::Params params(Call call) const {
        return {.transition_function = F{seed}, .halo_value = halo_cell<Cell>(seed), .iteration_offset = call.offset,
                .n_iterations = call.n, .blocking = true};
    }

    // ------------------------------------------------------------------ the cpu backend on the whole grid, once per key
    std::vector<Cell> const &reference(std::size_t h, std::size_t w, std::size_t n, std::size_t offset) {
        auto found = references.find({h, w, n, offset});
        if (found != references.end())
            return found->second;
        const auto started = std::chrono::steady_clock::now();
        stencil::cpu::Grid<Cell> grid(h, w);
        {
            typename stencil::cpu::Grid<Cell>::template GridAccessor<sycl::access::mode::read_write> ac(grid);
            for (std::size_t r = 0; r < h; r++)
                for (std::size_t c = 0; c < w; c++)
                    ac[r][c] = initial_cell<Cell>(u32(r), u32(c), seed);
        }
        Reference update({.transition_function = F{seed}, .halo_value = halo_cell<Cell>(seed), .iteration_offset = offset,
                          .n_iterations = n, .blocking = true});
        stencil::cpu::Grid<Cell> out = update(grid);
        std::vector<Cell> cells(h * w);
        {
            typename stencil::cpu::Grid<Cell>::template GridAccessor<sycl::access::mode::read> ac(out);
            for (std::size_t r = 0; r < h; r++)
                for (std::size_t c = 0; c < w; c++)
                    cells[r * w + c] = ac[r][c];
        }
        reference_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - started).count();
        return references[{h, w, n, offset}] = std::move(cells);
    }

    // ------------------------------------------------------------------ one rank
    struct Report {
        std::size_t r0 = 0, r1 = 0, c0 = 0, c1 = 0;
        std::uint64_t launches = 0, exchanges = 0;
    };
    template <typename Driver>
    void drive(Driver &driver, std::size_t r0, std::size_t r1, std::size_t c0, std::size_t c1, std::size_t w,
               std::vector<Call> const &calls, Cell *got, Report &report) {
        const std::size_t n_cols = c1 - c0;
        std::vector<Cell> mine((r1 - r0) * n_cols);
        for (std::size_t r = r0; r < r1; r++)
            for (std::size_t c = c0; c < c1; c++)
                mine[(r - r0) * n_cols + (c - c0)] = initial_cell<Cell>(u32(r), u32(c), seed);
        driver.upload(mine.data());
        for (Call call : calls) { // the later calls resume through get_params(), without a new upload
            driver.get_params().iteration_offset = call.offset;
            driver.get_params().n_iterations = call.n;
            driver();
        }
        driver.download(mine.data());
        for (std::size_t r = r0; r < r1; r++)
            for (std::size_t c = c0; c < c1; c++)
                got[r * w + c] = mine[(r - r0) * n_cols + (c - c0)];
        report = Report{r0, r1, c0, c1, 0, 0};
        driver.counters(report.launches, report.exchanges);
    }
    void run_rank(Decomposition d, mesh_harness::Mesh *mesh, int rank, std::size_t h, std::size_t w,
                  std::vector<Call> const *calls, Cell *got, Report *report) {
        try {
            mesh_harness::Side side{mesh, rank};
            const bool alone = d.ranks() == 1;
            ststhip_exchange_fn rows = alone ? nullptr : &mesh_harness::exchange_rows;
            ststhip_exchange_fn cols = alone ? nullptr : &mesh_harness::exchange_cols;
            if (d.strips) {
                Strip strip(params(calls->front()), h, w, rank, d.rows, nullptr, rows, &side);
                drive(strip, strip.first_row(), strip.end_row(), 0, w, w, *calls, got, *report);
            } else {
                Block block(params(calls->front()), h, w, rank, d.rows, d.cols, nullptr, rows, &side, cols, &side);
                drive(block, block.first_row(), block.end_row(), block.first_col(), block.end_col(), w, *calls, got, *report);
            }
        } catch (std::exception const &e) {
            // the neighbours would wait for this rank until their limit: end here, with the reason
            std::fprintf(stderr, "%s, %s, %zu x %zu, rank %d: %s\n", name, d.name().c_str(), h, w, rank, e.what());
            std::_Exit(mesh_harness::exit_call_failed);
        }
    }

    // ------------------------------------------------------------------ one decomposition of one grid
    // `m`: the exchange interval the extents were chosen for; `launches_per_rank`: asserted when non-zero
    void run(Decomposition d, std::size_t h, std::size_t w, std::size_t m, std::vector<Call> calls, const char *what,
             std::uint64_t launches_per_rank = 0) {
        const auto started = std::chrono::steady_clock::now();
        std::size_t n_total = 0, groups = 0;
        for (std::size_t i = 0; i < calls.size(); i++) {
            REQUIRE(i == 0 || calls[i].offset == calls[i - 1].offset + calls[i - 1].n);
            n_total += calls[i].n;
            const std::size_t passes = planned_passes(calls[i].n, desc.max_generations, D).size();
            groups += (passes + m - 1) / m;
        }
        const std::uint64_t exchanges_wanted = d.ranks() == 1 ? 0 : groups;
        std::vector<Cell> const &want = reference(h, w, n_total, calls.front().offset);

        mesh_harness::Mesh mesh(d.rows, d.cols);
        std::vector<Cell> got(h * w, cell_from<Cell>(0xDEADu));
        std::vector<Report> reports(d.ranks());
        std::vector<std::thread> ranks;
        for (int rank = 0; rank < d.ranks(); rank++)
            ranks.emplace_back([&, rank] { run_rank(d, &mesh, rank, h, w, &calls, got.data(), &reports[rank]); });
        for (auto &t : ranks)
            t.join();

        std::string generations;
        for (Call call : calls)
            generations += (generations.empty() ? "" : "+") + std::to_string(call.n);
        const Difference diff = compare_fields<Cell>(
            h, w, [&](std::size_t r, std::size_t c) { return got[r * w + c]; },
            [&](std::size_t r, std::size_t c) { return want[r * w + c]; });
        if (diff.count != 0) {
            std::fprintf(stderr,
                         "MISMATCH %s%s: %s, %zu x %zu, m = %zu, generations %s from %zu (D = %zu, hpg = %zu): %zu cells "
                         "differ, first at (row %zu, column %zu, field %d): got %u, want %u\n",
                         name, what, d.name().c_str(), h, w, m, generations.c_str(), calls.front().offset, D, hpg, diff.count,
                         diff.row, diff.column, diff.field_index, unsigned(diff.got), unsigned(diff.want));
            for (int rank = 0; rank < d.ranks(); rank++)
                std::fprintf(stderr, "    rank %d: rows [%zu, %zu) x columns [%zu, %zu)%s\n", rank, reports[rank].r0,
                             reports[rank].r1, reports[rank].c0, reports[rank].c1,
                             diff.row >= reports[rank].r0 && diff.row < reports[rank].r1 && diff.column >= reports[rank].c0 &&
                                     diff.column < reports[rank].c1
                                 ? "   <- the first difference"
                                 : "");
        }
        REQUIRE(diff.count == 0);
        for (int rank = 0; rank < d.ranks(); rank++) {
            if (reports[rank].exchanges != exchanges_wanted)
                std::fprintf(stderr, "INTERVAL %s%s: %s, %zu x %zu, generations %s, rank %d: %llu exchanges, m = %zu means %llu\n",
                             name, what, d.name().c_str(), h, w, generations.c_str(), rank,
                             static_cast<unsigned long long>(reports[rank].exchanges), m,
                             static_cast<unsigned long long>(exchanges_wanted));
            REQUIRE(reports[rank].exchanges == exchanges_wanted);
            if (launches_per_rank != 0) {
                if (reports[rank].launches != launches_per_rank)
                    std::fprintf(stderr, "LAUNCHES %s%s: %s, rank %d: %llu launches, %llu planned\n", name, what, d.name().c_str(),
                                 rank, static_cast<unsigned long long>(reports[rank].launches),
                                 static_cast<unsigned long long>(launches_per_rank));
                REQUIRE(reports[rank].launches == launches_per_rank);
            }
        }
        const std::string tag = " " + d.name() + ":" + std::to_string(h) + "x" + std::to_string(w);
        if ((extents_report + " ").find(tag + " ") == std::string::npos)
            extents_report += tag;
        exchanges_report += tag + "/m" + std::to_string(m) + "/n" + generations + "=" + std::to_string(exchanges_wanted);
        n_runs++;
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - started).count();
        if (seconds > slowest_run) {
            slowest_run = seconds;
            slowest_name = d.name() + " " + std::to_string(h) + "x" + std::to_string(w) + " n=" + generations;
        }
    }

    // ------------------------------------------------------------------ extents
    struct Extent {
        std::size_t total, m; // m: the interval the extent lets the driver keep
    };
    // variant 0 / 1 of the header's table for an axis cut over n ranks; `small`: the extent of an axis that is not cut
    Extent extent(int n, int variant, std::size_t small, std::size_t rule_m) const {
        if (n == 1)
            return {small, unbounded};
        const std::size_t ranks = std::size_t(n);
        switch (interval) {
        case Interval::every_launch: {
            const std::size_t ragged = std::max<std::size_t>(2 * g, OW) + 1;
            return variant == 0 ? Extent{ranks * 2 * g, 1} : Extent{ranks * ragged + (ranks - 1), 1};
        }
        case Interval::rule: {
            const std::size_t ragged = std::max<std::size_t>(4 * g * rule_m, OW) + 1;
            return variant == 0 ? Extent{ranks * 4 * g * rule_m, rule_m} : Extent{ranks * ragged + (ranks - 1), rule_m};
        }
        default:
            return variant == 0 ? Extent{ranks * 8 * g, 2} : Extent{ranks * (8 * g - 1), 1};
        }
    }
    std::vector<std::size_t> counts(std::size_t m) const { return {1, m * D + 1, 2 * m * D + 3}; }

    // ------------------------------------------------------------------ the matrix
    void run_matrix() {
        const Decomposition decompositions[10] = {{true, 1, 1},  {true, 2, 1},  {true, 3, 1},  {false, 1, 1}, {false, 1, 2},
                                                  {false, 2, 1}, {false, 2, 2}, {false, 1, 3}, {false, 3, 1}, {false, 3, 3}};
        // (rows, columns) variants of the extents: limit and ragged; at STSTHIP_EXCHANGE_EVERY=2 both axes keep 2, then
        // either axis alone makes the interval fall to 1
        std::vector<std::array<int, 2>> variants = {{0, 0}, {1, 1}};
        if (interval == Interval::two)
            variants = {{0, 0}, {0, 1}, {1, 0}};
        for (std::size_t i = 0; i < 10; i++) {
            Decomposition const d = decompositions[i];
            const bool all_counts = (d.strips && d.rows == 3) || (!d.strips && d.rows == d.cols && d.rows >= 2);
            const std::size_t rule_m = d.strips ? 4 : 2;
            std::vector<std::array<std::size_t, 2>> done;
            for (std::size_t v = 0; v < variants.size(); v++) {
                const Extent rows = extent(d.rows, variants[v][0], G + 1, rule_m);
                const Extent cols = extent(d.strips ? 1 : d.cols, variants[v][1], OW + 1, rule_m);
                if (std::find(done.begin(), done.end(), std::array<std::size_t, 2>{rows.total, cols.total}) != done.end())
                    continue; // (an axis that is not cut has one extent)
                done.push_back({rows.total, cols.total});
                const std::size_t m = d.ranks() == 1 ? 1 : std::min(rows.m, cols.m);
                const std::vector<std::size_t> n = counts(m);
                if (all_counts) {
                    // (the longest run once per decomposition where the grids are thick: the cpu backend's time)
                    for (std::size_t k = 0; k < (interval == Interval::every_launch || v == 0 ? 3u : 2u); k++)
                        run(d, rows.total, cols.total, m, {{n[k], 0}}, "");
                } else {
                    // in rotation; one generation is one exchange at every interval, so where the interval must fall
                    // the run is a longer one
                    std::size_t pick = (i + v) % 3;
                    if (interval == Interval::two && m == 1 && pick == 0)
                        pick = 1;
                    run(d, rows.total, cols.total, m, {{n[pick], 0}}, "");
                }
            }
            // once per case, on the ragged extents (at STSTHIP_EXCHANGE_EVERY=2: the ones that keep 2)
            const int v = interval == Interval::two ? 0 : 1;
            const Extent rows = extent(d.rows, v, G + 1, rule_m), cols = extent(d.strips ? 1 : d.cols, v, OW + 1, rule_m);
            const std::size_t m = d.ranks() == 1 ? 1 : std::min(rows.m, cols.m);
            if (d.ranks() == 2 || (!d.strips && d.rows == 2 && d.cols == 2))
                run(d, rows.total, cols.total, m, {{m * D + 1, 5}}, " (offset)");
            if ((d.strips && d.rows == 3) || (!d.strips && d.rows == 3 && d.cols == 3)) {
                // a second call resumes through get_params() after an odd number of launches: the other buffer set is
                // the current one
                std::size_t first = m * D + 1;
                while (planned_passes(first, desc.max_generations, D).size() % 2 == 0)
                    first++;
                run(d, rows.total, cols.total, m, {{first, 0}, {D + 2, first}}, " (resumed)");
            }
        }
        if (interval == Interval::every_launch)
            check_refusals();
        report("mesh");
    }

    // ------------------------------------------------------------------ thinner than two ghost depths: refused
    void check_refusals() {
        Update update(params({1, 0}));
        mesh_harness::Side nobody{nullptr, 0}; // (never called: nothing is launched)
        const std::size_t thin = 2 * g - 1, thick = 2 * g;
        ststhip_strip handle = nullptr;
        int rc = ststhip_strip_create_custom(Update::launch_entry(), &update, &desc, 2 * thin, OW + 1, 0, 2, nullptr,
                                             &mesh_harness::exchange_rows, &nobody, &handle);
        REQUIRE(rc == STSTHIP_ERR_INVALID && handle == nullptr);
        const std::size_t extents[2][2] = {{2 * thin, 2 * thick}, {2 * thick, 2 * thin}};
        for (auto const &e : extents) {
            rc = ststhip_block_create_custom(Update::launch_entry(), &update, &desc, e[0], e[1], 0, 2, 2, nullptr,
                                             &mesh_harness::exchange_rows, &nobody, &mesh_harness::exchange_cols, &nobody,
                                             &handle);
            REQUIRE(rc == STSTHIP_ERR_INVALID && handle == nullptr);
        }
    }

    // ------------------------------------------------------------------ a strip as two sub-strips with a moving boundary
    // (STSTHIP_STRIP_SUBSTRIPS=2, ststhip_strip_advance): 3 ranks at the smallest owned height the driver accepts for
    // two sub-strips, enough generations that the boundary moves further than its span and starts over
    void run_substrips() {
        std::size_t m = interval == Interval::every_launch ? 1 : interval == Interval::two ? 2 : 4;
        // the boundary's span is a quarter of the owned rows once the run's ghost rows add up to that much
        std::size_t rows = 8 * g;
        while (!(rows / 4 >= 2 * g && rows >= 2 * (g * m + 2 * g) + 2 * (rows / 4) + 64 && rows >= 4 * g * m))
            rows++;
        const std::size_t n = (rows / 4 + hpg - 1) / hpg + 2 * m * D + 3; // moves further than the span
        const std::vector<std::size_t> passes = planned_passes(n, desc.max_generations, D);
        REQUIRE(passes.size() >= 2);
        std::size_t moved = 0;
        for (std::size_t i = 0; i < passes.size(); i++)
            moved += std::max(passes[i], i ? passes[i - 1] : 0) * hpg;
        REQUIRE(moved > rows / 4);
        // per pass an upper and a lower launch; per group but the first one launch of the boundary bands in front of
        // the exchange (the middle rank: both bands as one launch with a row hole)
        const std::size_t groups = (passes.size() + m - 1) / m;
        run({true, 3, 1}, 3 * rows, OW + 1, m, {{n, 0}}, " (two sub-strips)", 2 * passes.size() + (groups - 1));
        report("substrips");
    }

    void report(const char *mode) {
        std::printf("%s shape %s: D=%zu hpg=%zu g=%zu interval=%s runs=%zu reference=%.2fs slowest=%.2fs (%s) extents:%s "
                    "exchanges:%s\n",
                    mode, name, D, hpg, g, name_of(interval), n_runs, reference_seconds, slowest_run, slowest_name.c_str(),
                    extents_report.c_str(), exchanges_report.c_str());
        std::fflush(stdout);
    }
};

// the second mode of a shape binary: true when the arguments asked for it (and it has run)
template <typename F, bool SPLIT = false> void run_mesh_case(const char *mode, const char *name, u32 seed) {
    MeshCase<F, SPLIT> c(name, seed);
    if (std::strcmp(mode, "mesh") == 0)
        c.run_matrix();
    else
        c.run_substrips();
}
inline const char *mesh_mode(int argc, char **argv) {
    if (argc < 2)
        return nullptr;
    if (argc == 2 && (std::strcmp(argv[1], "mesh") == 0 || std::strcmp(argv[1], "substrips") == 0))
        return argv[1];
    std::fprintf(stderr, "usage: %s [mesh | substrips]\n", argv[0]);
    std::exit(2);
}

} // namespace shapes
#endif // __HIPCC__

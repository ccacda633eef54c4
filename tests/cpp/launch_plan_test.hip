// The launch plan of a sweep, checked on the host: pick_chunk_rows and plan_tiers (Sweep.hpp) against the decode
// Sweep::entry() applies to blockIdx on the device.  No kernel is instantiated and the GPU is never opened: the
// planners read ststhip_options and the launch concurrency only, and ststhip_compute_units answers 256 before
// ststhip_init.
//
//   launch_plan_test                                   properties over a sweep of options and launch shapes
//   launch_plan_test plan <out_begin> <out_end> <grid_h> <halo_rows> [overhead_rows [resident_blocks [units_per_block]]]
//                                                      one JSON line: the plan of such a launch (three column strips)
//                                                      under the STSTHIP_* environment the program was started in
//
// The decode (unit -> chunk -> tier -> rows) and the XCD renumbering are RESTATED here on purpose; they mirror
// Sweep::entry() in include/StencilStream/hip/internal/Sweep.hpp:
//   renumbering          lines 1009-1014   (block = x * q + min(x, r) + block / n_xcd)
//   unit -> strip, chunk lines 1019-1026   (the bottom chunk second when last_chunk_early and n_chunks >= 3)
//   chunk -> tier        lines 1027-1031
//   tier -> (ya, yb)     lines 1032-1034
#include <StencilStream/hip/internal/Sweep.hpp>
#include <ststhip.h>

#include "mini_test.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using stencil::hip::internal::pick_chunk_rows;
using stencil::hip::internal::plan_tiers;
using stencil::hip::internal::SweepGeometry;

static long g_cases = 0;

static void set_knob(const char *name, const char *value) {
    if (value)
        setenv(name, value, 1);
    else
        unsetenv(name);
}

// rows [ya, yb) of unit `unit` of one column strip: Sweep::entry(), lines 1024-1034
static void decode(SweepGeometry const &g, unsigned unit, int &ya, int &yb) {
    int chunk = int(unit);
    if (g.last_chunk_early && g.n_chunks >= 3)
        chunk = chunk == 0 ? 0 : (chunk == 1 ? int(g.n_chunks) - 1 : chunk - 1);
    int tier = 0;
    for (int t = 1; t < SweepGeometry::max_tiers; t++)
        if (t < int(g.n_tiers) && unsigned(chunk) >= g.tier_first[t])
            tier = t;
    ya = g.tier_begin[tier] + (chunk - int(g.tier_first[tier])) * g.tier_rows[tier];
    yb = ya + g.tier_rows[tier];
    yb = yb < g.out_end ? yb : g.out_end;
}

// The plan launch_sweep makes for rows [out_begin, out_end) with chunks of `chunk_rows` rows (lines 1286-1289, 1299).
static SweepGeometry plan_of(int out_begin, int out_end, int chunk_rows, bool last_chunk_early) {
    SweepGeometry g;
    std::memset(&g, 0, sizeof g);
    g.out_begin = out_begin;
    g.out_end = out_end;
    g.chunk_rows = chunk_rows;
    g.n_strips = 3;
    g.n_chunks = unsigned((out_end - out_begin + chunk_rows - 1) / chunk_rows);
    plan_tiers(g, out_end - out_begin);
    g.last_chunk_early = last_chunk_early ? 1u : 0u;
    return g;
}

static bool same_plan(SweepGeometry const &a, SweepGeometry const &b) {
    if (a.n_tiers != b.n_tiers || a.n_chunks != b.n_chunks)
        return false;
    for (unsigned t = 0; t < a.n_tiers; t++)
        if (a.tier_first[t] != b.tier_first[t] || a.tier_rows[t] != b.tier_rows[t] || a.tier_begin[t] != b.tier_begin[t])
            return false;
    return a.tier_first[a.n_tiers] == b.tier_first[b.n_tiers];
}

// every property of one plan; `cover` is scratch of at least out_end - out_begin entries
static void check_plan(SweepGeometry const &g, std::vector<int> &cover) {
    g_cases++;
    const int out_rows = g.out_end - g.out_begin;
    REQUIRE(g.n_tiers >= 1 && g.n_tiers <= unsigned(SweepGeometry::max_tiers));
    if (g.n_tiers < 1 || g.n_tiers > unsigned(SweepGeometry::max_tiers))
        return;
    bool firsts = g.tier_first[0] == 0 && g.tier_first[g.n_tiers] == g.n_chunks && g.n_chunks >= 1;
    bool rows = g.tier_rows[0] == g.chunk_rows && g.tier_rows[0] >= 1;
    bool begins = g.tier_begin[0] == g.out_begin;
    for (unsigned t = 1; t <= g.n_tiers; t++)
        firsts = firsts && g.tier_first[t] > g.tier_first[t - 1];
    for (unsigned t = 1; t < g.n_tiers; t++) {
        rows = rows && g.tier_rows[t] < g.tier_rows[t - 1] && g.tier_rows[t] >= 4;
        begins = begins && g.tier_begin[t] == g.tier_begin[t - 1] + int(g.tier_first[t] - g.tier_first[t - 1]) * g.tier_rows[t - 1];
    }
    REQUIRE(firsts);
    REQUIRE(rows);
    REQUIRE(begins);
    if (!firsts)
        return; // (the decode below would index by a broken table)
    std::fill(cover.begin(), cover.begin() + out_rows, 0);
    bool inside = true, none_empty = true;
    for (unsigned unit = 0; unit < g.n_chunks; unit++) {
        int ya, yb;
        decode(g, unit, ya, yb);
        none_empty = none_empty && ya < yb;
        if (ya < g.out_begin || yb > g.out_end) {
            inside = false;
            continue;
        }
        for (int y = ya; y < yb; y++)
            cover[y - g.out_begin]++;
    }
    bool exactly_once = true;
    for (int y = 0; y < out_rows; y++)
        exactly_once = exactly_once && cover[y] == 1;
    REQUIRE(inside);
    REQUIRE(none_empty);
    REQUIRE(exactly_once);
}

static const int kChunkRows[] = {1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 31, 32, 40, 64, 100, 128, 333, 700, 1000000};

// STSTHIP_TAPER specs: unset (the default taper), empty, one to three entries, entries that cannot apply
static const char *const kTapers[] = {
    nullptr, "", "120:4", "150:2", "500:2", "1000:2", "999:3", "1:2", "500:2,250:4", "600:2,300:4", "300:2,600:4",
    "600:2,300:4,150:8", "500:2,250:4,125:8", "900:2,800:3,700:5", "500:3,400:5,100:7", "800:2,400:2,200:4",
    "500:1", "500:0", "0:4", "1500:2", "-5:2", "500:2,0:4,250:4", "500:1,250:4", "2000:2,500:4,250:8", "500:2,250:4,125:8,60:16",
    "500:1000000", "garbage", "500", "500:2,", ":", "700:2,700:4"};

TEST_CASE(tiers_tile_the_row_range) {
    std::vector<int> cover(701);
    const int begins[] = {0, 23};
    for (const char *taper : kTapers) {
        set_knob("STSTHIP_TAPER", taper);
        ststhip_reload_options();
        for (int concurrency = 1; concurrency <= 2; concurrency++) {
            ststhip_set_launch_concurrency(concurrency);
            for (int out_rows = 1; out_rows <= 700; out_rows++)
                for (int chunk : kChunkRows)
                    for (int early = 0; early < 2; early++) {
                        const int out_begin = begins[(out_rows + early) & 1];
                        check_plan(plan_of(out_begin, out_begin + out_rows, std::min(chunk, out_rows), early != 0), cover);
                    }
        }
    }
    ststhip_set_launch_concurrency(1);
    set_knob("STSTHIP_TAPER", nullptr);
    ststhip_reload_options();
}

// A taper entry that cannot apply is skipped.  Two kinds never apply, whatever the launch: a split of 1 or less, and
// a permille above 1000 (it is clamped to 1000, the tier would start where the one before it starts); the plan is then
// the plan of the other entries.  The other kinds depend on the launch: an entry that does not shrink the chunks is
// skipped (tier_rows strictly decreasing, check_plan), but may apply where an earlier entry could not; a permille of 0
// names a tier that starts at the launch's end and is moved down to a chunk boundary like any other start, so a ragged
// last chunk is cut finer on its own -- a valid tiling; it adds no tier where the chunks divide the rows.
TEST_CASE(inapplicable_taper_entries_are_skipped) {
    std::vector<int> cover(701);
    struct {
        const char *spec, *same_as;
    } const pairs[] = {{"500:1", ""},
                       {"500:0", ""},
                       {"500:-3", ""},
                       {"1500:2", ""},
                       {"1001:4", ""},
                       {"500:1,250:4", "250:4"},
                       {"2000:2,500:4", "500:4"},
                       {"500:2,1500:4,250:8", "500:2,250:8"},
                       {"500:2,500:1,250:4", "500:2,250:4"},
                       {"600:2,300:4,300:0", "600:2,300:4"}};
    const int rows_list[] = {1, 5, 16, 17, 100, 108, 157, 255, 640, 700};
    const int chunk_list[] = {4, 8, 16, 40, 64, 100, 700};
    for (auto const &pair : pairs)
        for (int out_rows : rows_list)
            for (int chunk : chunk_list) {
                set_knob("STSTHIP_TAPER", pair.spec);
                ststhip_reload_options();
                const SweepGeometry with = plan_of(3, 3 + out_rows, std::min(chunk, out_rows), true);
                check_plan(with, cover);
                set_knob("STSTHIP_TAPER", pair.same_as);
                ststhip_reload_options();
                const SweepGeometry without = plan_of(3, 3 + out_rows, std::min(chunk, out_rows), true);
                if (!same_plan(with, without) && g_failures < 20)
                    std::fprintf(stderr, "taper %s differs from %s at %d rows in chunks of %d\n", pair.spec, pair.same_as,
                                 out_rows, chunk);
                REQUIRE(same_plan(with, without));
                if (!*pair.same_as)
                    REQUIRE(with.n_tiers == 1);
            }
    for (const char *spec : {"0:4", "-5:2", "500:2,400:2", "500:4,250:2", "700:2,700:4", "500:2,0:4,250:4", "300:8,600:4,900:2"}) {
        set_knob("STSTHIP_TAPER", spec);
        ststhip_reload_options();
        for (int out_rows : rows_list)
            for (int chunk : chunk_list) {
                const SweepGeometry g = plan_of(3, 3 + out_rows, std::min(chunk, out_rows), true);
                check_plan(g, cover);
                if (std::atoi(spec) <= 0 && out_rows % std::min(chunk, out_rows) == 0)
                    REQUIRE(g.n_tiers == 1);
            }
    }
    // the plans the GPU tests force: three and four tiers on their three row ranges
    set_knob("STSTHIP_TAPER", "500:2,250:4");
    ststhip_reload_options();
    for (int out_rows : {157, 108, 97}) {
        const SweepGeometry g = plan_of(0, out_rows, 16, false);
        REQUIRE(g.n_tiers == 3 && g.tier_rows[1] == 8 && g.tier_rows[2] == 4);
    }
    set_knob("STSTHIP_TAPER", "600:2,300:4,150:8");
    ststhip_reload_options();
    for (int out_rows : {157, 108}) {
        const SweepGeometry g = plan_of(0, out_rows, 40, false);
        REQUIRE(g.n_tiers == 4 && g.tier_rows[1] == 20 && g.tier_rows[2] == 10 && g.tier_rows[3] == 5);
    }
    set_knob("STSTHIP_TAPER", nullptr);
    ststhip_reload_options();
}

// Sweep::entry(), lines 1009-1014: a bijection of [0, gridDim)
TEST_CASE(xcd_renumbering_is_a_bijection) {
    for (unsigned grid_dim = 1; grid_dim <= 300; grid_dim++) {
        std::vector<int> hit(grid_dim, 0);
        bool inside = true;
        for (unsigned b = 0; b < grid_dim; b++) {
            constexpr unsigned n_xcd = 8;
            const unsigned q = grid_dim / n_xcd, r = grid_dim % n_xcd, x = b % n_xcd;
            const unsigned block = x * q + (x < r ? x : r) + b / n_xcd;
            if (block < grid_dim)
                hit[block]++;
            else
                inside = false;
        }
        bool once = true;
        for (unsigned b = 0; b < grid_dim; b++)
            once = once && hit[b] == 1;
        g_cases++;
        REQUIRE(inside);
        REQUIRE(once);
    }
}

TEST_CASE(chunk_rows_stay_inside_the_launch) {
    std::vector<int> out_rows_list, strips_list;
    for (int v = 1; v <= 48; v++)
        out_rows_list.push_back(v);
    for (int v : {63, 64, 97, 100, 108, 157, 255, 256, 300, 511, 700, 1000, 1024, 2047, 2048, 4095, 4999, 5000})
        out_rows_list.push_back(v);
    for (int v : {1, 2, 3, 5, 8, 17, 64, 100, 255, 256, 300})
        strips_list.push_back(v);
    const char *const tails[] = {nullptr, "50", "2000"};
    const char *const chunks[] = {nullptr, "1", "1000000"};
    for (const char *tail : tails)
        for (const char *chunk : chunks) {
            set_knob("STSTHIP_TAIL_PERMILLE", tail);
            set_knob("STSTHIP_CHUNK_ROWS", chunk);
            ststhip_reload_options();
            for (int concurrency = 1; concurrency <= 3; concurrency++) {
                ststhip_set_launch_concurrency(concurrency);
                bool ok = true;
                long calls = 0;
                for (int out_rows : out_rows_list)
                    for (int n_strips : strips_list)
                        for (int overhead : {2, 8, 32, 44, 70, 139, 140})
                            for (int resident = 1; resident <= 8; resident++)
                                for (int units_per_block : {1, 4})
                                    for (int beside : {350, 200}) {
                                        bool kernel_rule = false;
                                        const int rows = pick_chunk_rows(out_rows, unsigned(n_strips), overhead, resident,
                                                                         units_per_block, beside, &kernel_rule);
                                        ok = ok && rows >= 1 && rows <= out_rows;
                                        calls++;
                                    }
                g_cases += calls;
                REQUIRE(ok);
                // a forced length is the length, clipped to the launch
                if (chunk) {
                    REQUIRE(pick_chunk_rows(157, 3, 44, 2, 1) == std::min(std::atoi(chunk), 157));
                    REQUIRE(pick_chunk_rows(1, 3, 44, 2, 1) == 1);
                }
            }
        }
    ststhip_set_launch_concurrency(1);
    set_knob("STSTHIP_TAIL_PERMILLE", nullptr);
    set_knob("STSTHIP_CHUNK_ROWS", nullptr);
    ststhip_reload_options();
    // ... and what it picks tiles the launch with the taper of the environment it was picked in
    std::vector<int> cover(5001);
    for (int out_rows : out_rows_list)
        for (int n_strips : {1, 3, 64})
            for (int early = 0; early < 2; early++) {
                const int rows = pick_chunk_rows(out_rows, unsigned(n_strips), 44, 2, 1);
                check_plan(plan_of(7, 7 + out_rows, rows, early != 0), cover);
            }
}

static int print_plan(int argc, char **argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s plan <out_begin> <out_end> <grid_h> <halo_rows> [overhead_rows [resident_blocks "
                             "[units_per_block]]]\n", argv[0]);
        return 2;
    }
    const int out_begin = std::atoi(argv[2]), out_end = std::atoi(argv[3]), grid_h = std::atoi(argv[4]);
    const int halo_rows = std::atoi(argv[5]);
    const int overhead_rows = argc > 6 ? std::atoi(argv[6]) : 2 * halo_rows;
    const int resident_blocks = argc > 7 ? std::atoi(argv[7]) : 2;
    const int units_per_block = argc > 8 ? std::atoi(argv[8]) : 1;
    if (out_begin < 0 || out_end <= out_begin || out_end > grid_h || halo_rows < 0) {
        std::fprintf(stderr, "need 0 <= out_begin < out_end <= grid_h and halo_rows >= 0\n");
        return 2;
    }
    ststhip_options const &opt = *ststhip_get_options(); // (read from the environment at first use)
    SweepGeometry g;
    std::memset(&g, 0, sizeof g);
    g.out_begin = out_begin;
    g.out_end = out_end;
    g.n_strips = 3;
    // Sweep.hpp, launch_sweep, lines 1286-1289 and 1298-1299
    g.chunk_rows = pick_chunk_rows(out_end - out_begin, g.n_strips, overhead_rows, resident_blocks, units_per_block);
    g.n_chunks = unsigned((out_end - out_begin + g.chunk_rows - 1) / g.chunk_rows);
    plan_tiers(g, out_end - out_begin);
    g.xcd_remap = opt.xcd_remap ? 1u : 0u;
    g.last_chunk_early = (out_end + halo_rows > grid_h && opt.last_chunk_early) ? 1u : 0u;
    std::string tiers;
    for (unsigned t = 0; t < g.n_tiers; t++)
        tiers += (t ? ",[" : "[") + std::to_string(g.tier_first[t]) + "," + std::to_string(g.tier_rows[t]) + "," +
                 std::to_string(g.tier_begin[t]) + "]";
    std::printf("{\"chunk_rows\":%d,\"n_chunks\":%u,\"tiers\":[%s],\"last_chunk_early\":%u,\"xcd_remap\":%u}\n", g.chunk_rows,
                g.n_chunks, tiers.c_str(), g.last_chunk_early, g.xcd_remap);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "plan") == 0)
        return print_plan(argc, argv);
    if (argc > 1) {
        std::fprintf(stderr, "unknown mode %s\n", argv[1]);
        return 2;
    }
    // the properties hold for the options this file sets, whatever the caller's environment says
    for (const char *knob : {"STSTHIP_CHUNK_ROWS", "STSTHIP_TAIL_PERMILLE", "STSTHIP_TAPER", "STSTHIP_XCD_REMAP",
                             "STSTHIP_LAST_CHUNK_EARLY"})
        unsetenv(knob);
    ststhip_reload_options();
    tiers_tile_the_row_range();
    inapplicable_taper_entries_are_skipped();
    xcd_renumbering_is_a_bijection();
    chunk_rows_stay_inside_the_launch();
    std::printf("launch plan: %ld cases\n", g_cases);
    return finish("launch_plan_test");
}

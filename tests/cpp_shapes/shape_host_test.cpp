// The reference of the shape coverage, pinned on the host: stencil::cpu::StencilUpdate on every functor of
// shape_cases.hpp and hook_cases.hpp (the one-way read policy and the copied constant field among them) against a plain double loop over two arrays that substitutes the halo, steps through the sub-iterations
// and the generations and evaluates the time-dependent value by hand (no Stencil object).  g++, runs anywhere.
#include "hook_cases.hpp"

using namespace shapes;

template <typename F> static void pin_reference(const char *name, u32 seed, std::size_t h, std::size_t w, std::size_t n,
                                                std::size_t offset) {
    using Cell = typename F::Cell;
    constexpr long R = long(F::stencil_radius);
    const F f{seed};
    const Cell halo = halo_cell<Cell>(seed);

    stencil::cpu::Grid<Cell> grid(h, w);
    std::vector<Cell> now(h * w), next(h * w);
    {
        typename stencil::cpu::Grid<Cell>::template GridAccessor<sycl::access::mode::read_write> ac(grid);
        for (std::size_t r = 0; r < h; r++)
            for (std::size_t c = 0; c < w; c++)
                now[r * w + c] = ac[r][c] = initial_cell<Cell>(u32(r), u32(c), seed);
    }
    stencil::cpu::StencilUpdate<F> update(
        {.transition_function = f, .halo_value = halo, .iteration_offset = offset, .n_iterations = n, .blocking = true});
    stencil::cpu::Grid<Cell> out = update(grid);

    for (std::size_t i = offset; i < offset + n; i++) {
        const u32 tdv = tdv_word(f.get_time_dependent_value(i));
        for (std::size_t sub = 0; sub < F::n_subiterations; sub++) {
            for (long r = 0; r < long(h); r++)
                for (long c = 0; c < long(w); c++) {
                    const Context context{u32(r), u32(c), u32(h), u32(w), u32(i), u32(sub), tdv};
                    next[r * w + c] = f.evaluate(context, [&](int dr, int dc) {
                        const long nr = r + dr, nc = c + dc;
                        static_assert(R >= 1);
                        return (nr < 0 || nc < 0 || nr >= long(h) || nc >= long(w)) ? halo : now[nr * long(w) + nc];
                    });
                }
            now.swap(next);
        }
    }

    typename stencil::cpu::Grid<Cell>::template GridAccessor<sycl::access::mode::read> ac(out);
    const Difference d = compare_fields<Cell>(
        h, w, [&](std::size_t r, std::size_t c) { return ac[r][c]; },
        [&](std::size_t r, std::size_t c) { return now[r * w + c]; });
    if (d.count != 0)
        std::fprintf(stderr,
                     "MISMATCH %s: %zu x %zu, n = %zu, offset = %zu: %zu cells differ, first at (row %zu, column %zu, "
                     "field %d): cpu backend %u, plain loop %u\n",
                     name, h, w, n, offset, d.count, d.row, d.column, d.field_index, unsigned(d.got), unsigned(d.want));
    REQUIRE(d.count == 0);
    // the functor is not constant: the run changed the grid (or there was nothing to run)
    bool changed = false;
    for (std::size_t r = 0; r < h; r++)
        for (std::size_t c = 0; c < w; c++) {
            Cell const before = initial_cell<Cell>(u32(r), u32(c), seed), after = now[r * w + c];
            changed = changed || !(field<0>(before) == field<0>(after));
        }
    REQUIRE(changed || n == 0);
    // ... except in the fields the functor declares constant: the last field of such a cell never changes
    if constexpr (requires { F::constant_fields; }) {
        constexpr int last = n_fields<Cell>() - 1;
        bool kept = true;
        for (std::size_t r = 0; r < h; r++)
            for (std::size_t c = 0; c < w; c++)
                kept = kept && field<last>(initial_cell<Cell>(u32(r), u32(c), seed)) == field<last>(now[r * w + c]);
        REQUIRE(kept);
    }
}

template <typename F> static void pin(const char *name, u32 seed) {
    constexpr std::size_t R = F::stencil_radius;
    pin_reference<F>(name, seed, 1, 1, 3, 0);
    pin_reference<F>(name, seed, 1, 4 * R + 3, 4, 5);  // a single row
    pin_reference<F>(name, seed, 2 * R + 5, 2 * R + 4, 5, 2);
    std::printf("reference %s: radius %zu, %zu sub-iterations, %d fields\n", name, R, std::size_t(F::n_subiterations),
                n_fields<typename F::Cell>());
}

int main() {
    pin<U16>("U16", 0x1001u);
    pin<Quad1>("Quad1", 0x1002u);
    pin<Tri1>("Tri1", 0x1003u);
    pin<F3>("F3", 0x2001u);
    pin<D1>("D1", 0x2002u);
    pin<Octo1>("Octo1", 0x3001u);
    pin<Penta1>("Penta1", 0x3002u);
    pin<Mixed2>("Mixed2", 0x3003u);
    pin<F2x2>("F2x2", 0x4001u);
    pin<F3x1>("F3x1", 0x4002u);
    pin<D2x1>("D2x1", 0x4003u);
    pin<Canary>("Canary", 0x5001u);
    pin<Rim>("Rim", 0x5002u);
    pin<Levels>("Levels", 0x5003u);
    pin<OneWayRim>("OneWayRim", 0x5004u);
    pin<OneWay>("OneWay", 0x5101u);
    pin<OneWayPlanes>("OneWayPlanes", 0x5102u);
    pin<Liar>("Liar", 0x5103u);
    pin<Lone8>("Lone8", 0x5201u);
    pin<Twelve>("Twelve", 0x5202u);
    pin<Batch8>("Batch8", 0x5203u);
    pin<FatOn>("FatOn", 0x5204u);
    pin<Stateless>("Stateless", 0x5005u);
    pin<State7>("State7", 0x5302u);
    pin<State16>("State16", 0x5303u);
    pin<State36>("State36", 0x5304u);
    pin<State40>("State40", 0x5305u);
    pin<StateTable>("StateTable", 0x5306u);
    return finish("shape_host_test");
}

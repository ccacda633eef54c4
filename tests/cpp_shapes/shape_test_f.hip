// Hooks, hints and tunings of the template sweep, part f: the column hint: one-way reads as AoS and on planes with a
// constant field, and a functor whose hint is wrong (hook_cases.hpp; run by tests/test_template_hooks_gpu.py).  With
// the argument "mesh": the two hinted functors through the strip and block drivers (mesh_cases.hpp; run by
// tests/test_mesh_shapes_gpu.py).
#include "mesh_cases.hpp"
#include "hook_cases.hpp"

using namespace shapes;

int main(int argc, char **argv) {
    if (const char *mode = mesh_mode(argc, argv)) {
        run_mesh_case<OneWay>(mode, "OneWay", 0x5101u);
        run_mesh_case<OneWayPlanes, true>(mode, "OneWayPlanes/planes", 0x5102u);
        return finish("shape_test_f");
    }
    run_case<OneWay>("OneWay", 0x5101u);
    // (4 T + 1 generations: five passes, from the third on without the constant plane's stores)
    run_case<OneWayPlanes, true>("OneWayPlanes/planes", 0x5102u, {4 * 4 + 1});
    run_liar(0x5103u);
    return finish("shape_test_f");
}

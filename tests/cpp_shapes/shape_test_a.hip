// Shape coverage of the template sweep, part a: the sub-word cell with its depth 16, the 16-byte AoS cell, the three-float cell as AoS
// (shape_cases.hpp; run by tests/test_template_shapes_gpu.py).  With the argument "mesh" or "substrips": the same functors
// through the strip and block drivers (mesh_cases.hpp; run by tests/test_mesh_shapes_gpu.py).
#include "mesh_cases.hpp"

using namespace shapes;

int main(int argc, char **argv) {
    if (const char *mode = mesh_mode(argc, argv)) {
        run_mesh_case<U16>(mode, "U16", 0x1001u);
        run_mesh_case<Quad1, true>(mode, "Quad1/split-request", 0x1002u);
        run_mesh_case<Tri1>(mode, "Tri1/aos", 0x1003u);
        return finish("shape_test_a");
    }
    run_case<U16>("U16", 0x1001u);
    run_case<Quad1, true>("Quad1/split-request", 0x1002u);
    run_case<Tri1>("Tri1/aos", 0x1003u);
    return finish("shape_test_a");
}

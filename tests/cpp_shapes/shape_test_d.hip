// Shape coverage of the template sweep, part d: radius 2 and 3
// (shape_cases.hpp; run by tests/test_template_shapes_gpu.py).  With the argument "mesh" or "substrips": the same functors
// through the strip and block drivers (mesh_cases.hpp; run by tests/test_mesh_shapes_gpu.py).
#include "mesh_cases.hpp"

using namespace shapes;

int main(int argc, char **argv) {
    if (const char *mode = mesh_mode(argc, argv)) {
        run_mesh_case<F2x2>(mode, "F2x2", 0x4001u);
        run_mesh_case<F3x1>(mode, "F3x1", 0x4002u);
        run_mesh_case<D2x1>(mode, "D2x1", 0x4003u);
        return finish("shape_test_d");
    }
    run_case<F2x2>("F2x2", 0x4001u);
    run_case<F3x1>("F3x1", 0x4002u);
    run_case<D2x1>("D2x1", 0x4003u);
    return finish("shape_test_d");
}

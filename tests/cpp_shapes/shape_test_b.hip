// Shape coverage of the template sweep, part b: the relaxed depth 6 with a struct as time-dependent value, one double per cell, the three-float cell on planes
// (shape_cases.hpp; run by tests/test_template_shapes_gpu.py).  With the argument "mesh" or "substrips": the same functors
// through the strip and block drivers (mesh_cases.hpp; run by tests/test_mesh_shapes_gpu.py).
#include "mesh_cases.hpp"

using namespace shapes;

int main(int argc, char **argv) {
    if (const char *mode = mesh_mode(argc, argv)) {
        run_mesh_case<F3>(mode, "F3", 0x2001u);
        run_mesh_case<D1>(mode, "D1", 0x2002u);
        run_mesh_case<Tri1, true>(mode, "Tri1/planes", 0x2003u);
        return finish("shape_test_b");
    }
    run_case<F3>("F3", 0x2001u);
    run_case<D1>("D1", 0x2002u);
    run_case<Tri1, true>("Tri1/planes", 0x2003u);
    return finish("shape_test_b");
}

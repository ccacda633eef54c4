// Shape coverage of the template sweep, part c: the fat cells: 32 bytes at the LDS limit, five doubles, planes of 1, 2 and 8 bytes
// (shape_cases.hpp; run by tests/test_template_shapes_gpu.py).  With the argument "mesh" or "substrips": the same functors
// through the strip and block drivers (mesh_cases.hpp; run by tests/test_mesh_shapes_gpu.py).
#include "mesh_cases.hpp"

using namespace shapes;

int main(int argc, char **argv) {
    if (const char *mode = mesh_mode(argc, argv)) {
        run_mesh_case<Octo1>(mode, "Octo1", 0x3001u);
        run_mesh_case<Penta1>(mode, "Penta1", 0x3002u);
        run_mesh_case<Mixed2, true>(mode, "Mixed2/planes", 0x3003u);
        return finish("shape_test_c");
    }
    run_case<Octo1>("Octo1", 0x3001u);
    run_case<Penta1>("Penta1", 0x3002u);
    run_case<Mixed2, true>("Mixed2/planes", 0x3003u);
    return finish("shape_test_c");
}

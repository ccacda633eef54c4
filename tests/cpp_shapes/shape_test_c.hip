// Shape coverage of the template sweep, part c: the fat cells: 32 bytes at the LDS limit, five doubles, planes of 1, 2 and 8 bytes
// (shape_cases.hpp; run by tests/test_template_shapes_gpu.py).
#include "shape_cases.hpp"

using namespace shapes;

int main() {
    run_case<Octo1>("Octo1", 0x3001u);
    run_case<Penta1>("Penta1", 0x3002u);
    run_case<Mixed2, true>("Mixed2/planes", 0x3003u);
    return finish("shape_test_c");
}

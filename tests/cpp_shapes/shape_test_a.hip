// Shape coverage of the template sweep, part a: the sub-word cell with its depth 16, the 16-byte AoS cell, the three-float cell as AoS
// (shape_cases.hpp; run by tests/test_template_shapes_gpu.py).
#include "shape_cases.hpp"

using namespace shapes;

int main() {
    run_case<U16>("U16", 0x1001u);
    run_case<Quad1, true>("Quad1/split-request", 0x1002u);
    run_case<Tri1>("Tri1/aos", 0x1003u);
    return finish("shape_test_a");
}

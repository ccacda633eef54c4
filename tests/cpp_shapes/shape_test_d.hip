// Shape coverage of the template sweep, part d: radius 2 and 3
// (shape_cases.hpp; run by tests/test_template_shapes_gpu.py).
#include "shape_cases.hpp"

using namespace shapes;

int main() {
    run_case<F2x2>("F2x2", 0x4001u);
    run_case<F3x1>("F3x1", 0x4002u);
    run_case<D2x1>("D2x1", 0x4003u);
    return finish("shape_test_d");
}

// Hooks, hints and tunings of the template sweep, part j: the function object's state: ten words, a table indexed at
// run time; the time-dependent values evaluated by the kernel and precomputed on the device (hook_cases.hpp; run by
// tests/test_template_hooks_gpu.py).
#include "hook_cases.hpp"

using namespace shapes;

int main() {
    run_case<State40>("State40", 0x5305u);
    run_case<StateTable>("StateTable", 0x5306u);
    run_case<F3, false, stencil::tdv::single_pass::InlineStrategy>("F3/inline", 0x2001u);
    run_case<F3, false, stencil::tdv::single_pass::PrecomputeOnDeviceStrategy>("F3/on-device", 0x2001u);
    return finish("shape_test_j");
}

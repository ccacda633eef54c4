// Hooks, hints and tunings of the template sweep, part g: explicit tunings: independent waves eight deep, twelve
// generations on four stages (hook_cases.hpp; run by tests/test_template_hooks_gpu.py).
#include "hook_cases.hpp"

using namespace shapes;

int main() {
    run_case<Lone8>("Lone8", 0x5201u);
    run_case<Twelve>("Twelve", 0x5202u);
    return finish("shape_test_g");
}

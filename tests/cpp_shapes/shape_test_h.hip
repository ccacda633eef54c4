// Hooks, hints and tunings of the template sweep, part h: explicit tunings: batches of eight rows with every toggle
// off, a fat cell with every toggle on (hook_cases.hpp; run by tests/test_template_hooks_gpu.py).
#include "hook_cases.hpp"

using namespace shapes;

int main() {
    run_case<Batch8>("Batch8", 0x5203u);
    run_case<FatOn>("FatOn", 0x5204u);
    return finish("shape_test_h");
}

// Hooks, hints and tunings of the template sweep, part e: the hooks: a canary for the check-free code, interior() with
// a rim check, at_level, the column hint against the check-free promise (hook_cases.hpp; run by
// tests/test_template_hooks_gpu.py).
#include "hook_cases.hpp"

using namespace shapes;

int main() {
    run_canary(0x5001u);
    run_case<Rim>("Rim", 0x5002u);
    run_case<Levels>("Levels", 0x5003u);
    run_case<OneWayRim>("OneWayRim", 0x5004u);
    return finish("shape_test_e");
}

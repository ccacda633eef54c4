// Hooks, hints and tunings of the template sweep, part i: the function object's state: none, seven bytes, a double and
// two words, nine words (hook_cases.hpp; run by tests/test_template_hooks_gpu.py).
#include "hook_cases.hpp"

using namespace shapes;

int main() {
    run_case<Stateless>("Stateless", 0x5005u);
    run_case<State7>("State7", 0x5302u);
    run_case<State16>("State16", 0x5303u);
    run_case<State36>("State36", 0x5304u);
    return finish("shape_test_i");
}

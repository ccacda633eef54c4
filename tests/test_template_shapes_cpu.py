"""The reference of the shape coverage (tests/cpp_shapes): stencil::cpu::StencilUpdate on every functor of
shape_cases.hpp and hook_cases.hpp equals a plain double loop over two arrays that substitutes the halo, steps through sub-iterations
and generations and evaluates the time-dependent value by hand -- on a 1 x 1 grid, a single row and a small grid per
functor.  Host-only (g++); tests/test_template_shapes_gpu.py compares the HIP sweeps with this cpu backend."""
import os
import subprocess

from conftest import ROOT

OUT = os.path.join(ROOT, "build", "tests")
FUNCTORS = ["U16", "Quad1", "Tri1", "F3", "D1", "Octo1", "Penta1", "Mixed2", "F2x2", "F3x1", "D2x1"]
# tests/cpp_shapes/hook_cases.hpp: the hooks, the one-way read policy, the copied constant field, the explicit tunings'
# functors and the function objects with state of their own
FUNCTORS += ["Canary", "Rim", "Levels", "OneWayRim", "OneWay", "OneWayPlanes", "Liar", "Lone8", "Twelve", "Batch8", "FatOn",
             "Stateless", "State7", "State16", "State36", "State40", "StateTable"]


def test_cpu_backend_equals_a_plain_loop_on_every_shape_functor():
    binary = os.path.join(OUT, "shape_host_test")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp_shapes"), binary])
    res = subprocess.run([binary], capture_output=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="4"))
    text = (res.stdout + res.stderr).decode()
    assert res.returncode == 0, text[-3000:]
    assert "shape_host_test:" in text and " 0 failures" in text, text[-3000:]
    for name in FUNCTORS:
        assert f"reference {name}:" in text, f"no report line for {name}\n" + text[-3000:]

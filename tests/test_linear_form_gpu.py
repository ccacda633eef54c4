"""Declared linear five-point functors (include/StencilStream/hip/LinearForm.hpp): a functor that declares
stencil::hip::LinearCross5 and passes the device-side probe is swept by the product-carrying form of the five-point
Jacobi where its coefficients and halo allow it, with the cpu backend's cells bit for bit; everything else runs the
general sweep as before.  Drives tests/cpp_forms/linear_form_test.hip (plain, -ffp-contract=fast and
-fgpu-flush-denormals-to-zero builds) and the reference's unchanged Jacobi example."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

OUT = os.path.join(ROOT, "build", "tests")
EX = os.path.join(ROOT, "build", "examples")
# small grids take the one-cell-per-lane kernels unless told otherwise (STSTHIP_NARROW_FORM_KCELLS, default 6000)
WIDE = {"STSTHIP_NARROW_FORM_KCELLS": "0"}


def binary(name):
    path = os.path.join(OUT, name)
    if not os.path.exists(path):
        pytest.fail(f"build/tests/{name} missing: run __graft_entry__.build()")
    return path


def example(name):
    path = os.path.join(EX, name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not built (needs the reference tree; run `make -C examples`)")
    return path


def run(cmd, **env):
    env = dict({k: v for k, v in os.environ.items() if k not in ("STSTHIP_LINEAR_FORM", "STSTHIP_TRACE_FORM")},
               OMP_NUM_THREADS="4", **env)
    res = subprocess.run(cmd, capture_output=True, env=env, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr).decode()[-3000:]
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, WIDE], ids=["narrow-lanes", "four-cells-per-lane"])
def test_forms_and_cells_of_every_case(env):
    """Every case of the plain build: UserCross5 with 0.2 x 5 and a +0 halo runs jacobi5_uniform on 300 x 700,
    130 x 257, 3 x 5 and 1 x 1 for 1, 2, 16, 17 and 37 generations (only / first / middle / last launch kernels), on
    data in [0, 1) and of both signs, and for 17 and 37 generations on data around the subnormal threshold and on data
    with planted NaN, +-inf, subnormal and -0.0 cells (there: NaNs in the same cells, all other cells equal); distinct or negative coefficients, other halos, a functor that lies about its
    form, a clamped one and an undeclared one run general; resuming at generation 20 and changing the parameters
    through get_params() follow.  All cells equal stencil::cpu::StencilUpdate on the same functor."""
    res = run([binary("linear_form_test")], **env)
    assert b"linear_form_test:" in res.stdout and b" 0 failures" in res.stdout, (res.stdout + res.stderr).decode()[-3000:]


@pytest.mark.gpu
def test_knob_keeps_the_general_sweep_and_the_trace_names_the_form():
    routed = run([binary("linear_form_test"), "knob"], STSTHIP_TRACE_FORM="1")
    assert b"form: jacobi5_uniform" in routed.stdout
    assert b"sweep form: jacobi5_uniform" in routed.stderr
    kept = run([binary("linear_form_test"), "knob"], STSTHIP_LINEAR_FORM="0", STSTHIP_TRACE_FORM="1")
    assert b"form: general" in kept.stdout
    assert b"sweep form: general (STSTHIP_LINEAR_FORM=0)" in kept.stderr
    quiet = run([binary("linear_form_test"), "knob"])
    assert b"sweep form" not in quiet.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, WIDE], ids=["narrow-lanes", "four-cells-per-lane"])
def test_contracted_build_is_never_changed_by_the_route(tmp_path, env):
    """linear_form_test_fma (-ffp-contract=fast): its cells with and without STSTHIP_LINEAR_FORM=0 are the same bits
    whichever form it reports; a build that reports the uniform form must also give the plain build's cells."""
    routed, kept, plain = tmp_path / "routed.bin", tmp_path / "kept.bin", tmp_path / "plain.bin"
    res = run([binary("linear_form_test_fma"), "dump", str(routed)], **env)
    run([binary("linear_form_test_fma"), "dump", str(kept)], STSTHIP_LINEAR_FORM="0", **env)
    got, want = np.fromfile(routed, dtype=np.uint32), np.fromfile(kept, dtype=np.uint32)
    assert got.size == 300 * 700 and np.array_equal(got, want)
    assert b"form: " in res.stdout
    if b"form: jacobi5_uniform" in res.stdout:
        run([binary("linear_form_test"), "dump", str(plain)], **env)
        assert np.array_equal(got, np.fromfile(plain, dtype=np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, WIDE], ids=["narrow-lanes", "four-cells-per-lane"])
def test_flushing_build_is_never_changed_by_the_route(tmp_path, env):
    """linear_form_test_ftz (-fgpu-flush-denormals-to-zero: its kernels flush fp32 subnormals, the library's keep them)
    on data around the subnormal threshold: its cells with and without STSTHIP_LINEAR_FORM=0 are the same bits
    whichever form it reports, and the trace names the reason; a build that reports the uniform form must also give
    the plain build's cells.  Its `all` mode is not run: the cpu backend does not flush."""
    routed, kept, plain = tmp_path / "routed.bin", tmp_path / "kept.bin", tmp_path / "plain.bin"
    res = run([binary("linear_form_test_ftz"), "dump-tiny", str(routed)], STSTHIP_TRACE_FORM="1", **env)
    run([binary("linear_form_test_ftz"), "dump-tiny", str(kept)], STSTHIP_LINEAR_FORM="0", **env)
    run([binary("linear_form_test"), "dump-tiny", str(plain)], **env)
    got, want = np.fromfile(routed, dtype=np.uint32), np.fromfile(kept, dtype=np.uint32)
    unflushed = np.fromfile(plain, dtype=np.uint32)
    # the data is telling: a third of the plain build's cells are subnormal, a flushing kernel cannot return them
    subnormal = ((unflushed & 0x7F800000) == 0) & ((unflushed & 0x007FFFFF) != 0)
    print(f"subnormal cells of the plain build: {subnormal.mean():.3f}; {res.stdout.decode().strip()}; "
          f"routed and kept differ in {(got != want).sum()} cells")
    assert unflushed.size == 300 * 700 and subnormal.mean() >= 0.1
    assert got.size == 300 * 700 and np.array_equal(got, want)
    assert b"form: " in res.stdout
    if b"form: jacobi5_uniform" in res.stdout:
        assert np.array_equal(got, unflushed)
    else:
        assert b"sweep form: general (this build flushes fp32 subnormals)" in res.stderr, res.stderr.decode()[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("coef,form", [(["0.2"] * 5, b"sweep form: jacobi5_uniform"),
                                       (["0.2", "0.21", "0.19", "0.22", "0.18"], b"sweep form: general")],
                         ids=["uniform", "distinct"])
def test_unchanged_example_is_routed(tmp_path, oracle, coef, form):
    """The reference's examples/jacobi, source untouched (examples/reference_linear_forms.hpp declares its functor)."""
    H, W, its = 300, 700, 37
    out_file = tmp_path / "out.bin"
    res = run([example("jacobi_Jacobi5General_hip"), str(H), str(W), str(its), str(out_file)] + coef,
              STSTHIP_TRACE_FORM="1")
    assert form in res.stderr, res.stderr.decode()[-2000:]
    got = np.fromfile(out_file, dtype=np.float32).reshape(H, W)
    want = oracle.jacobi("Jacobi5General", [float(c) for c in coef], oracle.jacobi_init(H, W), its, halo=0.0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_unchanged_example_built_with_contraction_is_not_changed(tmp_path):
    H, W, its = 300, 700, 37
    outs = []
    for i, env in enumerate(({}, {"STSTHIP_LINEAR_FORM": "0"})):
        out_file = tmp_path / f"out{i}.bin"
        run([example("jacobi_Jacobi5General_hip_fma"), str(H), str(W), str(its), str(out_file)] + ["0.2"] * 5, **env)
        outs.append(np.fromfile(out_file, dtype=np.uint32))
    assert outs[0].size == H * W and np.array_equal(outs[0], outs[1])

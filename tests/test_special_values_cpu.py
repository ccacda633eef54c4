"""The oracle on subnormal, non-finite and signed-zero cells, without a GPU: pinned against a step-by-step numpy float32
evaluation of the same expressions, and the content conditions that keep the cases of test_special_values_gpu.py from
being vacuous, checked on the oracle's result of every one of them."""
import dataclasses

import numpy as np
import pytest

import special_values as sv
from test_special_values_gpu import CASES, dynamic_fields, reference

F = np.float32


def numpy_jacobi(variant, coef, grid, n, halo):
    """`n` generations in numpy float32, every operation rounded on its own, in the reference's operand order:
    (((c0*N + c1*W) + c2*S) + c3*E) + c4*C."""
    c = [F(v) for v in coef]
    grid = grid.astype(F)
    with np.errstate(all="ignore"):
        for _ in range(n):
            p = np.pad(grid, 1, constant_values=F(halo))
            N, W, S, E, C = p[:-2, 1:-1], p[1:-1, :-2], p[2:, 1:-1], p[1:-1, 2:], p[1:-1, 1:-1]
            if variant == "Jacobi5General":
                grid = (((c[0] * N + c[1] * W) + c[2] * S) + c[3] * E) + c[4] * C
            elif variant == "Jacobi5Constant":
                grid = ((((N + W) + S) + E) + C) * F(0.2)
            else:  # Jacobi9General: rows, then columns, from 0.0f
                grid = np.zeros_like(grid)
                for r in range(3):
                    for k in range(3):
                        grid = grid + c[r * 3 + k] * p[r:r + grid.shape[0], k:k + grid.shape[1]]
            assert grid.dtype == F
    return grid


PINNED = [("Jacobi5General", (0.11, 0.19, 0.23, 0.31, 0.16)), ("Jacobi5General", (0.47, -0.43, 0.51, 0.39, -0.44)),
          ("Jacobi5General", (0.3,) * 5), ("Jacobi5General", (0.9, 0.91, 0.89, 0.92, 0.88)), ("Jacobi5Constant", ()),
          ("Jacobi9General", (0.05, 0.1, 0.07, 0.12, 0.2, 0.13, 0.08, 0.14, 0.11)),
          ("Jacobi9General", (0.31, -0.37, 0.29, -0.33, 0.36, 0.3, -0.28, 0.35, -0.34))]


@pytest.mark.parametrize("variant,coef", PINNED, ids=lambda v: v if isinstance(v, str) else f"c{v[0]}x{len(v)}" if v else "-")
@pytest.mark.parametrize("data", ["tiny", "huge", "planted", "negzero"])
def test_oracle_equals_numpy_step_by_step(oracle, data, variant, coef):
    """70 x 300 with a planted seam at column 224; tiny and huge data to 17 generations, planted data to 8 (after that
    most of the grid is NaN)."""
    shape = (70, 300)
    grid = sv.planted(shape, 7, 224) if data == "planted" else getattr(sv, data)(shape, 7)
    for halo in (0.0, -0.0, 0.25):
        for n in (1, 3, 8) if data in ("planted", "negzero") else (1, 3, 8, 17):
            want = numpy_jacobi(variant, coef, grid, n, halo)
            got = oracle.jacobi(variant, coef, grid, n, halo=halo, n_threads=4)
            sv.assert_same_cells(got, want, f"{variant} {data} halo {halo} n={n}")


def test_generators_and_classify():
    shape = (130, 257)
    t, h, z = sv.classify(sv.tiny(shape, 1)), sv.classify(sv.huge(shape, 1)), sv.classify(sv.negzero(shape))
    assert t["subnormal"] > 0.5 and t["normal"] > 0.1 and t["inf"] == t["nan"] == 0
    assert h["normal"] == 1.0 and np.abs(sv.huge(shape, 1)).min() >= 2.0 ** 120
    assert z["zero"] == z["negzero"] == 1.0
    assert np.array_equal(sv.tiny(shape, 1).view(np.uint32), sv.tiny(shape, 1).view(np.uint32))  # seeded
    for double in (sv.tiny(shape, 1, np.float64), sv.huge(shape, 1, np.float64)):
        assert double.dtype == np.float64
    assert sv.classify(sv.tiny(shape, 1, np.float64))["subnormal"] > 0.5
    # planted: every kind is there, at the corners, the rims, beside column 64 and on both sides of every seam
    for shape, strips in (((3, 5), 0), ((130, 257), 224), ((300, 700), 224), ((300, 700), 0)):
        sites = sv.planted_sites(shape, strips)
        grid = sv.planted(shape, 3, strips)
        H, W = shape
        assert np.isnan(grid[0, 0]) and grid[H - 1, W - 2] == np.inf and grid[H - 1, W - 1] == -np.inf
        assert all(sites[kind] for kind in ("nan", "+inf", "subnormal", "-0"))
        share = sv.classify(grid)
        assert share["nan"] > 0 and share["inf"] > 0 and share["subnormal"] > 0 and share["negzero"] > 0
        assert share["normal"] > 0.5
        special = ~(np.isfinite(grid) & (np.abs(grid) >= np.finfo(F).tiny))
        assert special[0].any() and special[-1].any() and special[:, 0].any() and special[:, -1].any()
        if strips and W > strips:
            for seam in range(strips, W, strips):
                assert special[:, seam - 1].any() and special[:, seam].any(), seam
        if W > 65:
            assert special[:, 63].any() and special[:, 64].any() and special[:, 65].any()


def test_the_comparison_rule():
    a = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1e-45], dtype=F)
    assert not sv.differing(a, a.copy()).any()
    other_nan = a.copy()
    other_nan.view(np.uint32)[4] = 0xFFC00001  # sign and payload of a NaN are left out
    assert not sv.differing(other_nan, a).any()
    for i, v in ((0, -0.0), (1, 0.0), (2, -np.inf), (4, 1.0), (5, np.nan), (5, np.nextafter(F(1), F(2))), (6, 0.0)):
        b = a.copy()
        b[i] = v
        assert sv.differing(b, a).sum() == 1 and sv.differing(b, a)[i], (i, v)
        with pytest.raises(AssertionError):
            sv.assert_same_cells(b, a)
    cells = np.zeros((2, 2), dtype=[("temp", "<f8"), ("power", "<f8")])
    flipped = cells.copy()
    flipped["power"][1, 0] = -0.0
    assert sv.differing(flipped, cells).sum() == 1


SHARED = list({dataclasses.replace(c, fastpath="", variant=c.variant if c.app == "jacobi" else ""): c for c in CASES}.values())


@pytest.mark.parametrize("case", SHARED, ids=lambda c: c.id)
def test_content_conditions(oracle, built_lib, case):
    """On the oracle's result of every case of the GPU test: the class the case is named for covers at least 1 % of the
    cells, NaNs at most half, and at least 10 % are finite and not zero (except on negzero data)."""
    _, want = reference(oracle, case)
    share = sv.classify(dynamic_fields(case, want))
    print(case.id, {k: round(float(v), 4) for k, v in share.items()})
    assert share[case.named] >= 0.01, share
    assert share["nan"] <= 0.5, share
    if case.data != "negzero":
        assert share["subnormal"] + share["normal"] >= 0.10, share
    else:
        assert share["zero"] == 1.0, share

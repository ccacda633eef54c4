"""The row form of the uniform Jacobi kernel in EDGE waves (Sweep.hpp: row form, edge waves; lane order c0 c2 c1 c3 in
the edge code's loads, halo fill and stores), through ststhip_app_run("jacobi5general") with five equal coefficients
and a +0 halo, in the wide shape (STSTHIP_NARROW_FORM_KCELLS=0), row chunks of sixteen rows, no taper.

Shapes, the smallest at which each piece can go wrong (K = 4 cells per lane, strips of OW = 224 output columns and a
column halo of GX = 16 at sixteen generations):
  widths   1, 3, 5      the grid's edge inside one lane, in every position within the lane
           63           partial lanes
           223 224 225  around one strip's output: a ragged last strip, the per-cell stores
           463          = 2 OW + GX - 1: strip 1 just misses being check-free
           701          check-free and edge units side by side in one launch
  heights  1, 3, 17     every unit is at the grid's first AND last rows
           71           top, middle and bottom chunks (units whose columns all lie inside take the select-free code)
  generations 1, 2, 16 (the only launch of their call), 31 = 16 + 8 + 4 + 2 + 1 (every depth as first, middle and last
           launch), 48 (a middle launch of full depth)
as a pairwise cover of widths x heights x generations (every pair of values of two of the three occurs), with 701 x 71
and 5 x 3 at every generation count.  Data: random, distinct from cell to cell, so a swapped pair of cells shows; and a
grid of special values -- +inf beside -inf in row 0 and in the last column, a NaN in a corner, runs of -0.0 down
column 0 and along the last row, subnormals on the rim, values around the subnormal threshold elsewhere: what a cell
outside the grid computes from these must never come back into the grid.

Every result is compared bit for bit (NaNs by position, tests/special_values.py) with the CPU oracle and with the
general kernel (STSTHIP_JACOBI_FASTPATH=0)."""
import functools

import numpy as np
import pytest

import special_values as sv

WIDTHS = (1, 3, 5, 63, 223, 224, 225, 463, 701)
HEIGHTS = (1, 3, 17, 71)
GENERATIONS = (1, 2, 16, 31, 48)
CHUNK = 16
COEF = (0.2,) * 5
ENV = {"STSTHIP_NARROW_FORM_KCELLS": "0", "STSTHIP_CHUNK_ROWS": str(CHUNK), "STSTHIP_TAPER": ""}
OTHER_KNOBS = ("STSTHIP_LAST_CHUNK_EARLY", "STSTHIP_XCD_REMAP", "STSTHIP_TAIL_PERMILLE", "STSTHIP_NARROW_BAND_ROWS",
               "STSTHIP_MAX_GENERATIONS", "STSTHIP_VIRTUAL_STRIPS")


def cover():
    """(width, height, generations): every width with every generation count, the height shifted by one from pair to
    pair; then the two shapes the issue names at every generation count."""
    cases = []
    for i, w in enumerate(WIDTHS):
        for j, n in enumerate(GENERATIONS):
            cases.append((w, HEIGHTS[(i + j) % len(HEIGHTS)], n))
    for n in GENERATIONS:
        for w, h in ((701, 71), (5, 3)):
            if (w, h, n) not in cases:
                cases.append((w, h, n))
    return cases


CASES = cover()


def test_the_cover_is_pairwise():
    for a, b, xs, ys in ((0, 1, WIDTHS, HEIGHTS), (0, 2, WIDTHS, GENERATIONS), (1, 2, HEIGHTS, GENERATIONS)):
        assert {(c[a], c[b]) for c in CASES} == {(x, y) for x in xs for y in ys}
    for n in GENERATIONS:
        assert (701, 71, n) in CASES and (5, 3, n) in CASES


def random_grid(h, w):
    grid = np.random.default_rng(0xed6e0000 + 1000 * h + w).random((h, w), dtype=np.float32)
    assert np.unique(grid).size > 0.99 * grid.size
    return grid


def special_grid(h, w):
    """Around the subnormal threshold everywhere; -0.0 down column 0 and along the last row; subnormals of a few units on
    every third cell of the rest of the rim; +inf with -inf to its right in row 0 and ending in the last column, +inf
    above -inf in the last column; a NaN in the first row's last corner.  On a grid too small for all of them the later
    ones win."""
    grid = sv.tiny((h, w), 0x7e57 + 1000 * h + w)
    least = np.finfo(np.float32).smallest_subnormal
    grid[:, 0] = -0.0
    grid[h - 1, :] = -0.0
    rim = [(0, c) for c in range(1, w)] + [(r, w - 1) for r in range(1, h - 1)]
    for i, (r, c) in enumerate(rim[1::3]):
        grid[r, c] = (-1) ** i * least * (1 + 37 * i)
    if w >= 6:
        grid[0, w // 2], grid[0, w // 2 + 1] = np.inf, -np.inf
    if h >= 6 and w >= 2:
        grid[h // 3, w - 2], grid[h // 3, w - 1] = np.inf, -np.inf
        grid[2 * h // 3, w - 1], grid[2 * h // 3 + 1, w - 1] = np.inf, -np.inf
    elif w >= 3:
        grid[0, w - 3], grid[0, w - 2] = np.inf, -np.inf
    grid[0, w - 1] = np.nan
    return grid


GRIDS = {"random": random_grid, "special": special_grid}


@functools.lru_cache(maxsize=None)
def start_and_oracle(oracle, data, h, w, n):
    grid = GRIDS[data](h, w)
    return grid, oracle.jacobi("Jacobi5General", COEF, grid, n, halo=0.0, n_threads=8)


def run(grid, n, fastpath, monkeypatch):
    import torch

    from stencilstream_amd import capi

    h, w = grid.shape
    for knob in OTHER_KNOBS:
        monkeypatch.delenv(knob, raising=False)
    for knob, value in ENV.items():
        monkeypatch.setenv(knob, value)
    if fastpath:
        monkeypatch.delenv("STSTHIP_JACOBI_FASTPATH", raising=False)
    else:
        monkeypatch.setenv("STSTHIP_JACOBI_FASTPATH", "0")
    capi.reload_options()
    o = capi.options()
    assert o.chunk_rows == CHUNK and o.n_taper == 0 and o.narrow_form_kcells == 0 and o.jacobi_fastpath == int(fastpath)
    params = capi.JacobiParams()
    for i, c in enumerate(COEF):
        params.coef[i] = c
    src = torch.from_numpy(grid).cuda()
    dst = torch.full_like(src, 12345.0)
    torch.cuda.synchronize()  # (the library's stream is not ordered with torch's copies above)
    info = capi.app_run("jacobi5general", params, np.float32(0).tobytes(), capi.Domain(h, w, 0, h, w),
                        [src.data_ptr()], [dst.data_ptr()], 0, n, blocking=True)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), info


def depths_of(n, deepest):
    out = []
    while n:
        t = deepest
        while t > n:
            t //= 2
        out.append(t)
        n -= t
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,n", CASES)
@pytest.mark.parametrize("data", ["random", "special"])
def test_edge_waves_equal_the_oracle_and_the_general_kernel(gpu, oracle, monkeypatch, data, w, h, n):
    from stencilstream_amd import capi

    info = capi.app_info("jacobi5uniform")
    assert info.cells_per_lane == 4 and info.max_generations == 16
    grid, want = start_and_oracle(oracle, data, h, w, n)
    if data == "special":
        print(f"{data} {h} x {w}, n={n}, oracle:", {k: round(float(v), 4) for k, v in sv.classify(want).items()})
        if (w, h) == (701, 71):
            start = sv.classify(grid)
            assert start["subnormal"] > 0.1 and start["nan"] > 0 and start["inf"] > 0 and start["negzero"] > 0
            assert sv.classify(want)["nan"] > 0
    got, ran = run(grid, n, True, monkeypatch)
    assert ran.n_launches == len(depths_of(n, int(info.max_generations))), ran.n_launches
    what = f"{data}, {h} x {w}, {n} generations"
    sv.assert_same_cells(got, want, f"{what}, uniform kernel against the oracle")
    general, _ = run(grid, n, False, monkeypatch)
    sv.assert_same_cells(general, want, f"{what}, general kernel against the oracle")
    sv.assert_same_cells(got, general, f"{what}, uniform against general kernel")

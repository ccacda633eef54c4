"""The packed row form of the uniform Jacobi kernel on the GPU (Sweep.hpp: row form, lane order c0 c2 c1 c3;
forms/Jacobi5Uniform.hpp: row_at_level), through ststhip_app_run("jacobi5general") with five equal coefficients and a
+0 halo.

Only check-free waves with four cells per lane run the row form, so the grid and the plan are chosen to have some at
every depth: 64 x 701 with STSTHIP_NARROW_FORM_KCELLS=0 (the wide shape), STSTHIP_CHUNK_ROWS=16 and no taper -- four
chunks of 16 rows, of which rows 16-48 keep a launch's depth away from the grid's first and last row, and column
strips of which strip 1 (at 16 generations strip 2 as well) lies inside the grid with its whole footprint.
`check_free_units` restates Sweep::entry's condition; the test asserts that every depth it runs has such units, and
the planted cells of the second case lie inside them at every depth.

Generations 1, 2 and 16 are the only launch of their call; 31 = 16 + 8 + 4 + 2 + 1 runs every depth as first, middle
and last launch; 48 has a middle launch of full depth.  Every result is compared with the CPU oracle bit for bit (NaNs
by position, tests/special_values.py) and with the general kernel (STSTHIP_JACOBI_FASTPATH=0).  Random data differs
from cell to cell, so a pair of cells swapped on the way in or out shows.  The second case is where a denormal mode
that differed between packed and plain instructions would show: data around the subnormal threshold everywhere (the
coefficients sum to 1: it stays there through every level), with -0, subnormals, +inf beside -inf and a NaN planted."""
import functools

import numpy as np
import pytest

import special_values as sv

H, W = 64, 701
CHUNK = 16
COEF = (0.2,) * 5
GENERATIONS = (1, 2, 16, 31, 48)
ENV = {"STSTHIP_NARROW_FORM_KCELLS": "0", "STSTHIP_CHUNK_ROWS": str(CHUNK), "STSTHIP_TAPER": ""}
OTHER_KNOBS = ("STSTHIP_LAST_CHUNK_EARLY", "STSTHIP_XCD_REMAP", "STSTHIP_TAIL_PERMILLE", "STSTHIP_NARROW_BAND_ROWS",
               "STSTHIP_MAX_GENERATIONS", "STSTHIP_VIRTUAL_STRIPS")
PLANT_ROWS, PLANT_COLS = (20, 44), (300, 320)


def depths_of(n, deepest):
    """The launches of a call of n generations: the deepest compiled depth that still fits, again and again."""
    out = []
    while n:
        t = deepest
        while t > n:
            t //= 2
        out.append(t)
        n -= t
    return out


def check_free_units(depth, cells_per_lane):
    """Sweep::entry's condition for a launch of the whole grid at `depth`: [(strip, chunk, output columns, output
    rows)] of the units whose footprint -- 64 lanes of columns, the chunk's rows and `depth` more on either side --
    lies inside the grid."""
    k = cells_per_lane
    gx = -(-depth // k) * k  # the column halo in whole lanes
    lw = 64 * k
    ow = lw - 2 * gx
    units = []
    for strip in range(-(-W // ow)):
        xw0 = strip * ow - gx
        if not (xw0 > 0 and xw0 + lw <= W and xw0 + lw - gx <= W):
            continue
        for chunk in range(-(-H // CHUNK)):
            ya, yb = chunk * CHUNK, min((chunk + 1) * CHUNK, H)
            if ya - depth >= 0 and yb + depth <= H:
                units.append((strip, chunk, (strip * ow, min((strip + 1) * ow, W)), (ya, yb)))
    return units


def random_grid():
    grid = np.random.default_rng(0x9ac4ed).random((H, W), dtype=np.float32)
    assert np.unique(grid).size > 0.99 * grid.size
    return grid


def special_grid():
    """Values around the subnormal threshold of both signs everywhere; inside rows 20-44, columns 300-320: a run of
    -0, subnormals of a few units, +inf with -inf to its right (a NaN after one generation) and a NaN."""
    grid = sv.tiny((H, W), 0x7e57)
    least = np.finfo(np.float32).smallest_subnormal
    grid[22, 301:312] = -0.0
    grid[23:30, 304] = -0.0
    for i, (r, c) in enumerate([(26, 308), (26, 309), (27, 308), (31, 317), (43, 300), (20, 319)]):
        grid[r, c] = (-1) ** i * least * (1 + 37 * i)
    grid[40, 315], grid[40, 316] = np.inf, -np.inf
    grid[36, 318] = np.nan
    return grid


GRIDS = {"random": random_grid, "special": special_grid}


@functools.lru_cache(maxsize=None)
def start_and_oracle(oracle, data, n):
    grid = GRIDS[data]()
    return grid, oracle.jacobi("Jacobi5General", COEF, grid, n, halo=0.0, n_threads=8)


def run(grid, n, fastpath, monkeypatch):
    import torch

    from stencilstream_amd import capi

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
    info = capi.app_run("jacobi5general", params, np.float32(0).tobytes(), capi.Domain(H, W, 0, H, W),
                        [src.data_ptr()], [dst.data_ptr()], 0, n, blocking=True)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), info


@pytest.mark.gpu
@pytest.mark.parametrize("n", GENERATIONS)
@pytest.mark.parametrize("data", ["random", "special"])
def test_check_free_waves_equal_the_oracle_and_the_general_kernel(gpu, oracle, monkeypatch, data, n):
    from stencilstream_amd import capi

    info = capi.app_info("jacobi5uniform")
    assert info.cells_per_lane == 4 and info.max_generations == 16
    depths = depths_of(n, int(info.max_generations))
    for depth in set(depths):
        units = check_free_units(depth, int(info.cells_per_lane))
        assert units, f"no check-free unit at depth {depth}"
        # the planted cells lie in columns and rows that check-free units produce
        assert any(cols[0] <= PLANT_COLS[0] and PLANT_COLS[1] < cols[1] for _, _, cols, _ in units), (depth, units)
        assert min(rows[0] for *_, rows in units) <= PLANT_ROWS[0] and PLANT_ROWS[1] <= max(rows[1] for *_, rows in units)
    assert set(depths_of(31, 16)) == {16, 8, 4, 2, 1}

    grid, want = start_and_oracle(oracle, data, n)
    if data == "special":
        shares = sv.classify(want)
        print(f"{data} n={n} oracle:", {k: round(float(v), 4) for k, v in shares.items()})
        assert shares["subnormal"] > 0.1 and shares["nan"] > 0
    got, ran = run(grid, n, True, monkeypatch)
    assert ran.n_launches == len(depths), (ran.n_launches, depths)
    sv.assert_same_cells(got, want, f"{data}, {n} generations, uniform kernel against the oracle")
    general, _ = run(grid, n, False, monkeypatch)
    sv.assert_same_cells(general, want, f"{data}, {n} generations, general kernel against the oracle")
    sv.assert_same_cells(got, general, f"{data}, {n} generations, uniform against general kernel")

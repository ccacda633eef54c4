"""The precompiled transition functions that had never met a neighbour, through the strip and block drivers
(ststhip_strip_*, ststhip_block_*) on chains of 3 strips and meshes of 2 x 2 and 3 x 3 blocks, against the oracle on
the whole grid, bit for bit.  The ranks are threads of this process (mesh_threads.py): one process on the GPU, a
mailbox with bounded waits.

The extents follow the shape of each function as ststhip_app_info describes it (D generations per launch, hpg halo
cells per generation, g = D * hpg, OW columns per strip of the sweep, m launches per ghost exchange, set through
STSTHIP_EXCHANGE_EVERY): per cut axis of n ranks E = max(2 g, OW) + 1 (m = 1; 4 g m for a larger m, so that the
driver keeps it) and n * E + (n - 1) in all -- the earlier ranks own one more than the last, the sweep's column
seams fall inside the blocks; an axis that is not cut has OW + 1 columns.  Generations: m * D + 1 (a full group whose
last launch feeds the exchange, and one launch more), then 2 * m * D + 3 in a second call, from an iteration offset."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def shape_of(app, m):
    """(D, g, OW) of a registered function and the two generation counts of a run at m launches per exchange"""
    from stencilstream_amd import capi

    info = capi.app_info(app)
    D = info.default_generations if 0 < info.default_generations < info.max_generations else info.max_generations
    g = D * info.halo_depth_per_generation
    return D, g, max(int(info.strip_width), 1), (m * D + 1, 2 * m * D + 3)


def extents(app, m, n_rows, n_cols):
    """the grid for n_rows x n_cols ranks (a chain of strips: n_cols = 1)"""
    _D, g, OW, _n = shape_of(app, m)
    E = max(2 * g if m == 1 else 4 * g * m, OW) + 1
    return (n_rows * E + (n_rows - 1) if n_rows > 1 else 2 * g + 1,
            n_cols * E + (n_cols - 1) if n_cols > 1 else OW + 1)


def decomposed(app, params, halo, cells, offset, m, decomposition, monkeypatch):
    """two advance calls from `offset`; returns the assembled grid and the generations it has run"""
    from stencilstream_amd import capi

    from mesh_threads import run_decomposed

    monkeypatch.setenv("STSTHIP_EXCHANGE_EVERY", str(m))
    capi.init(0)
    n1, n2 = shape_of(app, m)[3]
    kwargs = {"n_strips": decomposition} if isinstance(decomposition, int) else {"mesh": decomposition}
    got, counters = run_decomposed(app, params, halo, cells, [(offset, n1), (offset + n1, n2)], **kwargs)
    for launches, exchanges in counters:
        # one exchange per group of m launches: at least m + 1 launches in the first call and 2 m + 1 in the second
        # are 2 + 3 exchanges; a run at a larger interval than meant would make fewer
        assert launches >= 3 * m + 2 and exchanges >= 5, (launches, exchanges)
    return got, n1 + n2


def ranks_of(decomposition):
    return (decomposition, 1) if isinstance(decomposition, int) else decomposition


DECOMPOSITIONS = {"strips3": 3, "mesh2x2": (2, 2), "mesh3x3": (3, 3)}


@pytest.mark.parametrize("decomposition", ["strips3", "mesh2x2", "mesh3x3"])
def test_jacobi25_radius2_with_neighbours(gpu, oracle, monkeypatch, decomposition):
    from stencilstream_amd import capi

    d = DECOMPOSITIONS[decomposition]
    H, W = extents("jacobi25general", 1, *ranks_of(d))
    rng = np.random.default_rng(2525)
    grid = rng.random((H, W), dtype=np.float32)
    coef = (rng.random(25, dtype=np.float32) / 12).astype(np.float32)
    p = capi.Jacobi25Params()
    for i in range(25):
        p.coef[i] = float(coef[i])
    got, n = decomposed("jacobi25general", p, np.float32(0.25).tobytes(), grid, 5, 1, d, monkeypatch)
    want = oracle.jacobi25(coef, grid, n, halo=0.25, n_threads=8)
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(got), bits(grid))


@pytest.mark.parametrize("offset", [0, 32])
@pytest.mark.parametrize("decomposition", ["strips3", "mesh2x2"])
@pytest.mark.parametrize("app,radius", [("selfcheck1", 1), ("selfcheck1_soa", 1), ("selfcheck2", 2)])
def test_selfcheck_with_neighbours(gpu, oracle, monkeypatch, app, radius, decomposition, offset):
    """The transition function verifies the global coordinates, the iteration, the sub-iteration and the
    time-dependent value of everything it sees: what a decomposition can get wrong."""
    from stencilstream_amd import capi

    d = DECOMPOSITIONS[decomposition]
    H, W = extents(app, 1, *ranks_of(d))
    halo = np.zeros((), dtype=oracle.SELFCHECK_CELL)
    halo["status"] = 2
    cells = oracle.selfcheck_input(H, W, offset)
    out, n = decomposed(app, capi.NoParams(), halo.tobytes(), cells, offset, 1, d, monkeypatch)
    assert (out["status"] == 0).all(), "a cell saw a wrong neighbour, index or TDV"
    assert (out["r"] == np.arange(H)[:, None]).all() and (out["c"] == np.arange(W)[None, :]).all()
    assert (out["i_iteration"] == offset + n).all() and (out["i_subiteration"] == 0).all()
    assert np.array_equal(bits(out), bits(oracle.selfcheck(radius, cells, offset, n)))


@pytest.mark.parametrize("app", ["hotspot_aos", "hotspot_f64", "hotspot_f64_aos"])
def test_hotspot_layouts_on_a_mesh(gpu, oracle, monkeypatch, app):
    from stencilstream_amd import capi

    H, W = extents(app, 1, 2, 2)
    rng = np.random.default_rng(640)
    p32 = oracle.hotspot_params(H, W)
    vals = [float(p32.Rx_1), float(p32.Ry_1), float(p32.Rz_1), float(p32.Cap_1)]
    if "f64" in app:
        cells = np.zeros((H, W), dtype=oracle.HOTSPOT_CELL_F64)
        cells["temp"] = 320 + 10 * rng.random((H, W))
        cells["power"] = rng.random((H, W)) * 0.01
        got, n = decomposed(app, capi.HotspotParamsF64(*vals), bytes(16), cells, 5, 1, (2, 2), monkeypatch)
        want = oracle.hotspot_f64(oracle.HotspotParamsF64(*vals), cells, n, n_threads=8)
    else:
        cells = np.zeros((H, W), dtype=oracle.HOTSPOT_CELL)
        cells["temp"] = 320 + 10 * rng.random((H, W), dtype=np.float32)
        cells["power"] = rng.random((H, W), dtype=np.float32) * 0.01
        got, n = decomposed(app, capi.HotspotParams(*vals), bytes(8), cells, 5, 1, (2, 2), monkeypatch)
        want = oracle.hotspot(p32, cells, n, n_threads=8)
    assert np.array_equal(bits(got), bits(want))
    assert np.abs(want["temp"] - cells["temp"]).max() > 0


@pytest.mark.parametrize("app,decomposition,m",
                         [(app, "strips3", m) for app in ("fdtd_coef", "fdtd_coef_aos", "fdtd_coef_grouped") for m in (1, 2)]
                         + [("fdtd_coef", "mesh2x2", 1)])
def test_fdtd_layouts_with_neighbours(gpu, oracle, monkeypatch, app, decomposition, m):
    """Eight planes of one field each, AoS cells and two planes of 16-byte halves; two sub-iterations, time-dependent
    values (one device table per call); the source's cut-off and the detection iteration lie inside the run."""
    from test_parity_gpu import fdtd_setup

    d = DECOMPOSITIONS[decomposition]
    H, W = extents(app, m, *ranks_of(d))
    po, pc, cells = fdtd_setup(oracle, H, W)
    n1, n2 = shape_of(app, m)[3]
    offset = 5
    for params in (po, pc):
        params.detect_iteration = offset + n1 // 2
        params.cutoff_iteration = offset + n1 + n2 // 2
    got, n = decomposed(app, pc, bytes(32), cells, offset, m, d, monkeypatch)
    want = oracle.fdtd(po, cells, n, iteration_offset=offset, n_threads=8)
    assert np.array_equal(bits(got), bits(want))
    assert np.abs(want["hz_sum"]).max() > 0 and np.abs(want["hz"]).max() > 0

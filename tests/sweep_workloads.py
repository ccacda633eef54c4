"""Workloads the GPU tests share: a registered transition function, its parameter block, halo cell, cells on a grid and
the oracle routine that advances them.  A plain module (imported by name from the tests beside it), no fixtures.

  * `Workload`: what tests/test_pass_driver_gpu.py drives the pass driver with (Jacobi5General and HotSpot, planes on
    the device, the oracle's cells after n generations).
  * `fdtd_setup`: the FDTD parameters and material coefficients of tests/test_parity_gpu.py::test_fdtd_bit_exact.
  * `LaunchWorkload`: one for EVERY name of capi.list_apps(), on the host, for tests that call ststhip_app_sweep
    themselves (tests/test_launch_geometry_gpu.py).  A name it does not know raises KeyError: a newly registered kernel
    has to be given a workload here before that file passes again."""
import numpy as np

N_THREADS = 8

JACOBI5_COEF = [0.11, 0.19, 0.23, 0.31, 0.16]


def jacobi_params(coef):
    from stencilstream_amd import capi

    p = capi.JacobiParams()
    for i, c in enumerate(coef):
        p.coef[i] = float(np.float32(c))
    return p


def hotspot_cells(oracle, shape, rng, dtype=None):
    dtype = oracle.HOTSPOT_CELL if dtype is None else dtype
    cells = np.zeros(shape, dtype=dtype)
    if dtype == oracle.HOTSPOT_CELL:
        cells["temp"] = 320 + 10 * rng.random(shape, dtype=np.float32)
        cells["power"] = rng.random(shape, dtype=np.float32) * 0.01
    else:
        cells["temp"] = 320 + 10 * rng.random(shape)
        cells["power"] = rng.random(shape) * 0.01
    return cells


class Workload:
    """A precompiled transition function on one grid: planes on the device, the oracle's cells after n generations."""

    def __init__(self, oracle, app, shape):
        import torch

        from stencilstream_amd import capi

        self.oracle, self.app, self.shape = oracle, app, shape
        H, W = shape
        rng = np.random.default_rng(H * 131 + W + len(app))
        if app == "jacobi5general":
            self.coef = list(JACOBI5_COEF)
            self.params = jacobi_params(self.coef)
            self.halo = np.float32(0.0).tobytes()
            self.known = {0: rng.random((H, W), dtype=np.float32)}
        else:
            assert app == "hotspot"
            self.hp = oracle.hotspot_params(H, W)
            self.params = capi.HotspotParams(self.hp.Rx_1, self.hp.Ry_1, self.hp.Rz_1, self.hp.Cap_1)
            self.halo = bytes(8)
            self.known = {0: hotspot_cells(oracle, (H, W), rng)}
        self.info = capi.app_info(app)
        self.dom = capi.Domain(H, W, 0, H, W)
        self.host = self.planes_of(self.known[0])
        self.src = [torch.from_numpy(p).cuda() for p in self.host]
        self.dst = [torch.empty_like(t) for t in self.src]
        self.stream = torch.cuda.Stream()
        self._launch_ms = None
        torch.cuda.synchronize()

    def planes_of(self, cells):
        if self.app == "jacobi5general":
            return [np.ascontiguousarray(cells)]
        return [np.ascontiguousarray(cells["temp"]), np.ascontiguousarray(cells["power"])]

    def want(self, n):
        """The oracle's planes after n generations (neither function depends on the generation's number: continued
        from the nearest earlier result, computed once, never changed)."""
        if n not in self.known:
            m = max(k for k in self.known if k < n)
            if self.app == "jacobi5general":
                self.known[n] = self.oracle.jacobi("Jacobi5General", self.coef, self.known[m], n - m, halo=0.0,
                                                   n_threads=N_THREADS)
            else:
                self.known[n] = self.oracle.hotspot(self.hp, self.known[m], n - m, n_threads=N_THREADS)
        return self.planes_of(self.known[n])

    def desc(self, alt=0, key=0):
        from stencilstream_amd import capi

        return capi.sweep_desc_of(self.app, alt, key)

    def launch_ms(self):
        """One undelayed launch of the deepest depth over the whole grid, between two events (the second of two)."""
        import torch

        from stencilstream_amd import capi

        if self._launch_ms is None:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            H = self.shape[0]
            for _ in range(2):
                t0.record(self.stream)
                capi.app_sweep(self.app, self.params, self.halo, self.dom, [t.data_ptr() for t in self.src],
                               [t.data_ptr() for t in self.dst], 0, H, 0, self.info.max_generations,
                               self.stream.cuda_stream)
                t1.record(self.stream)
                t1.synchronize()
            self._launch_ms = t0.elapsed_time(t1)
        return self._launch_ms


def fdtd_setup(oracle, H, W):
    from stencilstream_amd import capi

    # parameters in the range of examples/fdtd/experiments/default.json, source off-centre
    kw = dict(dt=8.3e-18, t_0=3e-13 * 0.01, tau=1e-13 * 0.01, omega=7.5e14, cutoff_iteration=40,
              detect_iteration=10, source_radius_squared=36.0, source_r=H / 2.0 + 3, source_c=W / 2.0 - 2,
              source_distance_bound=0.0, double_center_rc=float(H))
    kw["source_distance_bound"] = 36.0 - (kw["source_c"] ** 2 + kw["source_r"] ** 2)
    po, pc = oracle.FdtdParams(), capi.FdtdParams()
    for k, v in kw.items():
        setattr(po, k, v)
        setattr(pc, k, v)
    rng = np.random.default_rng(3)
    cells = np.zeros((H, W), dtype=oracle.FDTD_CELL)
    for f in ("ex", "ey", "hz"):
        cells[f] = (rng.random((H, W), dtype=np.float32) - 0.5) * 1e-3
    inside = ((np.arange(H)[:, None] - H / 2) ** 2 + (np.arange(W)[None, :] - W / 2) ** 2) < (min(H, W) * 0.4) ** 2
    cells["ca"] = np.where(inside, 1.0, 1.0).astype(np.float32)
    cells["cb"] = np.where(inside, 0.31, 0.0).astype(np.float32)
    cells["da"] = np.where(inside, 1.0, 1.0).astype(np.float32)
    cells["db"] = np.where(inside, 0.29, 0.0).astype(np.float32)
    return po, pc, cells


# ------------------------------------------------------------------------------------------------ one per registered name
# what a destination plane is filled with before a launch: a quiet NaN with a payload no computation produces for
# float planes (fp32: 0x7fc00bad, fp64: 0x7ff8000000000bad), the byte 0xA5 for the cells of the Game of Life
SENTINEL_F32 = np.array([0x7FC00BAD], dtype="<u4").view(np.uint8)
SENTINEL_F64 = np.array([0x7FF8000000000BAD], dtype="<u8").view(np.uint8)
SENTINEL_LIFE = np.array([0xA5], dtype=np.uint8)

JACOBI_VARIANTS = {  # registered name -> (the oracle's variant, number of coefficients)
    "jacobi1general": ("Jacobi1General", 1), "jacobi2constant": ("Jacobi2Constant", 0),
    "jacobi3constant": ("Jacobi3Constant", 0), "jacobi4constant": ("Jacobi4Constant", 0),
    "jacobi5constant": ("Jacobi5Constant", 0), "jacobi4general": ("Jacobi4General", 4),
    "jacobi9general": ("Jacobi9General", 9), "jacobi5general": ("Jacobi5General", 5),
    "jacobi5general_independent": ("Jacobi5General", 5), "jacobi5general_fma": ("Jacobi5General", 5),
}
UNIFORM_CHAIN = ("jacobi5uniform_first", "jacobi5uniform", "jacobi5uniform_last")
UNIFORM_C = 0.2


class LaunchWorkload:
    """A registered transition function on a grid of `shape` rows x columns (columns counted in the function's own
    cells: conway_packed's are words of four Game-of-Life cells), on the host:

      info, params, halo     what ststhip_app_sweep takes
      cells                  the grid at generation `offset` (the function's cell dtype)
      offset                 the iteration index of the first generation (5 for functions that check or use it)
      sentinel               bytes a destination plane is filled with
      want(n)                the oracle's cells after n generations, computed once and kept
      fma                    the function is the build with fused multiply-adds: want() needs oracle.use_fma_build()

    The three product-carrying middle kernels carry the oracle of the chain first -> middle -> last (raw values in and
    out, the products in between are nobody's interface): want(n) is the plain Jacobi after n generations."""

    def __init__(self, oracle, app, shape):
        from stencilstream_amd import capi

        self.oracle, self.app = oracle, app
        self.info = capi.app_info(app)
        H, W = shape
        self.shape = (H, W)
        rng = np.random.default_rng(0x5EED + len(app) * 1009 + sum(app.encode()))
        self.offset, self.fma, self.sentinel = 0, False, SENTINEL_F32
        self._known = {}
        if app in JACOBI_VARIANTS:
            variant, ncoef = JACOBI_VARIANTS[app]
            coef = list(JACOBI5_COEF) if ncoef == 5 else list(rng.random(ncoef, dtype=np.float32) * 0.2)
            self.params, self.halo = jacobi_params(coef), np.float32(0.25).tobytes()
            self.cells = rng.random((H, W), dtype=np.float32)
            self.fma = app.endswith("_fma")
            self._advance = lambda cells, n: oracle.jacobi(variant, coef, cells, n, halo=0.25, n_threads=N_THREADS)
        elif app.startswith("jacobi5uniform"):
            # five equal positive coefficients, halo +0: the only setting these kernels are valid for
            self.params, self.halo = capi.JacobiUniformParams(float(np.float32(UNIFORM_C))), np.float32(0.0).tobytes()
            self.cells = rng.random((H, W), dtype=np.float32)
            self._advance = lambda cells, n: oracle.jacobi("Jacobi5General", [UNIFORM_C] * 5, cells, n, halo=0.0,
                                                           n_threads=N_THREADS)
        elif app == "jacobi25general":
            coef = (rng.random(25, dtype=np.float32) / 12).astype(np.float32)
            self.params = capi.Jacobi25Params()
            for i in range(25):
                self.params.coef[i] = float(coef[i])
            self.halo = np.float32(0.25).tobytes()
            self.cells = rng.random((H, W), dtype=np.float32)
            self._advance = lambda cells, n: oracle.jacobi25(coef, cells, n, halo=0.25, n_threads=N_THREADS)
        elif app in ("hotspot", "hotspot_aos", "hotspot_independent"):
            hp = oracle.hotspot_params(H, W)
            self.params, self.halo = capi.HotspotParams(hp.Rx_1, hp.Ry_1, hp.Rz_1, hp.Cap_1), bytes(8)
            self.cells = hotspot_cells(oracle, (H, W), rng)
            self._advance = lambda cells, n: oracle.hotspot(hp, cells, n, n_threads=N_THREADS)
        elif app in ("hotspot_f64", "hotspot_f64_aos"):
            hp = oracle.hotspot_params(H, W)
            vals = [float(hp.Rx_1), float(hp.Ry_1), float(hp.Rz_1), float(hp.Cap_1)]
            po = oracle.HotspotParamsF64(*vals)
            self.params, self.halo, self.sentinel = capi.HotspotParamsF64(*vals), bytes(16), SENTINEL_F64
            self.cells = hotspot_cells(oracle, (H, W), rng, oracle.HOTSPOT_CELL_F64)
            self._advance = lambda cells, n: oracle.hotspot_f64(po, cells, n, n_threads=N_THREADS)
        elif app == "conway":
            self.params, self.halo, self.sentinel = capi.NoParams(), b"\0", SENTINEL_LIFE
            self.cells = (rng.random((H, W)) < 0.37).astype(np.uint8)
            self._advance = lambda cells, n: oracle.conway(cells, n, n_threads=N_THREADS)
        elif app == "conway_packed":
            # the same rule on 32-bit words of four cells (bytes 0 / 1), dead halo: the oracle sees the bytes
            self.params, self.halo, self.sentinel = capi.NoParams(), bytes(4), SENTINEL_LIFE
            self.cells = np.ascontiguousarray((rng.random((H, 4 * W)) < 0.37).astype(np.uint8)).view("<u4")
            self._advance = lambda cells, n: np.ascontiguousarray(
                oracle.conway(np.ascontiguousarray(cells).view(np.uint8), n, n_threads=N_THREADS)).view("<u4")
        elif app.startswith("selfcheck"):
            radius = int(app[len("selfcheck")])
            halo = np.zeros((), dtype=oracle.SELFCHECK_CELL)
            halo["status"] = 2
            self.offset = 5  # a wrong generation index inside a launch shows in the cells' status
            self.params, self.halo = capi.NoParams(), halo.tobytes()
            self.cells = oracle.selfcheck_input(H, W, self.offset)
            self._advance = lambda cells, n: oracle.selfcheck(radius, cells, self.offset, n, n_threads=N_THREADS)
        elif app.startswith("fdtd_coef"):
            po, pc, cells = fdtd_setup(oracle, H, W)
            self.offset = 5  # the source term is a function of the iteration; detect_iteration = 10 falls into a launch
            self.params, self.halo, self.cells = pc, bytes(oracle.FDTD_CELL.itemsize), cells
            self._advance = lambda cells, n: oracle.fdtd(po, cells, n, iteration_offset=self.offset, n_threads=N_THREADS)
        else:
            raise KeyError(f"no workload for the registered transition function {app!r}: add one to tests/sweep_workloads.py")
        assert self.cells.dtype.itemsize == self.info.cell_size, (app, self.cells.dtype, self.info.cell_size)

    def want(self, n):
        """The cells `n` generations after `cells` (generation offset .. offset + n), from the oracle; every call for
        the same n returns the same array, which nobody changes."""
        if n not in self._known:
            if self.fma:
                with self.oracle.use_fma_build():
                    self._known[n] = self._advance(self.cells, n)
            else:
                self._known[n] = self._advance(self.cells, n)
            self._known[n].setflags(write=False)
        return self._known[n]

"""Parity of the HIP sweeps with the CPU oracle on subnormal, non-finite and signed-zero cells (tests/special_values.py:
the generators and the comparison rule -- NaNs in the same cells, every other cell bit for bit, no tolerance).

"Bit-exact" holds only while every kernel keeps subnormals, keeps the sign of a zero and overflows at the same
operation as the reference's expression; the product-carrying form of the five-point Jacobi carries fl(c*x) between
levels and must go subnormal or infinite exactly where Jacobi5General does.  CASES is shared with
test_special_values_cpu.py, which pins the oracle on such data and checks on the oracle's result of every case that the
class the case is named for is really there (so that no case passes on a grid of zeros or of NaNs alone).

Depths: 1 generation is the only launch of its call, 8 and 17 make a first and a last one, 37 has middle launches.
Special cells spread by one cell per generation, so huge data and non-finite halos run few generations and the deep
runs with inf and NaN use planted data."""
import dataclasses
import functools
import zlib

import numpy as np
import pytest

import special_values as sv

SMALL, MIDDLE, LARGE = (3, 5), (130, 257), (300, 700)

# Distinct coefficients.  With a sum of 1 (POSITIVE) tiny data stays around the subnormal threshold for many
# generations and huge data never overflows; larger ones (THIRDS, NEAR_ONE) overflow after a few generations.
MIXED = (0.47, -0.43, 0.51, 0.39, -0.44)
POSITIVE = (0.11, 0.19, 0.23, 0.31, 0.16)
NEAR_ONE = (0.9, 0.91, 0.89, 0.92, 0.88)
THIRDS = (0.3, 0.31, 0.29, 0.32, 0.28)
MIXED9 = (0.31, -0.37, 0.29, -0.33, 0.36, 0.3, -0.28, 0.35, -0.34)
POSITIVE9 = (0.05, 0.1, 0.07, 0.12, 0.2, 0.13, 0.08, 0.14, 0.11)
MIXED25 = tuple(float(np.float32((-1) ** (i * i // 3) * (0.15 + 0.004 * i))) for i in range(25))
POSITIVE25 = tuple(float(np.float32(0.02 + 0.002 * i)) for i in range(25))
SUBNORMAL_COEF = float(np.ldexp(np.float32(1.25), -130))
SUBNORMAL_HALO = float(np.ldexp(np.float32(1.5), -140))
INF, NAN = float("inf"), float("nan")

SWEEPS = {("jacobi25", ""): "jacobi25general", ("hotspot", "planes"): "hotspot", ("hotspot", "aos"): "hotspot_aos",
          ("hotspot_f64", "planes"): "hotspot_f64", ("hotspot_f64", "aos"): "hotspot_f64_aos",
          ("fdtd", "grouped"): "fdtd_coef_grouped", ("fdtd", "aos"): "fdtd_coef_aos"}


@dataclasses.dataclass(frozen=True)
class Case:
    app: str  # jacobi, jacobi25, hotspot, hotspot_f64, fdtd
    data: str  # the generator of special_values, or what is planted where
    shape: tuple
    n: int
    named: str  # the class of special_values.classify the case is there for
    variant: str = ""  # the Jacobi variant, or the layout of the cells
    coef: tuple = ()
    halo: float = 0.0  # Jacobi only; HotSpot runs a NaN halo against the oracle's zero, FDTD a zero one
    offset: int = 0
    fastpath: str = ""  # STSTHIP_JACOBI_FASTPATH for the run, "" = unset
    zero: str = ""  # negzero data: "-0" / "+0" / "both", the zeros the oracle gives

    @property
    def id(self):
        parts = [self.variant or self.app, self.data, "x".join(map(str, self.shape)), f"n{self.n}"]
        if self.app == "jacobi" and len(self.coef) == 5:
            parts.append(f"c{self.coef[0]:.3g}" + ("x5" if len(set(self.coef)) == 1 else ".."))
        if self.app in ("hotspot", "hotspot_f64", "fdtd"):
            parts.insert(0, self.app)
        if self.halo != 0.0 or np.signbit(self.halo):
            parts.append(f"halo{self.halo:.3g}")
        if self.offset:
            parts.append(f"offset{self.offset}")
        if self.fastpath:
            parts.append(f"fastpath{self.fastpath}")
        return "-".join(parts)

    @property
    def sweep(self):
        """The sweep's name in the library's registry."""
        return self.variant.lower() if self.app == "jacobi" else SWEEPS[(self.app, self.variant)]


def _cases():
    cases = []
    five = functools.partial(Case, "jacobi", variant="Jacobi5General")
    # Jacobi5General, distinct coefficients; halos 0.25, subnormal, -0.0, +inf and NaN; two iteration offsets
    cases += [
        five("tiny", SMALL, 1, "subnormal", coef=MIXED, halo=SUBNORMAL_HALO),
        five("tiny", MIDDLE, 1, "subnormal", coef=MIXED, halo=-0.0),
        five("tiny", MIDDLE, 8, "subnormal", coef=POSITIVE, halo=SUBNORMAL_HALO),
        five("tiny", LARGE, 17, "subnormal", coef=POSITIVE, halo=-0.0),
        five("tiny", LARGE, 37, "subnormal", coef=POSITIVE, halo=0.25, offset=5),
        five("huge", SMALL, 1, "inf", coef=NEAR_ONE, halo=0.25),
        five("huge", MIDDLE, 1, "inf", coef=NEAR_ONE, halo=-0.0),
        five("huge", MIDDLE, 2, "nan", coef=NEAR_ONE, halo=SUBNORMAL_HALO),
        five("huge", LARGE, 8, "inf", coef=THIRDS, halo=0.25),
        five("planted", SMALL, 1, "nan", coef=POSITIVE, halo=0.25),
        five("planted", MIDDLE, 8, "nan", coef=POSITIVE, halo=-0.0),
        five("planted", LARGE, 17, "nan", coef=MIXED, halo=0.25),
        five("planted", LARGE, 37, "nan", coef=POSITIVE, halo=SUBNORMAL_HALO, offset=3),
        five("planted", MIDDLE, 1, "inf", coef=POSITIVE, halo=INF),
        five("planted", LARGE, 8, "nan", coef=POSITIVE, halo=NAN),
        five("negzero", MIDDLE, 8, "negzero", coef=POSITIVE, halo=-0.0, zero="-0"),
        five("negzero", LARGE, 17, "negzero", coef=POSITIVE, halo=0.0, zero="both"),
    ]
    # five equal positive coefficients and a +0 halo: the product-carrying form, and the general kernel on the same
    # parameters with the switch off
    for fastpath in ("", "0"):
        uniform = functools.partial(five, halo=0.0, fastpath=fastpath)
        cases += [
            uniform("tiny", MIDDLE, 8, "subnormal", coef=(0.2,) * 5),
            uniform("tiny", LARGE, 17, "subnormal", coef=(0.2,) * 5),
            uniform("planted", MIDDLE, 17, "nan", coef=(0.2,) * 5),
            uniform("planted", LARGE, 37, "nan", coef=(0.2,) * 5),
            uniform("tiny", MIDDLE, 1, "subnormal", coef=(1.0,) * 5),
            uniform("tiny", LARGE, 2, "subnormal", coef=(1.0,) * 5),
            uniform("huge", SMALL, 1, "inf", coef=(1.0,) * 5),
            uniform("huge", LARGE, 1, "inf", coef=(1.0,) * 5),
            uniform("huge", MIDDLE, 2, "nan", coef=(1.0,) * 5),
            uniform("planted", MIDDLE, 8, "nan", coef=(1.0,) * 5),
            uniform("tiny", LARGE, 1, "subnormal", coef=(3.0e-3,) * 5),
            uniform("tiny", MIDDLE, 3, "subnormal", coef=(3.0e-3,) * 5),
            uniform("planted", LARGE, 17, "nan", coef=(3.0e-3,) * 5),
            uniform("huge", MIDDLE, 2, "subnormal", coef=(SUBNORMAL_COEF,) * 5),
            uniform("planted", MIDDLE, 1, "subnormal", coef=(SUBNORMAL_COEF,) * 5),
            uniform("planted", SMALL, 1, "nan", coef=(SUBNORMAL_COEF,) * 5),
        ]
    # the other variants; negzero data with positive coefficients and a -0.0 halo: a sum that starts from 0.0f gives
    # +0, a sum of the products alone -0
    for variant, mixed, positive in (("Jacobi1General", (0.5,), (0.5,)), ("Jacobi4Constant", (), ()),
                                     ("Jacobi5Constant", (), ()), ("Jacobi9General", MIXED9, POSITIVE9)):
        one = functools.partial(Case, "jacobi", variant=variant)
        # c0 * centre: a planted cell stays where it is, so it counts on the smallest grid only; without the centre a
        # special cell reaches every other cell only, so those runs are deeper
        middle, large = (SMALL, SMALL) if variant == "Jacobi1General" else (MIDDLE, LARGE)
        deep = variant == "Jacobi4Constant"
        zero, named = ("+0", "zero") if variant == "Jacobi9General" else ("-0", "negzero")
        cases += [
            one("tiny", MIDDLE, 8, "subnormal", coef=positive, halo=SUBNORMAL_HALO),
            one("tiny", LARGE, 17, "subnormal", coef=positive, halo=0.25),
            one("planted", middle, 17 if deep else 8, "nan", coef=positive, halo=-0.0),
            one("planted", large, 37 if deep else 17, "nan", coef=mixed, halo=0.25),
            one("negzero", MIDDLE, 8, named, coef=positive, halo=-0.0, zero=zero),
            one("negzero", SMALL, 1, named, coef=positive, halo=-0.0, zero=zero),
        ]
    dense = functools.partial(Case, "jacobi25")
    cases += [
        dense("tiny", SMALL, 1, "subnormal", coef=MIXED25, halo=SUBNORMAL_HALO),
        dense("tiny", MIDDLE, 7, "subnormal", coef=POSITIVE25, halo=SUBNORMAL_HALO),
        dense("planted", MIDDLE, 3, "nan", coef=POSITIVE25, halo=0.25),
        dense("planted", LARGE, 7, "nan", coef=MIXED25, halo=-0.0),
        dense("negzero", MIDDLE, 7, "zero", coef=POSITIVE25, halo=-0.0, zero="+0"),
    ]
    # HotSpot, fp32 and fp64, both layouts: specials planted in temp, in power, and temperatures near the overflow
    # threshold
    for app in ("hotspot", "hotspot_f64"):
        for layout in ("planes", "aos"):
            hot = functools.partial(Case, app, variant=layout)
            cases += [
                hot("temp-planted", SMALL, 1, "nan"),
                hot("temp-planted", MIDDLE, 8, "nan"),
                hot("power-planted", LARGE, 23, "nan"),
                hot("overflow", MIDDLE, 1, "inf"),
                hot("overflow", LARGE, 2, "nan"),
            ]
    # FDTD: ex, ey and hz scaled into the subnormal range, and planted specials
    for layout in ("grouped", "aos"):
        wave = functools.partial(Case, "fdtd", variant=layout)
        cases += [
            wave("tiny", MIDDLE, 7, "subnormal"),
            wave("tiny", LARGE, 17, "subnormal", offset=5),
            wave("planted", MIDDLE, 8, "nan"),
        ]
    return cases


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)


def strip_width(case):
    from stencilstream_amd import capi

    return int(capi.app_info(case.sweep).strip_width)


@functools.lru_cache(maxsize=4)
def _reference(oracle, case, strips):
    """(what the sweep starts from, the oracle's result) of a case; `case` comes without layout and switch, so the
    layouts and both settings of the switch share one reference."""
    seed = case.shape[0] * 1000003 + case.shape[1] * 101 + zlib.crc32(case.data.encode()) % 1000
    if case.app in ("jacobi", "jacobi25"):
        grid = sv.planted(case.shape, seed, strips) if case.data == "planted" else getattr(sv, case.data)(case.shape, seed)
        if case.app == "jacobi":
            want = oracle.jacobi(case.variant, case.coef, grid, case.n, halo=case.halo, iteration_offset=case.offset,
                                 n_threads=8)
        else:
            want = oracle.jacobi25(np.asarray(case.coef, dtype=np.float32), grid, case.n, halo=case.halo, n_threads=8)
        return grid, want
    rng = np.random.default_rng(seed)
    if case.app in ("hotspot", "hotspot_f64"):
        double = case.app == "hotspot_f64"
        real = np.float64 if double else np.float32
        cells = np.zeros(case.shape, dtype=oracle.HOTSPOT_CELL_F64 if double else oracle.HOTSPOT_CELL)
        temp = (320 + 10 * rng.random(case.shape)).astype(real)
        power = (rng.random(case.shape) * 0.01).astype(real)
        if case.data == "temp-planted":
            sv.plant(temp, strips)
        elif case.data == "power-planted":
            sv.plant(power, strips)
        else:  # sums of two temperatures reach past the largest finite number in part of the cells
            temp = (np.finfo(real).max * (0.30 + 0.25 * rng.random(case.shape))).astype(real)
        cells["temp"], cells["power"] = temp, power
        p32 = oracle.hotspot_params(*case.shape)
        if double:
            params = oracle.HotspotParamsF64(*[float(getattr(p32, k)) for k in ("Rx_1", "Ry_1", "Rz_1", "Cap_1")])
            want = oracle.hotspot_f64(params, cells, case.n, n_threads=8)
        else:
            params = p32
            want = oracle.hotspot(params, cells, case.n, n_threads=8)
        return (params, cells), want
    from test_parity_gpu import fdtd_setup  # its parameters and material coefficients

    po, pc, cells = fdtd_setup(oracle, *case.shape)
    for name in ("ex", "ey", "hz"):
        if case.data == "tiny":  # (-0.5, 0.5) * 1e-3 * 2^-118: below 2^-126
            cells[name] = np.ldexp(cells[name], -118)
        else:
            field = cells[name].copy()
            cells[name] = sv.plant(field, strips)
    want = oracle.fdtd(po, cells, case.n, iteration_offset=case.offset, n_threads=8)
    return (po, pc, cells), want


def reference(oracle, case):
    shared = dataclasses.replace(case, fastpath="", variant=case.variant if case.app == "jacobi" else "")
    return _reference(oracle, shared, strip_width(case))


def dynamic_fields(case, cells):
    """The fields a sweep changes: what the content conditions are about."""
    if case.app in ("hotspot", "hotspot_f64"):
        return cells["temp"]
    if case.app == "fdtd":
        return np.stack([cells[name] for name in ("ex", "ey", "hz")])
    return cells


def transition_function(case, start):
    from stencilstream_amd import capi, update as U

    if case.app == "jacobi":
        return U.jacobi(case.variant, case.coef), np.float32(case.halo)
    if case.app == "jacobi25":
        p = capi.Jacobi25Params()
        for i in range(25):
            p.coef[i] = case.coef[i]
        return U.TransitionFunction("jacobi25general", p, np.dtype("<f4")), np.float32(case.halo)
    if case.app in ("hotspot", "hotspot_f64"):
        params = start[0]
        make = U.hotspot_f64 if case.app == "hotspot_f64" else U.hotspot
        tf = make(params.Rx_1, params.Ry_1, params.Rz_1, params.Cap_1, split_cell_structure=case.variant == "planes")
        halo = np.zeros((), dtype=tf.cell_dtype)
        halo["temp"] = halo["power"] = np.nan  # the rim rule (top = old, ...) keeps the halo out; the oracle's is zero
        return tf, halo
    return U.fdtd(start[1], layout=case.variant), np.zeros((), dtype=U.FDTD_CELL)


def run_on_gpu(case, start, monkeypatch):
    """The case through stencilstream_amd.update: the result grid, still on the device."""
    from stencilstream_amd import update as U

    if case.fastpath:
        monkeypatch.setenv("STSTHIP_JACOBI_FASTPATH", case.fastpath)
    else:
        monkeypatch.delenv("STSTHIP_JACOBI_FASTPATH", raising=False)
    tf, halo = transition_function(case, start)
    cells = start if case.app in ("jacobi", "jacobi25") else start[-1]
    su = U.StencilUpdate(U.Params(tf, halo_value=halo, iteration_offset=case.offset, n_iterations=case.n, blocking=True))
    result = su(U.Grid.from_numpy(cells))
    assert su.get_n_processed_cells() == case.n * case.shape[0] * case.shape[1]
    return result


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_sweep_equals_the_oracle_on_special_values(gpu, oracle, monkeypatch, case):
    start, want = reference(oracle, case)
    if case.zero:  # which zeros the oracle gives: the comparison below then tells +0 from -0
        negative = np.signbit(want)
        assert (want == 0).all() and {"-0": negative.all(), "+0": not negative.any(),
                                      "both": negative.any() and not negative.all()}[case.zero]
    got = run_on_gpu(case, start, monkeypatch).to_numpy()
    print(case.id, {k: round(float(v), 4) for k, v in sv.classify(dynamic_fields(case, got)).items()})
    sv.assert_same_cells(got, want, case.id)


NORMS_CASES = [next(c for c in CASES if (c.app, c.data, c.shape) == key)
               for key in (("jacobi", "planted", LARGE), ("jacobi", "huge", LARGE), ("hotspot", "overflow", LARGE),
                           ("hotspot_f64", "temp-planted", MIDDLE), ("fdtd", "planted", MIDDLE))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", NORMS_CASES, ids=lambda c: c.id)
def test_norms_of_a_sweeps_result_count_its_non_finite_cells(gpu, oracle, monkeypatch, case):
    """Grid.norms() on the grid a sweep returned: n_nonfinite is the number of NaN and +-inf cells of the oracle's
    result, max_abs the largest magnitude among its finite cells (-inf if there is none: hip/Reduce.hpp)."""
    start, want = reference(oracle, case)
    norms = run_on_gpu(case, start, monkeypatch).norms()
    total = 0
    for name, got in norms.items():
        values = (want if name is None else want[name]).astype(np.float64).reshape(-1)
        finite = values[np.isfinite(values)]
        expected = float(np.abs(finite).max()) if finite.size else float("-inf")
        print(f"{case.id} {name}: n_nonfinite {got.n_nonfinite} / {values.size - finite.size}, max_abs {got.max_abs!r} / {expected!r}")
        assert got.n_cells == values.size and got.n_nonfinite == values.size - finite.size
        assert np.float64(got.max_abs).tobytes() == np.float64(expected).tobytes()
        total += got.n_nonfinite
    assert total > 0, "the case has no non-finite cell to count"

"""Grids of subnormal, non-finite and signed-zero cells for the parity tests, and the rule their results are compared by.

The rule (`differing`, `assert_same_cells`): `got` and `want` hold NaNs in exactly the same cells, and every other cell
-- +-inf and +-0 included -- is equal bit for bit.  Which NaN comes out of an operation with two NaN operands, and the
sign and payload of a NaN an operation creates, differ between x86 and the GPU, so payloads and signs of NaNs are left
out.  That is the only relaxation: there is no tolerance anywhere.

The generators are seeded and work for float32 and float64; the exponent ranges below are float32's, float64's sit at
the same distance from its own limits."""
import numpy as np


def _floats(a):
    """A plain float array of the cells: structured cells of one float type become a trailing axis of fields."""
    a = np.ascontiguousarray(a)
    if a.dtype.names is not None:
        kinds = {a.dtype[n] for n in a.dtype.names}
        assert len(kinds) == 1, "cells of mixed field types"
        kind = kinds.pop()
        a = a.view(kind).reshape(a.shape + (len(a.dtype.names),))
    assert a.dtype.kind == "f" and a.dtype.itemsize in (4, 8), a.dtype
    return a


def _bits(a):
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def differing(got, want):
    """Boolean array of the cells (fields) that break the rule."""
    g, w = _floats(got), _floats(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (g.shape, g.dtype, w.shape, w.dtype)
    g_nan, w_nan = np.isnan(g), np.isnan(w)
    return (g_nan != w_nan) | (~w_nan & (_bits(g) != _bits(w)))


def assert_same_cells(got, want, what=""):
    bad = differing(got, want)
    if bad.any():
        g, w = _floats(got), _floats(want)
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} cells differ, the first at {first}: got "
                             f"{g[first]!r} ({int(_bits(g)[first]):#x}), want {w[first]!r} ({int(_bits(w)[first]):#x})")


def classify(array):
    """Shares of the cells (fields) that are subnormal, +-0, -0, +-inf and NaN; `normal` is the rest."""
    a = _floats(array).reshape(-1)
    n = max(a.size, 1)
    tiny = np.finfo(a.dtype).tiny  # the smallest normal
    mag = np.abs(a)
    with np.errstate(invalid="ignore"):
        subnormal = (mag > 0) & (mag < tiny)
        zero = a == 0
        normal = np.isfinite(a) & (mag >= tiny)
    return {"subnormal": subnormal.sum() / n, "zero": zero.sum() / n, "negzero": (zero & np.signbit(a)).sum() / n,
            "inf": np.isinf(a).sum() / n, "nan": np.isnan(a).sum() / n, "normal": normal.sum() / n}


def _spread(shape, seed, lowest, highest, dtype):
    """Random sign and mantissa, exponents uniform in [lowest, highest]."""
    rng = np.random.default_rng(seed)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    values = np.ldexp(sign * (1.0 + rng.random(shape)), rng.integers(lowest, highest + 1, shape))
    with np.errstate(under="ignore"):
        return values.astype(dtype)


def tiny(shape, seed, dtype=np.float32):
    """Exponents 2^-150 .. 2^-120 around float32's smallest normal 2^-126: subnormals and normals side by side (the
    few values below half the smallest subnormal are zeros of either sign)."""
    least = np.finfo(dtype).minexp  # -126
    return _spread(shape, seed, least - 24, least + 6, dtype)


def huge(shape, seed, dtype=np.float32):
    """Exponents 2^120 .. 2^127, both signs: sums and products overflow."""
    most = np.finfo(dtype).maxexp  # 128
    return _spread(shape, seed, most - 8, most - 1, dtype)


def negzero(shape, seed=0, dtype=np.float32):
    return np.full(shape, -0.0, dtype=dtype)


def planted_sites(shape, strip_width=0):
    """Where `planted` puts its cells: {kind: [(row, column), ...]}.  A NaN sits in a corner, in the last column and
    on either side of a strip seam (of column 64 on a grid of one strip); a +inf with a -inf to its right sit in the last row's
    corner, in the first row and across the seam; subnormals sit in a corner, in the first column and beside the
    multiples of 64; the run of -0.0 goes along the first row across column 64 and down from the last row's corner."""
    H, W = shape
    seams = [c for c in range(strip_width, W, strip_width)] if 0 < strip_width < W else []
    seam = seams[0] if seams else (64 if W > 65 else W // 2)  # the column right of the seam
    sites = {"nan": [(0, 0)], "+inf": [(H - 1, W - 2)], "subnormal": [(0, W - 1)], "-0": []}
    if H >= 8 and W >= 8:
        sites["nan"] += [(H // 2, seam - 1), ((2 * H) // 3, W - 1), ((3 * H) // 4, seam)]
        sites["+inf"] += [(H // 3, seam - 1), (0, W // 2)]
        sites["subnormal"] += [(H // 2, 0), (H - 2, seam), (1, seam - 1)]
        sites["subnormal"] += [(H // 4, c + d) for c in range(64, W - 1, 64) for d in (-1, 0, 1)]
        for other in seams[1:]:
            sites["subnormal"] += [(H // 4 + 1, other - 1), (H // 4 + 1, other)]
        sites["-0"] += [(0, c) for c in range(1, min(W // 2 - 1, 70))] + [(r, 0) for r in range(H - 4, H)]
        if seams:
            sites["-0"] += [(H - 1, c) for c in range(seam - 3, seam + 3)]
    else:
        sites["-0"] += [(H - 1, c) for c in range(0, max(W - 3, 1))]
    taken = set()
    for kind in ("nan", "+inf", "subnormal", "-0"):
        kept = []
        for r, c in sites[kind]:
            cells = {(r, c), (r, c + 1)} if kind == "+inf" else {(r, c)}
            if all(0 <= rr < H and 0 <= cc < W for rr, cc in cells) and not (cells & taken):
                kept.append((r, c))
                taken |= cells
        sites[kind] = kept
    return sites


def plant(grid, strip_width=0):
    """Plants the cells of planted_sites into `grid` (a plain float array), in place: NaNs, +inf with -inf as its right
    neighbour (a NaN after one generation), subnormals and a run of -0.0."""
    sites = planted_sites(grid.shape, strip_width)
    for r, c in sites["nan"]:
        grid[r, c] = np.nan
    for r, c in sites["+inf"]:
        grid[r, c], grid[r, c + 1] = np.inf, -np.inf
    for i, (r, c) in enumerate(sites["subnormal"]):
        grid[r, c] = (-1) ** i * np.finfo(grid.dtype).smallest_subnormal * (1 + 37 * i)
    for r, c in sites["-0"]:
        grid[r, c] = -0.0
    return grid


def planted(shape, seed, strip_width=0, dtype=np.float32):
    """Values of both signs in (-1, 1) with a handful of planted cells (plant).  `strip_width`: the sweep's, as
    capi.app_info(...).strip_width gives it."""
    rng = np.random.default_rng(seed)
    return plant((2.0 * rng.random(shape) - 1.0).astype(dtype), strip_width)

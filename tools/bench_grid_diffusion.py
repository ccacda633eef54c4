#!/usr/bin/env python3
"""Time ststhip_grid_diffusion beside the calls that move the same number of planes.

    python tools/bench_grid_diffusion.py [--repeats 15] [--warmup 3] [--out profiles/grid_diffusion.txt]

The cases are interleaved: one round runs each of them once, between two device events on the stream; median, min and
max are over the rounds.  Every diffusion call is reported as a fraction of its yardstick's rate in the same rounds:

  (a) 16384^2 f32 planes as the library routes them: APPLY without a right-hand side (the dense kernel, 16-byte units)
      and SOLVE_DIAG (three planes read, one written) beside ststhip_grid_combine of three terms; APPLY with a
      right-hand side and JACOBI (four read, one written) beside the combine of four terms.  SOLVE_DIAG, APPLY with a
      right-hand side and JACOBI have the general kernel only: their dense instantiations lost, or did not reliably
      win, the A/B recorded in sessions 1 and 2 of profiles/grid_diffusion.txt
  (b) APPLY without a right-hand side through the general kernel (STSTHIP_DIFFUSION_GENERAL): the A/B of the two kernels
  (c) members of 32-byte 4608^2 cells, general kernel: JACOBI on five members of ONE grid of cells and on hz of five
      grids, beside ststhip_grid_stencil CROSS5 with a right-hand side on hz of three grids

"moved" = the bytes a call must move: every element read once and written once.  "lines" = the bytes of the 128-byte
cache lines the call touches; for planes the two are the same, for a member of 32-byte cells every line of every grid
that is read, and of the one that is written, is touched (8 x the elements).  The rates are lines per second, as in
profiles/grid_algebra.txt and profiles/grid_stencil.txt.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWITCH = "STSTHIP_DIFFUSION_GENERAL"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1, help="divide every edge by this (rehearsals)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from stencilstream_amd import capi

    if not torch.cuda.is_available():
        sys.exit("bench_grid_diffusion needs a GPU: a timing taken anywhere else says nothing")
    os.environ.pop(SWITCH, None)
    capi.init(0)
    dev = torch.device("cuda:0")
    lib = capi.load()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    na, nb = 16384 // args.scale, 4608 // args.scale
    with torch.cuda.stream(stream):
        # faces in (0.5, 1.5): the diagonal stays away from zero
        planes = [torch.rand(na * na, dtype=torch.float32, device=dev) + 0.5 for _ in range(5)]
        grids = [torch.rand(nb * nb * 8, dtype=torch.float32, device=dev) + 0.5 for _ in range(5)]
    stream.synchronize()

    # dst, u, kx, ky, rhs
    plane = [capi.grid_view(p.data_ptr(), 4, na, na) for p in planes]
    one = [capi.grid_view(grids[0].data_ptr() + 4 * member, 32, nb, nb) for member in (3, 2, 0, 1, 4)]
    hz = [capi.grid_view(g.data_ptr() + 8, 32, nb, nb) for g in grids]
    A, J, D = capi.DIFFUSION_APPLY, capi.DIFFUSION_JACOBI, capi.DIFFUSION_SOLVE_DIAG

    def diffusion(views, n, mode, has_rhs, general=False):
        desc = capi.grid_diffusion_desc(views[0], None if mode == D else views[1], views[2], views[3], "<f4", mode, n, n,
                                        sigma=0.1, scale=0.9, omega=0.8, halo=0.5, k_halo=1.0,
                                        rhs=views[4] if has_rhs else None, rhs_coef=0.25)

        def run():
            if general:
                os.environ[SWITCH] = "1"
            try:
                capi.grid_diffusion([desc], s)
            finally:
                os.environ.pop(SWITCH, None)
        return run

    def combine(views, n, n_terms):
        desc = capi.grid_combine_desc(views[0], "<f4", [(0.7 / (k + 1), views[k + 1]) for k in range(n_terms)], n, n)
        return lambda: capi.grid_combine([desc], s)

    def stencil(views, n):
        cross = [0.0, 0.26, 0.0, 0.24, -0.03, 0.25, 0.0, 0.27, 0.0]
        desc = capi.grid_stencil_desc(views[0], views[1], "<f4", capi.STENCIL_CROSS5, cross, n, n, halo=0.5, rhs=views[2],
                                      rhs_coef=0.25)
        return lambda: capi.grid_stencil([desc], s)

    pa, pb = 4 * na * na, 4 * nb * nb  # bytes of a plane, of a member
    # name, (bytes of cache lines touched, bytes that must move), yardstick, call
    cases = [
        (f"    grid_combine, 3 terms, {na}^2 f32 planes", (4 * pa, 4 * pa), None, combine(plane, na, 3)),
        ("(a) APPLY (dense kernel)", (4 * pa, 4 * pa), 0, diffusion(plane, na, A, False)),
        ("(b) APPLY through the general kernel", (4 * pa, 4 * pa), 0, diffusion(plane, na, A, False, True)),
        ("(a) SOLVE_DIAG", (4 * pa, 4 * pa), 0, diffusion(plane, na, D, True)),
        ("    grid_combine, 4 terms, planes", (5 * pa, 5 * pa), None, combine(plane, na, 4)),
        ("(a) APPLY + rhs", (5 * pa, 5 * pa), 4, diffusion(plane, na, A, True)),
        ("(a) JACOBI", (5 * pa, 5 * pa), 4, diffusion(plane, na, J, True)),
        (f"    grid_stencil CROSS5 + rhs, hz of 3 grids of {nb}^2 x 32 B", (24 * pb, 3 * pb), None, stencil(hz, nb)),
        ("(c) JACOBI, five members of one grid", (16 * pb, 5 * pb), 7, diffusion(one, nb, J, True)),
        ("(c) JACOBI, hz of five grids", (40 * pb, 5 * pb), 7, diffusion(hz, nb, J, True)),
        ("(c) APPLY, hz of four grids", (32 * pb, 4 * pb), 7, diffusion(hz, nb, A, False)),
    ]
    start, stop = C.c_void_p(), C.c_void_p()
    capi.check(lib.ststhip_event_create(C.byref(start)), "event")
    capi.check(lib.ststhip_event_create(C.byref(stop)), "event")
    times = [[] for _ in cases]
    ms = C.c_float()
    for round_ in range(args.warmup + args.repeats):
        for k, (_, _, _, run) in enumerate(cases):
            capi.check(lib.ststhip_event_record(start, s), "event")
            run()
            capi.check(lib.ststhip_event_record(stop, s), "event")
            capi.check(lib.ststhip_event_synchronize(stop), "event")
            capi.check(lib.ststhip_event_elapsed_ms(start, stop, C.byref(ms)), "event")
            if round_ >= args.warmup:
                times[k].append(ms.value * 1e-3)

    lines = [f"grid diffusion on {torch.cuda.get_device_name(0)}: {args.repeats} interleaved rounds after {args.warmup} warm-up "
             "rounds, device events around every call",
             f"{'case':58s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'moved MiB':>10s} {'lines TB/s':>11s} "
             f"{'moved TB/s':>11s} {'of its yardstick':>17s}"]
    med = [statistics.median(t) for t in times]
    rate = [moved[0] / med[k] for k, (_, moved, _, _) in enumerate(cases)]
    for k, (name, moved, yardstick, _) in enumerate(cases):
        share = "        yardstick" if yardstick is None else f"{rate[k] / rate[yardstick]:17.2f}"
        lines.append(f"{name:58s} {med[k] * 1e3:10.4f} {min(times[k]) * 1e3:8.4f} {max(times[k]) * 1e3:8.4f} "
                     f"{moved[1] / 2 ** 20:10.1f} {rate[k] / 1e12:11.3f} {moved[1] / med[k] / 1e12:11.3f} {share}")
    lines.append(f"APPLY, general kernel against dense kernel on the same planes (medians): {med[2] * 1e3:.4f} ms / "
                 f"{med[1] * 1e3:.4f} ms = {med[2] / med[1]:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as out:
            out.write(text)


if __name__ == "__main__":
    main()

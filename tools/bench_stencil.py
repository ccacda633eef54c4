#!/usr/bin/env python3
"""Time ststhip_grid_stencil beside the calls that move the same bytes.

    python tools/bench_stencil.py [--repeats 15] [--warmup 3] [--out profiles/grid_stencil.txt]

The cases are interleaved: one round runs each of them once, between two device events on the stream; median, min and
max are over the rounds.  Every stencil is reported as a fraction of its yardstick's rate in the same rounds:

  (a) 16384^2 f32 planes as the library routes them: CROSS5 and BOX9 without a right-hand side beside
      ststhip_grid_copy of a plane (one plane read, one written), with one beside ststhip_grid_combine of two terms (two
      read, one written).  BOX9 takes the dense kernel; CROSS5 has none -- it lost the A/B recorded in
      profiles/grid_stencil.txt -- and takes the general kernel here as well
  (b) the same four calls through the general kernel (STSTHIP_STENCIL_GENERAL): the A/B of the two kernels on planes
  (c) hz (4 of 32 bytes) of 4608^2 FDTD cells, general kernel: the same four beside the copy and the combine of hz

"moved" = the bytes a call must move: every element read once and written once.  "lines" = the bytes of the 128-byte
cache lines the call touches; for planes the two are the same, for a member of 32-byte cells every line of every grid is
touched (8 x the elements).  The rates are lines per second, as in profiles/grid_algebra.txt.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWITCH = "STSTHIP_STENCIL_GENERAL"


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
        sys.exit("bench_stencil needs a GPU: a timing taken anywhere else says nothing")
    os.environ.pop(SWITCH, None)
    capi.init(0)
    dev = torch.device("cuda:0")
    lib = capi.load()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    na, nb = 16384 // args.scale, 4608 // args.scale
    with torch.cuda.stream(stream):
        planes = [torch.rand(na * na, dtype=torch.float32, device=dev) for _ in range(3)]
        grids = [torch.rand(nb * nb * 8, dtype=torch.float32, device=dev) for _ in range(3)]
    stream.synchronize()

    plane = [capi.grid_view(p.data_ptr(), 4, na, na) for p in planes]
    hz = [capi.grid_view(g.data_ptr() + 8, 32, nb, nb) for g in grids]
    cross = [0.0, 0.26, 0.0, 0.24, -0.03, 0.25, 0.0, 0.27, 0.0]
    box = [0.05, 0.2, 0.06, 0.19, -0.03, 0.21, 0.04, 0.22, 0.07]

    def stencil(views, n, shape, has_rhs, general=False):
        desc = capi.grid_stencil_desc(views[0], views[1], "<f4", shape, cross if shape == capi.STENCIL_CROSS5 else box, n, n,
                                      halo=0.5, rhs=views[2] if has_rhs else None, rhs_coef=0.25)

        def run():
            if general:
                os.environ[SWITCH] = "1"
            try:
                capi.grid_stencil([desc], s)
            finally:
                os.environ.pop(SWITCH, None)
        return run

    def combine(views, n):
        desc = capi.grid_combine_desc(views[0], "<f4", [(0.7, views[1]), (0.25, views[2])], n, n)
        return lambda: capi.grid_combine([desc], s)

    def copy(views, n):
        desc = capi.grid_copy_desc(views[0], views[1], 4, n, n)
        return lambda: capi.grid_copy([desc], s)

    X, B = capi.STENCIL_CROSS5, capi.STENCIL_BOX9
    pa, pb = 4 * na * na, 4 * nb * nb  # bytes of a plane, of a member
    # name, (bytes of cache lines touched, bytes that must move), yardstick, call
    cases = [
        (f"    grid_copy {na}^2 f32 plane -> plane", (2 * pa, 2 * pa), None, copy(plane, na)),
        ("(a) CROSS5 (general kernel: the A/B)", (2 * pa, 2 * pa), 0, stencil(plane, na, X, False)),
        ("(a) dense BOX9", (2 * pa, 2 * pa), 0, stencil(plane, na, B, False)),
        ("    grid_combine, 2 terms, planes", (3 * pa, 3 * pa), None, combine(plane, na)),
        ("(a) CROSS5 + rhs (general kernel: the A/B)", (3 * pa, 3 * pa), 3, stencil(plane, na, X, True)),
        ("(a) dense BOX9 + rhs", (3 * pa, 3 * pa), 3, stencil(plane, na, B, True)),
        ("(b) general CROSS5, the same planes", (2 * pa, 2 * pa), 0, stencil(plane, na, X, False, True)),
        ("(b) general BOX9", (2 * pa, 2 * pa), 0, stencil(plane, na, B, False, True)),
        ("(b) general CROSS5 + rhs", (3 * pa, 3 * pa), 3, stencil(plane, na, X, True, True)),
        ("(b) general BOX9 + rhs", (3 * pa, 3 * pa), 3, stencil(plane, na, B, True, True)),
        (f"    grid_copy hz -> hz of other {nb}^2 x 32 B", (16 * pb, 2 * pb), None, copy(hz, nb)),
        ("(c) hz CROSS5", (16 * pb, 2 * pb), 10, stencil(hz, nb, X, False)),
        ("(c) hz BOX9", (16 * pb, 2 * pb), 10, stencil(hz, nb, B, False)),
        ("    grid_combine, 2 terms, hz", (24 * pb, 3 * pb), None, combine(hz, nb)),
        ("(c) hz CROSS5 + rhs", (24 * pb, 3 * pb), 13, stencil(hz, nb, X, True)),
        ("(c) hz BOX9 + rhs", (24 * pb, 3 * pb), 13, stencil(hz, nb, B, True)),
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

    lines = [f"grid stencils on {torch.cuda.get_device_name(0)}: {args.repeats} interleaved rounds after {args.warmup} warm-up "
             "rounds, device events around every call",
             f"{'case':46s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'moved MiB':>10s} {'lines TB/s':>11s} "
             f"{'moved TB/s':>11s} {'of its yardstick':>17s}"]
    med = [statistics.median(t) for t in times]
    rate = [moved[0] / med[k] for k, (_, moved, _, _) in enumerate(cases)]
    for k, (name, moved, yardstick, _) in enumerate(cases):
        share = "        yardstick" if yardstick is None else f"{rate[k] / rate[yardstick]:17.2f}"
        lines.append(f"{name:46s} {med[k] * 1e3:10.4f} {min(times[k]) * 1e3:8.4f} {max(times[k]) * 1e3:8.4f} "
                     f"{moved[1] / 2 ** 20:10.1f} {rate[k] / 1e12:11.3f} {moved[1] / med[k] / 1e12:11.3f} {share}")
    lines.append("dense kernel against general kernel on the same planes (medians, general / dense):")
    for dense, general in ((2, 7), (5, 9)):
        lines.append(f"    {cases[dense][0][4:]:24s} {med[general] * 1e3:8.4f} ms / {med[dense] * 1e3:8.4f} ms = {med[general] / med[dense]:5.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as out:
            out.write(text)


if __name__ == "__main__":
    main()

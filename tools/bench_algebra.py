#!/usr/bin/env python3
"""Time the grid-algebra calls (ststhip_grid_combine / ststhip_grid_resample) on the shapes they were built for.

    python tools/bench_algebra.py [--repeats 15] [--warmup 3] [--out profiles/grid_algebra.txt]

The cases are interleaved: one round runs each of them once, between two device events on the stream; median, min and
max are over the rounds.  The yardsticks -- ststhip_grid_copy of a dense plane and of one member of AoS cells into the
same member of other cells -- run in the same rounds, and every case is reported as a fraction of its yardstick's rate.

  (a) combine with 1, 2 and 4 terms on 16384^2 f32 planes (destination and terms are planes of their own)
  (b) the same on hz (4 of 32 bytes) of 4608^2 FDTD cells; destination and terms are grids of their own
  (c) restrict 16384^2 -> 8192^2 and prolong 8192^2 -> 16384^2, f32 planes

"moved" = the bytes a call must move: every element read once and written once.  "lines" = the bytes of the 128-byte
cache lines the call touches; for planes the two are the same, for a member of 32-byte cells every line of every grid is
touched (8 x the elements).  The rates are lines per second, as in profiles/grid_regions.txt.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
        sys.exit("bench_algebra needs a GPU: a timing taken anywhere else says nothing")
    capi.init(0)
    dev = torch.device("cuda:0")
    lib = capi.load()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    na, nb = 16384 // args.scale, 4608 // args.scale
    nc = na // 2
    with torch.cuda.stream(stream):
        planes = [torch.rand(na * na, dtype=torch.float32, device=dev) for _ in range(5)]
        grids = [torch.rand(nb * nb * 8, dtype=torch.float32, device=dev) for _ in range(5)]
        coarse = torch.rand(nc * nc, dtype=torch.float32, device=dev)
    stream.synchronize()

    view = capi.grid_view
    plane = [view(p.data_ptr(), 4, na, na) for p in planes]
    hz = [view(g.data_ptr() + 8, 32, nb, nb) for g in grids]
    coefs = [0.1, -1.0, 0.7, 1.3]

    def combine(views, n, n_terms):
        desc = capi.grid_combine_desc(views[0], "<f4", [(coefs[k], views[1 + k]) for k in range(n_terms)], n, n)
        return lambda: capi.grid_combine([desc], s)

    copy_plane = capi.grid_copy_desc(plane[0], plane[1], 4, na, na)
    copy_member = capi.grid_copy_desc(hz[0], hz[1], 4, nb, nb)
    restrict = capi.grid_resample_desc(view(coarse.data_ptr(), 4, nc, nc), plane[1], "<f4", capi.RESTRICT_MEAN, nc, nc)
    prolong = capi.grid_resample_desc(plane[0], view(coarse.data_ptr(), 4, nc, nc), "<f4", capi.PROLONG_BILINEAR, nc, nc)

    pa, pb = 4 * na * na, 4 * nb * nb  # bytes of a plane, of a member
    # name, (bytes of cache lines touched, bytes that must move), yardstick, call
    cases = [
        ("    grid_copy 16384^2 f32 plane -> plane", (2 * pa, 2 * pa), None, lambda: capi.grid_copy([copy_plane], s)),
        ("(a) combine, 1 term, 16384^2 f32 planes", (2 * pa, 2 * pa), 0, combine(plane, na, 1)),
        ("(a) combine, 2 terms", (3 * pa, 3 * pa), 0, combine(plane, na, 2)),
        ("(a) combine, 4 terms", (5 * pa, 5 * pa), 0, combine(plane, na, 4)),
        ("    grid_copy hz -> hz of other 4608^2 x 32 B", (16 * pb, 2 * pb), None, lambda: capi.grid_copy([copy_member], s)),
        ("(b) combine, 1 term, hz of 4608^2 x 32 B", (16 * pb, 2 * pb), 4, combine(hz, nb, 1)),
        ("(b) combine, 2 terms", (24 * pb, 3 * pb), 4, combine(hz, nb, 2)),
        ("(b) combine, 4 terms", (40 * pb, 5 * pb), 4, combine(hz, nb, 4)),
        ("(c) restrict 16384^2 -> 8192^2 f32", (pa + pa // 4, pa + pa // 4), 0, lambda: capi.grid_resample([restrict], s)),
        ("(c) prolong 8192^2 -> 16384^2 f32", (pa + pa // 4, pa + pa // 4), 0, lambda: capi.grid_resample([prolong], s)),
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

    lines = [f"grid algebra on {torch.cuda.get_device_name(0)}: {args.repeats} interleaved rounds after {args.warmup} warm-up "
             "rounds, device events around every call",
             f"{'case':46s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'moved MiB':>10s} {'lines TB/s':>11s} "
             f"{'moved TB/s':>11s} {'of its copy':>12s}"]
    med = [statistics.median(t) for t in times]
    rate = [moved[0] / med[k] for k, (_, moved, _, _) in enumerate(cases)]
    for k, (name, moved, yardstick, _) in enumerate(cases):
        share = "   yardstick" if yardstick is None else f"{rate[k] / rate[yardstick]:12.2f}"
        lines.append(f"{name:46s} {med[k] * 1e3:10.4f} {min(times[k]) * 1e3:8.4f} {max(times[k]) * 1e3:8.4f} "
                     f"{moved[1] / 2 ** 20:10.1f} {rate[k] / 1e12:11.3f} {moved[1] / med[k] / 1e12:11.3f} {share}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as out:
            out.write(text)


if __name__ == "__main__":
    main()

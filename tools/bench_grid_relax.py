#!/usr/bin/env python3
"""Time ststhip_grid_relax beside the ststhip_grid_stencil call that touches the same cache lines.

    python tools/bench_grid_relax.py [--repeats 15] [--warmup 3] [--out profiles/grid_relax.txt]

The cases are interleaved: one round runs each of them once, between two device events on the stream; median, min and
max are over the rounds.  A half-sweep reads u and f and writes u, as a CROSS5 stencil with a right-hand side reads src
and f and writes dst: every line of the three grids once (a store of one colour still touches every 32-byte sector), so
that call on the same planes in the same rounds is the yardstick, and every relaxation is reported as its time over the
yardstick's.

  (a) 16384^2 f32 planes: one half-sweep with and without a right-hand side through the dense kernel and through the
      general kernel (STSTHIP_RELAX_GENERAL): the A/B of the two kernels; and a full sweep (two half-sweeps, one call)
  (b) hz (4 of 32 bytes) of 4608^2 FDTD cells, rhs hz_sum of the same cells, general kernel, beside the stencil from
      hz of other cells
  (c) 64 half-sweeps of 4096^2 f32 planes in one call and as 64 calls: what a call costs beyond its launches
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWITCH = "STSTHIP_RELAX_GENERAL"


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
        sys.exit("bench_grid_relax needs a GPU: a timing taken anywhere else says nothing")
    os.environ.pop(SWITCH, None)
    capi.init(0)
    dev = torch.device("cuda:0")
    lib = capi.load()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    na, nb, nc = 16384 // args.scale, 4608 // args.scale, 4096 // args.scale
    with torch.cuda.stream(stream):
        planes = [torch.rand(na * na, dtype=torch.float32, device=dev) - 0.5 for _ in range(3)]
        grids = [torch.rand(nb * nb * 8, dtype=torch.float32, device=dev) - 0.5 for _ in range(2)]
    stream.synchronize()

    plane = [capi.grid_view(p.data_ptr(), 4, na, na) for p in planes]
    small = [capi.grid_view(p.data_ptr(), 4, nc, nc) for p in planes]  # the first nc^2 elements as a plane of their own
    hz = [capi.grid_view(g.data_ptr() + 8, 32, nb, nb) for g in grids]
    hz_sum = capi.grid_view(grids[0].data_ptr() + 12, 32, nb, nb)
    # a contraction: the cells stay bounded however many rounds relax them in place
    taps = [0.26, 0.24, -0.03, 0.25, 0.27]
    nine = [0.0, taps[0], 0.0, taps[1], taps[2], taps[3], 0.0, taps[4], 0.0]

    def stencil(dst, src, rhs, n):
        desc = capi.grid_stencil_desc(dst, src, "<f4", capi.STENCIL_CROSS5, nine, n, n, halo=0.5, rhs=rhs, rhs_coef=0.25)
        return lambda: capi.grid_stencil([desc], s)

    def relax(u, rhs, n, half_sweeps=1, general=False, calls=1):
        desc = capi.grid_relax_desc(u, "<f4", taps, n, n, halo=0.5, rhs=rhs, rhs_coef=0.25, half_sweeps=half_sweeps)
        flipped = capi.grid_relax_desc(u, "<f4", taps, n, n, halo=0.5, rhs=rhs, rhs_coef=0.25, half_sweeps=half_sweeps,
                                       first_colour=1)

        def run():
            if general:
                os.environ[SWITCH] = "1"
            try:
                for k in range(calls):
                    capi.grid_relax([flipped if k % 2 else desc], s)
            finally:
                os.environ.pop(SWITCH, None)
        return run

    pa, pb, pc = 4 * na * na, 4 * nb * nb, 4 * nc * nc  # bytes of a plane, of a member, of a small plane
    # name, bytes of the 128-byte lines touched, yardstick (index) or None, half-sweeps, call
    cases = [
        (f"    grid_stencil CROSS5 + rhs, {na}^2 f32 planes", 3 * pa, None, 1, stencil(plane[1], plane[0], plane[2], na)),
        ("(a) half-sweep + rhs, dense kernel", 3 * pa, 0, 1, relax(plane[0], plane[2], na)),
        ("(a) half-sweep + rhs, general kernel", 3 * pa, 0, 1, relax(plane[0], plane[2], na, general=True)),
        ("(a) half-sweep, dense kernel", 2 * pa, 0, 1, relax(plane[0], None, na)),
        ("(a) half-sweep, general kernel", 2 * pa, 0, 1, relax(plane[0], None, na, general=True)),
        ("(a) full sweep + rhs (2 half-sweeps, one call)", 6 * pa, 0, 2, relax(plane[0], plane[2], na, 2)),
        # (hz and hz_sum share their lines: the stencil reads one grid's and writes the other's, the relaxation reads
        # and writes one grid's)
        (f"    grid_stencil CROSS5 + rhs, hz of {nb}^2 x 32 B", 16 * pb, None, 1, stencil(hz[1], hz[0], hz_sum, nb)),
        ("(b) half-sweep of hz, rhs hz_sum", 8 * pb, 6, 1, relax(hz[0], hz_sum, nb)),
        (f"(c) 64 half-sweeps + rhs of {nc}^2 f32, one call", 64 * 3 * pc, None, 64, relax(small[0], small[2], nc, 64)),
        ("(c) the same as 64 calls", 64 * 3 * pc, 8, 64, relax(small[0], small[2], nc, 1, calls=64)),
    ]
    start, stop = C.c_void_p(), C.c_void_p()
    capi.check(lib.ststhip_event_create(C.byref(start)), "event")
    capi.check(lib.ststhip_event_create(C.byref(stop)), "event")
    times = [[] for _ in cases]
    ms = C.c_float()
    for round_ in range(args.warmup + args.repeats):
        for k, case in enumerate(cases):
            capi.check(lib.ststhip_event_record(start, s), "event")
            case[4]()
            capi.check(lib.ststhip_event_record(stop, s), "event")
            capi.check(lib.ststhip_event_synchronize(stop), "event")
            capi.check(lib.ststhip_event_elapsed_ms(start, stop, C.byref(ms)), "event")
            if round_ >= args.warmup:
                times[k].append(ms.value * 1e-3)
    if not bool(torch.isfinite(planes[0]).all()) or not bool(torch.isfinite(grids[0]).all()):
        sys.exit("the relaxed cells are no longer finite")

    lines = [f"grid relaxation on {torch.cuda.get_device_name(0)}: {args.repeats} interleaved rounds after {args.warmup} warm-up "
             "rounds, device events around every call",
             f"{'case':52s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'lines MiB':>10s} {'lines TB/s':>11s} "
             f"{'ms per half-sweep':>18s} {'over its yardstick':>19s}"]
    med = [statistics.median(t) for t in times]
    for k, (name, touched, yardstick, halves, _) in enumerate(cases):
        per = med[k] / halves
        share = "          yardstick" if yardstick is None else f"{per / (med[yardstick] / cases[yardstick][3]):19.2f}"
        lines.append(f"{name:52s} {med[k] * 1e3:10.4f} {min(times[k]) * 1e3:8.4f} {max(times[k]) * 1e3:8.4f} "
                     f"{touched / 2 ** 20:10.1f} {touched / med[k] / 1e12:11.3f} {per * 1e3:18.4f} {share}")
    lines.append("general kernel against dense kernel on the same planes (medians, general / dense):")
    for dense, general in ((1, 2), (3, 4)):
        lines.append(f"    {cases[dense][0][4:].replace(', dense kernel', ''):24s} {med[general] * 1e3:8.4f} ms / "
                     f"{med[dense] * 1e3:8.4f} ms = {med[general] / med[dense]:5.2f}")
    lines.append(f"one half-sweep + rhs over the CROSS5 + rhs stencil of the same planes: {med[1] / med[0]:.2f} (dense), "
                 f"{med[2] / med[0]:.2f} (general)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as out:
            out.write(text)


if __name__ == "__main__":
    main()

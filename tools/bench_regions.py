#!/usr/bin/env python3
"""Time the grid-region calls (ststhip_grid_copy / _fill / _download) on the shapes they were built for.

    python tools/bench_regions.py [--repeats 15] [--warmup 3] [--out profiles/grid_regions.txt]

The cases are interleaved: one round runs each of them once, between two device events on the stream; median, min and
max are over the rounds.  Yardsticks run in the same rounds.

  (a) a whole 16384^2 f32 plane to a plane            against ststhip_memcpy_d2d of the same bytes
  (b) hz (4 of 32 bytes) of a 4608^2 AoS grid into a dense plane
  (c) one double of the 88-byte cells of a 4096^2 grid into a dense plane
  (d) (b) taking every 4th row and column
  (e) ststhip_grid_download of (b) and of (d) into pinned host memory, against ststhip_memcpy_d2h of the whole AoS grid
      (what a GridAccessor moves for the same frame)
  (f) a 3 x 3 fill of one member: events around the call, and the host's clock around call + synchronise

For (b)-(d): "lines" = bytes of the 128-byte cache lines the call touches (read and written) per second, "useful" = bytes
of the elements moved (read once, written once) per second.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

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
        sys.exit("bench_regions needs a GPU: a timing taken anywhere else says nothing")
    capi.init(0)
    dev = torch.device("cuda:0")
    lib = capi.load()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    na, nb, nc = 16384 // args.scale, 4608 // args.scale, 4096 // args.scale
    with torch.cuda.stream(stream):
        plane_a = torch.rand(na * na, dtype=torch.float32, device=dev)
        plane_to = torch.empty(na * na, dtype=torch.float32, device=dev)
        fdtd = torch.rand(nb * nb * 8, dtype=torch.float32, device=dev)
        hz = torch.empty(nb * nb, dtype=torch.float32, device=dev)
        conv = torch.rand(nc * nc * 11, dtype=torch.float64, device=dev)
        member = torch.empty(nc * nc, dtype=torch.float64, device=dev)
    stream.synchronize()
    pinned = C.c_void_p()
    capi.check(lib.ststhip_host_malloc(C.byref(pinned), nb * nb * 32), "ststhip_host_malloc")

    nd = -(-nb // 4)
    view = capi.grid_view
    desc = capi.grid_copy_desc
    a = desc(view(plane_to.data_ptr(), 4, na, na), view(plane_a.data_ptr(), 4, na, na), 4, na, na)
    b = desc(view(hz.data_ptr(), 4, nb, nb), view(fdtd.data_ptr() + 8, 32, nb, nb), 4, nb, nb)
    c = desc(view(member.data_ptr(), 8, nc, nc), view(conv.data_ptr() + 16, 88, nc, nc), 8, nc, nc)
    d = desc(view(hz.data_ptr(), 4, nd, nd), view(fdtd.data_ptr() + 8, 32, nb, nb), 4, nd, nd, step=(4, 4))
    eb = desc(view(pinned.value, 4, nb, nb), view(fdtd.data_ptr() + 8, 32, nb, nb), 4, nb, nb)
    ed = desc(view(pinned.value, 4, nd, nd), view(fdtd.data_ptr() + 8, 32, nb, nb), 4, nd, nd, step=(4, 4))
    f = capi.grid_fill_desc(view(fdtd.data_ptr() + 8, 32, nb, nb), b"\0\0\x80\x3f", 3, 3, dst_at=(nb // 2, nb // 2))

    def d2d():
        capi.check(lib.ststhip_memcpy_d2d(plane_to.data_ptr(), plane_a.data_ptr(), 4 * na * na, s), "copy")

    def d2h():
        capi.check(lib.ststhip_memcpy_d2h(pinned, fdtd.data_ptr(), 32 * nb * nb, s), "copy")

    # name, (bytes of cache lines touched, useful bytes) or None, call
    cases = [
        ("(a) grid_copy 16384^2 f32 plane -> plane", (8 * na * na, 8 * na * na), lambda: capi.grid_copy([a], s)),
        ("    memcpy_d2d of (a)'s bytes", (8 * na * na, 8 * na * na), d2d),
        ("(b) hz of 4608^2 x 32 B -> plane", (36 * nb * nb, 8 * nb * nb), lambda: capi.grid_copy([b], s)),
        ("(c) a double of 4096^2 x 88 B -> plane", (96 * nc * nc, 16 * nc * nc), lambda: capi.grid_copy([c], s)),
        ("(d) (b) every 4th row and column", (132 * nd * nd, 8 * nd * nd), lambda: capi.grid_copy([d], s)),
        ("(e) grid_download of (b), pinned", (36 * nb * nb, 4 * nb * nb), lambda: capi.grid_download([eb], s)),
        ("(e) grid_download of (d), pinned", (132 * nd * nd, 4 * nd * nd), lambda: capi.grid_download([ed], s)),
        ("    memcpy_d2h of the whole AoS grid", (32 * nb * nb, 32 * nb * nb), d2h),
        ("(f) grid_fill 3 x 3 of a member", None, lambda: capi.grid_fill([f], s)),
    ]
    start, stop = C.c_void_p(), C.c_void_p()
    capi.check(lib.ststhip_event_create(C.byref(start)), "event")
    capi.check(lib.ststhip_event_create(C.byref(stop)), "event")
    times = {name: [] for name, _, _ in cases}
    fill_host = []
    ms = C.c_float()
    for round_ in range(args.warmup + args.repeats):
        for name, _, run in cases:
            capi.check(lib.ststhip_event_record(start, s), "event")
            run()
            capi.check(lib.ststhip_event_record(stop, s), "event")
            capi.check(lib.ststhip_event_synchronize(stop), "event")
            capi.check(lib.ststhip_event_elapsed_ms(start, stop, C.byref(ms)), "event")
            if round_ >= args.warmup:
                times[name].append(ms.value * 1e-3)
        began = time.perf_counter()
        capi.grid_fill([f], s)
        capi.check(lib.ststhip_stream_synchronize(s), "sync")
        if round_ >= args.warmup:
            fill_host.append(time.perf_counter() - began)

    lines = [f"grid regions on {torch.cuda.get_device_name(0)}: {args.repeats} interleaved rounds after {args.warmup} warm-up rounds, "
             "device events around every call",
             f"{'case':44s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'lines TB/s':>11s} {'useful TB/s':>12s}"]
    med = {name: statistics.median(t) for name, t in times.items()}
    for name, moved, _ in cases:
        t = times[name]
        rates = f"{moved[0] / med[name] / 1e12:11.3f} {moved[1] / med[name] / 1e12:12.3f}" if moved else ""
        lines.append(f"{name:44s} {med[name] * 1e3:10.4f} {min(t) * 1e3:8.4f} {max(t) * 1e3:8.4f} {rates}")
    lines.append(f"{'(f) host clock, call + synchronise':44s} {statistics.median(fill_host) * 1e3:10.4f} "
                 f"{min(fill_host) * 1e3:8.4f} {max(fill_host) * 1e3:8.4f}")
    names = [name for name, _, _ in cases]
    lines.append(f"(a) / memcpy_d2d = {med[names[0]] / med[names[1]]:.2f}   download of (b) / whole-grid d2h = "
                 f"{med[names[5]] / med[names[7]]:.3f}   download of (d) / whole-grid d2h = {med[names[6]] / med[names[7]]:.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as out:
            out.write(text)
    capi.check(lib.ststhip_host_free(pinned), "ststhip_host_free")


if __name__ == "__main__":
    main()

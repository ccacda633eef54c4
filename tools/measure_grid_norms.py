#!/usr/bin/env python3
"""Time ststhip_grid_norms / ststhip_grid_distance against ststhip_reduce_max_abs and a device-to-device copy.

    python tools/measure_grid_norms.py [--repeats 15] [--warmup 3] [--out profiles/grid_norms.txt]

Every call blocks until its numbers are on the host, so a host clock around the call is the time a caller waits
(kernels, the copy of the results and the synchronise).  The cases are interleaved: one round runs each of them once,
and median / min / max are over the rounds.  Rates are bytes of the grids read per second; the copy of as many bytes
(read once, written once) is timed in the same rounds and is what the fractions refer to.

  (a) ststhip_reduce_max_abs, 16384^2 f32            (b) grid norms of the same grid as a plane
  (c) distance of two such grids                      (d) both fields of an 8192^2 HotSpot AoS grid
  (e) two f64 fields of an 88-byte cell at 4096^2 (the cells' cache lines are all touched: the grid's bytes count)
"""
import argparse
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
        sys.exit("measure_grid_norms needs a GPU: a timing taken anywhere else says nothing")
    capi.init(0)
    dev = torch.device("cuda:0")
    lib = capi.load()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    n1, n2, n3 = 16384 // args.scale, 8192 // args.scale, 4096 // args.scale
    with torch.cuda.stream(stream):
        a = torch.rand(n1 * n1, dtype=torch.float32, device=dev) - 0.5
        b = torch.rand(n1 * n1, dtype=torch.float32, device=dev) - 0.5
        hot = torch.rand(n2 * n2 * 2, dtype=torch.float32, device=dev)
        conv = torch.rand(n3 * n3 * 11, dtype=torch.float64, device=dev)
        spare = torch.empty(2 * n1 * n1, dtype=torch.float32, device=dev)
    stream.synchronize()

    def copy_of(src_ptr, n_bytes):
        def run():
            capi.check(lib.ststhip_memcpy_d2d(spare.data_ptr(), src_ptr, n_bytes, s), "copy")
            capi.check(lib.ststhip_stream_synchronize(s), "sync")
        return run

    # (c) reads two buffers; its copy moves a and b, one after the other, in one timed step
    def copy_two():
        capi.check(lib.ststhip_memcpy_d2d(spare.data_ptr(), a.data_ptr(), 4 * n1 * n1, s), "copy")
        capi.check(lib.ststhip_memcpy_d2d(spare.data_ptr() + 4 * n1 * n1, b.data_ptr(), 4 * n1 * n1, s), "copy")
        capi.check(lib.ststhip_stream_synchronize(s), "sync")

    plane = capi.norm_field(a.data_ptr(), "<f4", 4, n1, n1)
    hot_fields = [capi.norm_field(hot.data_ptr() + o, "<f4", 8, n2, n2) for o in (0, 4)]
    conv_fields = [capi.norm_field(conv.data_ptr() + 8 * k, "<f8", 88, n3, n3) for k in (2, 9)]
    gib1, gib_hot, gib_conv = 4 * n1 * n1, 8 * n2 * n2, 88 * n3 * n3
    cases = [
        ("(a) reduce_max_abs 16384^2 f32", gib1, lambda: capi.reduce_max_abs(a.data_ptr(), 4, n1, n1, [(0, "f4", n1, n1)], stream=s)),
        ("(b) grid_norms 16384^2 f32 plane", gib1, lambda: capi.grid_norms([plane], stream=s)),
        ("    copy of (a)/(b)'s bytes", gib1, copy_of(a.data_ptr(), gib1)),
        ("(c) grid_distance of two 16384^2 f32", 2 * gib1, lambda: capi.grid_norms([plane], [b.data_ptr()], stream=s)),
        ("    copy of (c)'s bytes", 2 * gib1, copy_two),
        ("(d) grid_norms 8192^2 HotSpot AoS, 2 fields", gib_hot, lambda: capi.grid_norms(hot_fields, stream=s)),
        ("    copy of (d)'s bytes", gib_hot, copy_of(hot.data_ptr(), gib_hot)),
        ("(e) grid_norms 4096^2 88-byte cells, 2 f64 fields", gib_conv, lambda: capi.grid_norms(conv_fields, stream=s)),
        ("    copy of (e)'s bytes", gib_conv, copy_of(conv.data_ptr(), gib_conv)),
    ]
    times = {name: [] for name, _, _ in cases}
    for round_ in range(args.warmup + args.repeats):
        for name, _, run in cases:
            started = time.perf_counter()
            run()
            elapsed = time.perf_counter() - started
            if round_ >= args.warmup:
                times[name].append(elapsed)

    name_of = torch.cuda.get_device_name(0)
    lines = [f"grid norms on {name_of}: {args.repeats} interleaved rounds after {args.warmup} warm-up rounds, host clock around "
             "blocking calls",
             f"{'case':52s} {'MiB read':>9s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'TB/s':>7s} {'of copy':>8s}"]
    med = {name: statistics.median(t) for name, t in times.items()}
    copy_for = {}  # case -> the copy of its bytes: the next copy in the list
    for i, (name, _, _) in enumerate(cases):
        if not name.startswith("    copy"):
            copy_for[name] = next(other for other, _, _ in cases[i:] if other.startswith("    copy"))
    for name, n_bytes, _ in cases:
        t = times[name]
        rate = n_bytes / med[name] / 1e12
        frac = ""
        ref = copy_for.get(name)
        if ref:
            frac = f"{med[ref] / med[name]:8.2f}"
        lines.append(f"{name:52s} {n_bytes / 2**20:9.0f} {med[name] * 1e3:10.3f} {min(t) * 1e3:8.3f} {max(t) * 1e3:8.3f} {rate:7.2f} {frac:>8s}")
    lines.append(f"(b) / (a) = {med[cases[1][0]] / med[cases[0][0]]:.2f}   (c) / (b) = {med[cases[3][0]] / med[cases[1][0]]:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

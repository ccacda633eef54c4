"""The pass driver (ststhip_run_passes) with an instrumented sweep callback.

Every whole-grid result comes out of that driver: it cuts the generations into launch depths, ping-pongs between the
target and scratch planes, advances row strips on separate streams, runs tiles behind a source that is still arriving
and, on the first long call for a grid shape, times two depths against each other.  The other tests see its end
product with whatever timing the machine produced.  Here the driver gets a callback that RECORDS what it is asked for,
performs the real launch through ststhip_app_sweep and can make chosen launches late on their stream (a device-side
wait enqueued behind the launch), so that
  * the schedule is checked as a schedule (tests/pass_schedule.py: I1 chain ... I7 values table),
  * the winner of the depth probe is chosen by the test, both ways, and
  * a missing dependency between streams has a launch to be late for.
Every run is also compared with the oracle, bit for bit."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest

from pass_schedule import Launch, assert_launch_state_idle, check_schedule, check_tile_frontiers, halvings
from sweep_workloads import Workload

pytestmark = pytest.mark.gpu

BIG = (2048, 1024)          # the smallest grid the existing tests run in two and three strips and in eight blocks
_keys = itertools.count(0x7E57_0001)   # a fresh tune_key per probing case: nothing depends on the order of the tests


@pytest.fixture(scope="module", autouse=True)
def file_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[pass driver] tests/test_pass_driver_gpu.py took {time.perf_counter() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------ workloads
# (the class lives in tests/sweep_workloads.py, shared with the tests of single launches)
_workloads = {}


@pytest.fixture
def workload(gpu, oracle):
    def get(app, shape):
        if (app, shape) not in _workloads:
            _workloads[(app, shape)] = Workload(oracle, app, shape)
        return _workloads[(app, shape)]
    return get


# ------------------------------------------------------------------------------------------------ the delay
class Delay:
    """A device-side wait of `ms` milliseconds enqueued on a stream handle (torch.cuda._sleep spins for a number of
    clock ticks; how many a millisecond has is measured once).  No host sleep, no launch of the library."""

    ticks_per_ms = None
    _streams = {}

    @classmethod
    def calibrate(cls):
        import torch

        if cls.ticks_per_ms is None:
            s = torch.cuda.Stream()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                cls._spin(1000)  # (first use)
                t0.record()
                cls._spin(2_000_000)
                t1.record()
            t1.synchronize()
            cls.ticks_per_ms = 2_000_000 / max(t0.elapsed_time(t1), 1e-3)
        return cls.ticks_per_ms

    @staticmethod
    def _spin(ticks):
        import torch

        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(int(ticks))
        else:  # a fixed large op: one "tick" = 1e-5 of a 2048^2 matrix product, so nothing under 100 000 ticks is
            # told apart (the ticks per millisecond are measured either way).  Never run: this torch has _sleep.
            a = torch.ones(2048, 2048, device="cuda")
            for _ in range(max(1, int(ticks) // 100_000)):
                a = (a @ a).clamp_(max=1.0)

    def __init__(self, ms):
        self.ms = ms
        self.ticks = int(ms * self.calibrate())

    def on(self, stream_handle):
        import torch

        if stream_handle not in self._streams:
            self._streams[stream_handle] = torch.cuda.ExternalStream(stream_handle)
        with torch.cuda.stream(self._streams[stream_handle]):
            self._spin(self.ticks)

    def measured_ms(self):
        import torch

        s = torch.cuda.Stream()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(s)
        self.on(s.cuda_stream)
        t1.record(s)
        t1.synchronize()
        return t0.elapsed_time(t1)


_delays = {}


def delay_for(w):
    """Ten launches of the deepest depth at the workload's shape, 1 ms at least: a delayed launch finishes after several
    later launches on other streams would have."""
    key = (w.app, w.shape)
    if key not in _delays:
        launch = w.launch_ms()
        d = Delay(max(10.0 * launch, 1.0))
        got = d.measured_ms()
        print(f"\n[pass driver] {w.app} {w.shape[0]}x{w.shape[1]}: one launch of {w.info.max_generations} generations "
              f"{launch:.3f} ms, delay asked {d.ms:.3f} ms, measured {got:.3f} ms")
        assert got >= 0.5 * d.ms, "the device-side wait is much shorter than asked for"
        _delays[key] = d
    return _delays[key]


# ------------------------------------------------------------------------------------------------ one recorded call
class Run:
    def __init__(self, w, n, offset, launches, info, planes):
        self.w, self.n, self.offset, self.launches, self.info, self.planes = w, n, offset, launches, info, planes
        self.streams = sorted({l.stream for l in launches})

    def check(self, allowed=None, expect_tdv=False):
        """The schedule's invariants, and the cells against the oracle's."""
        w = self.w
        passes = check_schedule(self.launches, w.shape[0], w.info.n_planes, [t.data_ptr() for t in w.src],
                                [t.data_ptr() for t in w.dst], self.offset, self.n, w.info.halo_depth_per_generation,
                                allowed if allowed is not None else halvings(w.info.max_generations),
                                expect_tdv=expect_tdv)
        for got, want in zip(self.planes, w.want(self.n)):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
                f"{w.app} {w.shape}, {self.n} generations from {self.offset}: cells differ from the oracle's"
        return passes


def record(w, desc, n, offset=0, late=None, delay=None, src_ptrs=None):
    """One ststhip_run_passes call whose launches are recorded, performed by ststhip_app_sweep with exactly the
    arguments the driver gave, and -- where late(launch, pass index) says so -- followed by the delay on their
    stream."""
    import torch

    from stencilstream_amd import capi

    launches, seen = [], {}
    for t in w.dst:
        t.fill_(float("nan"))
    torch.cuda.synchronize()

    def sweep(dom, src, dst, out_begin, out_end, iteration, depth, stream):
        l = Launch(order=len(launches), iteration=iteration, n_generations=depth, out_row_begin=out_begin,
                   out_row_end=out_end, hole=capi.launch_row_hole(), src=src, dst=dst, stream=stream,
                   target_holds_constants=capi.target_holds_constants(), concurrency=capi.launch_concurrency(),
                   tdv=capi.current_tdv_table())
        launches.append(l)
        capi.app_sweep(w.app, w.params, w.halo, dom, src, dst, out_begin, out_end, iteration, depth, stream)
        if late is not None and late(l, seen.setdefault(iteration, len(seen))):
            delay.on(stream)

    info = capi.run_passes(sweep, desc, w.dom, src_ptrs or [t.data_ptr() for t in w.src], [t.data_ptr() for t in w.dst],
                           offset, n, blocking=True, stream=w.stream.cuda_stream)
    torch.cuda.synchronize()
    assert info.n_launches == len(launches)
    return Run(w, n, offset, launches, info, [t.cpu().numpy() for t in w.dst])


SCHEMES = {
    # name: (STSTHIP_SKEWED_STRIPS, STSTHIP_BANDS_BESIDE_INTERIOR)
    "moving": ("1", "1"),
    "bands_beside": ("0", "1"),
    "bands_in_line": ("0", "0"),
}


def set_scheme(monkeypatch, strips, scheme=None):
    monkeypatch.setenv("STSTHIP_VIRTUAL_STRIPS", str(strips))
    monkeypatch.setenv("STSTHIP_NARROW_FORM_KCELLS", "0")
    if scheme:
        monkeypatch.setenv("STSTHIP_SKEWED_STRIPS", SCHEMES[scheme][0])
        monkeypatch.setenv("STSTHIP_BANDS_BESIDE_INTERIOR", SCHEMES[scheme][1])


def assert_scheme(run, strips, scheme, n_passes):
    """The scheme the case is about is the one that ran (calls of three passes and more)."""
    if scheme == "moving":
        assert len(run.launches) == strips * n_passes and len(run.streams) == strips
    elif scheme == "bands_beside":
        assert len(run.launches) > strips * n_passes and len(run.streams) == 2 * strips
    else:
        assert len(run.launches) > strips * n_passes and len(run.streams) == strips
    assert {l.concurrency for l in run.launches} == {strips}


# ------------------------------------------------------------------------------------------------ a. no probe
ONE_STRIP = [("jacobi5general", (257, 511)), ("hotspot", (300, 200))]
GENERATIONS = [0, 1, 5, 37, 95]


@pytest.mark.parametrize("n", GENERATIONS)
@pytest.mark.parametrize("app,shape", ONE_STRIP, ids=["jacobi", "hotspot"])
def test_one_strip_schedules(workload, monkeypatch, app, shape, n):
    set_scheme(monkeypatch, 1)
    w = workload(app, shape)
    for offset in (0, 7):
        run = record(w, w.desc(), n, offset)
        passes = run.check()
        assert len(run.launches) == len(passes) and run.info.n_streamed_passes == 0
        if app == "hotspot" and n == 95:
            assert [d for _, d, _ in passes] == [12] * 7 + [6, 3, 1, 1]  # the family of 12 / 6 / 3 / 1


@pytest.mark.parametrize("n", GENERATIONS)
@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("strips", [2, 3])
@pytest.mark.parametrize("app", ["jacobi5general", "hotspot"], ids=["jacobi", "hotspot"])
def test_strip_schedules(workload, monkeypatch, app, strips, scheme, n):
    set_scheme(monkeypatch, strips, scheme)
    w = workload(app, BIG)
    for offset in (0, 7):
        run = record(w, w.desc(), n, offset)
        passes = run.check()
        if n >= 37:
            assert_scheme(run, strips, scheme, len(passes))


@pytest.mark.parametrize("strips", [2, 3])
def test_moving_boundaries_start_over(workload, monkeypatch, strips):
    """700 generations move the boundaries further than their span: they start over in the middle of the call, the one
    pass in which every strip also waits for the one below it.  I4 and I5 hold across it."""
    set_scheme(monkeypatch, strips, "moving")
    w = workload("jacobi5general", BIG)
    run = record(w, w.desc(), 700)
    passes = run.check()
    assert_scheme(run, strips, "moving", len(passes))
    # the boundary below the first strip moves up pass by pass and jumps back down at least once
    ends = [min(l.out_row_end for l in group) for _, _, group in passes]
    assert any(b > a for a, b in zip(ends, ends[1:])), "the boundaries never started over"
    assert any(b < a for a, b in zip(ends, ends[1:]))


def test_values_table_of_the_call(workload, monkeypatch):
    """I7: a description with host-side time-dependent values: one device table per call, generations offset ... + n,
    visible to every launch of two strips."""
    from stencilstream_amd import capi

    set_scheme(monkeypatch, 2, "moving")
    w = workload("jacobi5general", BIG)
    asked = []

    def fill(_ctx, offset, n, values):
        asked.append((offset, n))
        table = (C.c_uint64 * n).from_address(values)
        for i in range(n):
            table[i] = offset + i

    desc, fill_fn = w.desc(), capi.FILL_TDV_FN(fill)
    desc.tdv_size = 8
    desc.fill_tdv = fill_fn
    run = record(w, desc, 37, 7)
    run.check(expect_tdv=True)
    assert asked == [(7, 37)]
    assert {l.tdv[1:] for l in run.launches} == {(7, 37, 8)} and len({l.tdv[0] for l in run.launches}) == 1


def test_launch_state_is_idle_after_a_call(workload, monkeypatch):
    """Whichever way a call leaves the driver -- done, refused, or ended by its callback -- the calling thread's launch
    state is idle afterwards: one launch at a time, no constants in the target, no row hole, no values table."""
    import torch

    from stencilstream_amd import capi

    set_scheme(monkeypatch, 2, "moving")
    w = workload("hotspot", BIG)
    run = record(w, w.desc(), 37)
    assert {l.concurrency for l in run.launches} == {2} and any(l.target_holds_constants for l in run.launches)
    assert_launch_state_idle(capi)

    w = workload("jacobi5general", BIG)
    desc, fill_fn = w.desc(), capi.FILL_TDV_FN(lambda _ctx, offset, n, values: None)
    desc.tdv_size = 8
    desc.fill_tdv = fill_fn
    run = record(w, desc, 37, 7)
    assert all(l.tdv[0] != 0 and l.tdv[1:] == (7, 37, 8) for l in run.launches)
    assert_launch_state_idle(capi)

    # refused: a second depth the sweep is not compiled for
    with pytest.raises(capi.StsthipError):
        record(w, w.desc(6, next(_keys)), 37)
    assert_launch_state_idle(capi)

    # the callback raises on its third launch (the two before it are real launches)
    seen = []

    def sweep(dom, src, dst, out_begin, out_end, iteration, depth, stream):
        seen.append((capi.launch_concurrency(), capi.current_tdv_table()[0]))
        if len(seen) == 3:
            raise RuntimeError("third launch")
        capi.app_sweep(w.app, w.params, w.halo, dom, src, dst, out_begin, out_end, iteration, depth, stream)

    with pytest.raises(RuntimeError, match="third launch"):
        capi.run_passes(sweep, desc, w.dom, [t.data_ptr() for t in w.src], [t.data_ptr() for t in w.dst], 0, 37,
                        blocking=True, stream=w.stream.cuda_stream)
    torch.cuda.synchronize()
    assert len(seen) == 3 and all(c == 2 and base != 0 for c, base in seen)
    assert_launch_state_idle(capi)


# ------------------------------------------------------------------------------------------------ b. the probe
PROBES = [
    # app, shape, deep, alt, generations
    ("jacobi5general", (257, 511), 16, 8, 96),    # the plans' parities differ: one pass of 8 becomes two of 4
    ("jacobi5general", (257, 511), 16, 8, 203),   # the same with a ragged tail
    ("jacobi5general", (257, 511), 16, 8, 112),   # no split
    ("jacobi5general", (257, 511), 16, 8, 117),
    ("hotspot", (300, 200), 12, 6, 72),           # split: 6 -> 3 + 3
    ("hotspot", (300, 200), 12, 6, 84),           # no split
    ("hotspot", (300, 200), 12, 3, 72),           # a pass of 3 cannot be split (1 + 1 loses a generation): 12 -> 6 + 6
    ("hotspot", (300, 200), 12, 3, 78),
]


def steered(w, deep, alt, n, winner, key, offset=0):
    """A call with a second depth in which every launch of the depth that is to LOSE is late: the delay lies behind
    the launch on its stream, inside the probe's fences."""
    loser = deep if winner == alt else alt
    return record(w, w.desc(alt, key), n, offset, late=lambda l, p: l.n_generations == loser, delay=delay_for(w))


@pytest.mark.parametrize("winner", ["alt", "deep"])
@pytest.mark.parametrize("app,shape,deep,alt,n", PROBES, ids=[f"{p[0]}-{p[2]}-{p[3]}-n{p[4]}" for p in PROBES])
def test_depth_probe_with_a_chosen_winner(workload, monkeypatch, app, shape, deep, alt, n, winner):
    from stencilstream_amd import capi

    set_scheme(monkeypatch, 1)
    w = workload(app, shape)
    assert w.info.max_generations == deep
    key, H, W = next(_keys), *shape
    winner = alt if winner == "alt" else deep
    assert capi.tuned_depth(key, H, W) == 0
    run = steered(w, deep, alt, n, winner, key)
    tuned = capi.tuned_depth(key, H, W)
    passes = run.check()
    depths = [d for _, d, _ in passes]
    print(f"\n[pass driver] {app} {deep}/{alt}, {n} generations, steered to {winner}: ststhip_tuned_depth = {tuned}, "
          f"depths {depths}")
    assert tuned == winner, "the probe was not steered"
    assert depths[:3 + 2 * (deep // alt)] == [deep] * 3 + [alt] * (2 * (deep // alt))
    # (what follows the probes is the winner's plan; a pass of either plan may have been halved for the parity)
    assert (max(depths[3 + 2 * (deep // alt):]) <= alt) == (winner == alt)
    # the call after it looks the depth up
    again = record(w, w.desc(alt, key), n, 7)
    later = again.check(halvings(deep, cap=winner))
    assert later[0][1] == winner and capi.tuned_depth(key, H, W) == winner


@pytest.mark.parametrize("winner", [8, 16])
def test_depth_probe_with_moving_boundaries(workload, monkeypatch, winner):
    from stencilstream_amd import capi

    set_scheme(monkeypatch, 2, "moving")
    w = workload("jacobi5general", BIG)
    key = next(_keys)
    run = steered(w, 16, 8, 203, winner, key)
    passes = run.check()
    assert capi.tuned_depth(key, *BIG) == winner, "the probe was not steered"
    assert_scheme(run, 2, "moving", len(passes))
    again = record(w, w.desc(8, key), 203, 7)
    again.check(halvings(16, cap=winner))


@pytest.mark.parametrize("app,deep,alt", [("hotspot", 12, 4), ("jacobi5general", 16, 6), ("hotspot", 12, 24)])
def test_second_depth_that_is_not_compiled_is_refused(workload, monkeypatch, app, deep, alt):
    """alt_generations must be a repeated halving of max_generations: 12 / 4 passed `deep % alt == 0` and put launches
    of four generations into the plan of a probing call."""
    from stencilstream_amd import capi

    set_scheme(monkeypatch, 1)
    w = workload(app, dict(ONE_STRIP)[app])
    assert w.info.max_generations == deep
    for n in (5, 6 * deep):
        with pytest.raises(capi.StsthipError) as e:
            record(w, w.desc(alt, next(_keys)), n)
        assert e.value.status == 2 and "alt_generations" in str(e.value)


# ------------------------------------------------------------------------------------------------ c. late launches
def late_runs(w, make_desc, n, check):
    """An undelayed run names the streams; then one run per stream with every launch on it late, and one with the
    launches of the odd passes late.  Each must pass `check`."""
    delay = delay_for(w)
    plain = record(w, make_desc(), n)
    check(plain)
    assert len(plain.streams) >= 2
    for stream in plain.streams:
        run = record(w, make_desc(), n, late=lambda l, p: l.stream == stream, delay=delay)
        assert run.streams == plain.streams
        check(run)
    check(record(w, make_desc(), n, late=lambda l, p: p % 2 == 1, delay=delay))


@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("strips", [2, 3])
def test_late_launches_in_row_strips(workload, monkeypatch, strips, scheme):
    set_scheme(monkeypatch, strips, scheme)
    w = workload("jacobi5general", BIG)
    late_runs(w, w.desc, 95, lambda run: assert_scheme(run, strips, scheme, len(run.check())))


def test_late_launches_while_the_depth_is_probed(workload, monkeypatch):
    """Two strips with moving boundaries in calls that probe (a fresh key each): whichever depth the delays let win."""
    from stencilstream_amd import capi

    set_scheme(monkeypatch, 2, "moving")
    w = workload("jacobi5general", BIG)
    keys = []

    def make_desc():
        keys.append(next(_keys))
        return w.desc(8, keys[-1])

    def check(run):
        run.check()
        assert capi.tuned_depth(keys[-1], *BIG) in (8, 16), "the call did not probe"

    late_runs(w, make_desc, 203, check)


# ------------------------------------------------------------------------------------------------ d. an arriving source
def record_behind_upload(w, desc, n, blocks=8, late=None, delay=None):
    """The source uploaded in row blocks on the runtime's upload stream; the recorded call follows them."""
    import torch

    from stencilstream_amd import capi

    H, W = w.shape
    pinned = [torch.from_numpy(p.reshape(-1)).pin_memory() for p in w.host]
    arriving = [torch.zeros_like(t) for t in w.src]
    torch.cuda.synchronize()
    events = capi.upload_in_blocks([(pin.data_ptr(), d.data_ptr(), W * p.itemsize)
                                    for pin, d, p in zip(pinned, arriving, w.host)], H, n_blocks=blocks)
    try:
        run = record(w, desc, n, late=late, delay=delay, src_ptrs=[t.data_ptr() for t in arriving])
    finally:
        torch.cuda.synchronize()
        capi.events_destroy(events)
    return run, [t.data_ptr() for t in arriving]


def check_behind_upload(run, src_ptrs):
    w = run.w
    allowed = halvings(w.info.max_generations)
    check_schedule(run.launches, w.shape[0], 1, src_ptrs, [t.data_ptr() for t in w.dst], 0, run.n, 1, allowed)
    check_tile_frontiers(run.launches, w.shape[0], 0, run.n, 1, allowed)
    assert run.info.n_streamed_passes >= 2, "the driver did not follow the blocks"
    assert np.array_equal(run.planes[0].view(np.uint32), w.want(run.n)[0].view(np.uint32))
    # the streamed passes are the call's first ones, produced in more than one tile each
    by_iteration = {}
    for l in run.launches:
        by_iteration.setdefault(l.iteration, []).append(l)
    tiled = [it for it in sorted(by_iteration) if len(by_iteration[it]) > 1]
    assert len(tiled) >= 2 and tiled == sorted(by_iteration)[:len(tiled)]
    assert {l.concurrency for it in tiled for l in by_iteration[it]} == {2}


@pytest.mark.parametrize("n", [200, 40])
def test_tiles_behind_an_arriving_source(workload, monkeypatch, n):
    """2048 x 1024 in eight blocks: 200 generations probe behind the tiles, 40 do not.  I1-I6 over tiles and later
    passes together, the tiles' frontiers, and once more with every launch on the side stream late."""
    from stencilstream_amd import capi

    monkeypatch.setenv("STSTHIP_VIRTUAL_STRIPS", "1")
    monkeypatch.setenv("STSTHIP_NARROW_FORM_KCELLS", "0")
    w = workload("jacobi5general", BIG)
    key = next(_keys)
    run, src_ptrs = record_behind_upload(w, w.desc(8, key), n)
    check_behind_upload(run, src_ptrs)
    assert capi.tuned_depth(key, *BIG) in ((8, 16) if n == 200 else (0,))
    side = [s for s in run.streams if s != w.stream.cuda_stream]
    assert len(side) == 1, "the tiles ran on the caller's stream and one side stream"
    key = next(_keys)
    late, src_ptrs = record_behind_upload(w, w.desc(8, key), n, late=lambda l, p: l.stream == side[0],
                                          delay=delay_for(w))
    check_behind_upload(late, src_ptrs)


# ------------------------------------------------------------------------------------------------ e. stale arrival list
def test_arrival_list_does_not_outlive_a_refused_call(workload, monkeypatch):
    """Blocks named for a call that is refused before it reaches the pass driver (an unknown transition function) are
    gone with it: the thread's next call, on a grid that is in HBM, does not follow them."""
    import torch

    from stencilstream_amd import capi

    monkeypatch.setenv("STSTHIP_VIRTUAL_STRIPS", "1")
    w = workload("jacobi5general", BIG)
    lib = capi.load()
    H, n_blocks = BIG[0], 8
    up = capi.upload_stream()
    blocks, events = (capi.SourceBlock * n_blocks)(), []
    for b in range(n_blocks):
        ev = C.c_void_p()
        capi.check(lib.ststhip_event_create(C.byref(ev)), "ststhip_event_create")
        capi.check(lib.ststhip_event_record(ev, C.c_void_p(up)), "ststhip_event_record")
        events.append(ev)
        blocks[b].row_end, blocks[b].ready = H * (b + 1) // n_blocks, ev.value
    try:
        capi.check(lib.ststhip_set_source_arrival(blocks, n_blocks), "ststhip_set_source_arrival")
        src, dst = [t.data_ptr() for t in w.src], [t.data_ptr() for t in w.dst]
        with pytest.raises(capi.StsthipError) as e:
            capi.app_run("no_such_kernel", w.params, w.halo, w.dom, src, dst, 0, 40)
        assert e.value.status == 3
        for t in w.dst:
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        info = capi.app_run(w.app, w.params, w.halo, w.dom, src, dst, 0, 40, blocking=True,
                            stream=w.stream.cuda_stream)
        print(f"\n[pass driver] after a refused call with 8 blocks named: n_streamed_passes = {info.n_streamed_passes}")
        assert info.n_streamed_passes == 0, "a later call followed the blocks of a call that was refused"
        assert np.array_equal(w.dst[0].cpu().numpy().view(np.uint32), w.want(40)[0].view(np.uint32))
    finally:
        torch.cuda.synchronize()
        capi.events_destroy(events)

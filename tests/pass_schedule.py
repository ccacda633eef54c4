"""The pass driver's schedule, checked as a schedule (ststhip_run_passes, include/ststhip.h).

The driver takes its launch as a callback.  A test hands it one that records every launch it is asked for as a `Launch`
and hands the list to `check_schedule`, which knows nothing of the driver's code: only what any correct schedule of
whole-grid passes must look like.  Pure Python, no GPU, no library of its own (tests/test_pass_schedule.py proves on hand-made
schedules that it accepts correct ones and rejects each kind of wrong one).

I6 is checked row-wise, on purpose: a launch may be told that its target holds the constant fields if an earlier pass
of the call wrote the same planes (every pass covers all rows, I2) AND the launches of that pass which produced the
rows this launch writes were enqueued before it.  "The whole target was written before" in host order would refuse
the tiles behind an arriving source, whose third pass starts at the top while the first is still on its way down.
This rests on what the flag means to a sweep -- it leaves out the stores of constant fields of the rows it writes,
nothing else; the schedule cannot show that, the comparison of every run with the oracle does."""
from dataclasses import dataclass


class ScheduleError(AssertionError):
    """A schedule breaks an invariant; `invariant` is "I1" ... "I7" or "tiles", the message names the launch."""

    def __init__(self, invariant, message):
        super().__init__(f"{invariant}: {message}")
        self.invariant = invariant


@dataclass(frozen=True)
class Launch:
    """One call of the sweep callback, with the thread's launch state at that moment."""

    order: int                 # position in the order in which the host enqueued the launches
    iteration: int             # first generation the launch computes
    n_generations: int
    out_row_begin: int
    out_row_end: int
    hole: tuple = (0, 0)       # ststhip_launch_row_hole: rows [begin, end) the launch leaves out (empty: begin >= end)
    src: tuple = ()            # plane pointers read
    dst: tuple = ()            # plane pointers written
    stream: int = 0
    target_holds_constants: int = 0   # ststhip_target_holds_constants()
    concurrency: int = 1              # ststhip_launch_concurrency()
    tdv: tuple = (0, 0, 0, 0)  # ststhip_current_tdv_table: base, first_iteration, n_values, value_size

    def produced(self):
        """Row ranges the launch writes: its range minus the hole."""
        a, b = self.out_row_begin, self.out_row_end
        ha, hb = max(self.hole[0], a), min(self.hole[1], b)
        if ha >= hb:
            return [(a, b)] if a < b else []
        return [r for r in ((a, ha), (hb, b)) if r[0] < r[1]]

    def reads(self, g, height):
        """Row ranges the launch reads: what it produces, widened by g ghost rows, inside the grid."""
        return [(max(0, a - g), min(height, b + g)) for a, b in self.produced()]

    def __str__(self):
        hole = f" hole {self.hole}" if self.hole[0] < self.hole[1] else ""
        return (f"launch #{self.order} (generation {self.iteration} + {self.n_generations}, rows "
                f"[{self.out_row_begin}, {self.out_row_end}){hole}, stream {self.stream:#x})")


def assert_launch_state_idle(capi):
    """The calling thread's launch state between driver calls, read through `capi` (stencilstream_amd.capi): what every
    way out of ststhip_run_passes, ststhip_strip_advance and the block driver leaves behind."""
    assert capi.launch_concurrency() == 1
    assert capi.target_holds_constants() == 0
    assert capi.launch_row_hole() == (0, 0)
    base, _first, n_values, _size = capi.current_tdv_table()
    assert (base, n_values) == (0, 0)


def halvings(max_generations, cap=0):
    """max_generations and its repeated halvings, at most `cap` when that is set: the depths a sweep is compiled for."""
    out, t = set(), int(max_generations)
    while t >= 1:
        if not cap or t <= cap:
            out.add(t)
        t //= 2
    return out


def _overlap(r, s):
    return r[0] < s[1] and s[0] < r[1]


def passes_of(launches, iteration_offset, n_iterations, allowed_depths):
    """I1: the launches grouped into the passes of one chain of generations: [(iteration, depth, [launches])]."""
    by_iteration = {}
    for l in sorted(launches, key=lambda l: l.order):
        by_iteration.setdefault(l.iteration, []).append(l)
    passes, at = [], iteration_offset
    for iteration in sorted(by_iteration):
        group = by_iteration[iteration]
        depth = group[0].n_generations
        for l in group:
            if l.n_generations != depth:
                raise ScheduleError("I1", f"{l} has another depth than {group[0]} of the same pass")
            if l.n_generations not in allowed_depths:
                raise ScheduleError("I1", f"{l}: depth {l.n_generations} is not one of {sorted(allowed_depths)}")
        if iteration != at:
            what = "a gap" if iteration > at else "an overlap"
            raise ScheduleError("I1", f"{group[0]} starts at generation {iteration}, the chain is at {at}: {what}")
        at = iteration + depth
        passes.append((iteration, depth, group))
    advanced = at - iteration_offset
    if advanced != n_iterations:
        last = passes[-1][2][-1] if passes else "no launch"
        raise ScheduleError("I1", f"the passes advance {advanced} generations, not {n_iterations} (last: {last})")
    return passes


def check_schedule(launches, H, n_planes_ptrs, src, dst, iteration_offset, n_iterations, halo_depth_per_generation,
                   allowed_depths, expect_tdv=False):
    """Raise ScheduleError unless `launches` is a correct schedule of one ststhip_run_passes call over a grid of H rows
    with `n_planes_ptrs` planes from `src` to `dst` (tuples of plane pointers).  Returns the passes (see passes_of).

    I1 chain, I2 partition, I3 ping-pong, I4 read-after-write and I5 write-after-read in host order (necessary
    conditions: a producer that is enqueued after its consumer cannot be waited for), I6 constants, I7 values table."""
    src, dst = tuple(src), tuple(dst)
    launches = sorted(launches, key=lambda l: l.order)
    if n_iterations == 0:
        if launches:
            raise ScheduleError("I3", f"no generations, but {launches[0]}")
        return []
    passes = passes_of(launches, iteration_offset, n_iterations, set(allowed_depths))

    # I2: the produced rows of a pass cover [0, H) exactly once
    for iteration, depth, group in passes:
        at, before = 0, None
        for a, b, l in sorted((a, b, l) for l in group for a, b in l.produced()):
            if b > H:
                raise ScheduleError("I2", f"{l} produces rows beyond the grid's {H}")
            if a > at:
                raise ScheduleError("I2", f"rows [{at}, {a}) of the pass at generation {iteration} are produced by no "
                                          f"launch (next: {l})")
            if a < at:
                raise ScheduleError("I2", f"rows [{a}, {min(at, b)}) of the pass at generation {iteration} are "
                                          f"produced twice: by {before} and {l}")
            at, before = b, l
        if at < H:
            raise ScheduleError("I2", f"rows [{at}, {H}) of the pass at generation {iteration} are produced by no "
                                      f"launch")

    # I3: one source set and one other target set per pass, chained, ending in dst, src never written
    others = []
    for p, (iteration, depth, group) in enumerate(passes):
        first = group[0]
        for l in group:
            if len(l.src) != n_planes_ptrs or len(l.dst) != n_planes_ptrs:
                raise ScheduleError("I3", f"{l} names {len(l.src)} / {len(l.dst)} planes, not {n_planes_ptrs}")
            if l.src != first.src or l.dst != first.dst:
                raise ScheduleError("I3", f"{l} reads or writes other planes than {first} of the same pass")
            if set(l.dst) & set(src):
                raise ScheduleError("I3", f"{l} writes the call's source")
            if set(l.dst) & set(l.src):
                raise ScheduleError("I3", f"{l} writes planes it reads")
        want = src if p == 0 else passes[p - 1][2][0].dst
        if first.src != want:
            raise ScheduleError("I3", f"{first} of pass {p} does not read " +
                                      ("the call's source" if p == 0 else f"what pass {p - 1} wrote"))
        if first.dst != dst and first.dst not in others:
            others.append(first.dst)
    last = passes[-1][2][0]
    if last.dst != dst:
        raise ScheduleError("I3", f"{last} of the last pass does not write the call's target")
    if len(others) > 1:
        raise ScheduleError("I3", f"{len(others)} plane sets besides the source and the target are in use")

    for p, (iteration, depth, group) in enumerate(passes):
        g = depth * halo_depth_per_generation
        for l in group:
            # I4: what a launch reads was produced by launches of the pass before that were enqueued earlier
            if p >= 1:
                for r in l.reads(g, H):
                    for q in passes[p - 1][2]:
                        if q.order > l.order and any(_overlap(r, w) for w in q.produced()):
                            raise ScheduleError("I4", f"{l} reads rows [{r[0]}, {r[1]}) and was enqueued before their "
                                                      f"producer {q}")
            # I5: what a launch overwrites was read by launches of the pass before that were enqueued earlier
            if p >= 2 and l.dst == passes[p - 1][2][0].src:
                g_before = passes[p - 1][1] * halo_depth_per_generation
                for w in l.produced():
                    for q in passes[p - 1][2]:
                        if q.order > l.order and any(_overlap(w, r) for r in q.reads(g_before, H)):
                            raise ScheduleError("I5", f"{l} overwrites rows [{w[0]}, {w[1]}) and was enqueued before "
                                                      f"their reader {q}")
            # I6: the target holds the constant fields only if an earlier pass of the call stored all of it (I2), and
            # the rows this launch relies on before it
            if l.target_holds_constants:
                earlier = [q for q in range(p) if passes[q][2][0].dst == l.dst]
                if not earlier:
                    raise ScheduleError("I6", f"{l} is told that its target holds the constant fields, but no earlier "
                                              f"pass of the call wrote these planes")
                for w in l.produced():
                    for q in passes[earlier[-1]][2]:
                        if q.order > l.order and any(_overlap(w, v) for v in q.produced()):
                            raise ScheduleError("I6", f"{l} is told that its target holds the constant fields, but "
                                                      f"{q}, which stores them, was enqueued later")
            # I7: one table of time-dependent values for the whole call
            if expect_tdv and (not l.tdv[0] or l.tdv[1] != iteration_offset or l.tdv[2] != n_iterations):
                raise ScheduleError("I7", f"{l} sees a values table (base, first, count, size) = {l.tdv}, the call is "
                                          f"generations {iteration_offset} + {n_iterations}")
    return passes


def check_tile_frontiers(launches, H, iteration_offset, n_iterations, halo_depth_per_generation, allowed_depths):
    """Passes that run as row tiles behind a source that is still arriving: at every moment of the host's order the
    rows [0, frontier) a pass has produced end at least g rows above the frontier of the pass before (or that pass is
    complete), g = ghost rows of a launch."""
    passes = passes_of(launches, iteration_offset, n_iterations, set(allowed_depths))
    index = {iteration: p for p, (iteration, _, _) in enumerate(passes)}
    frontier, done = [0] * len(passes), [[] for _ in passes]
    for l in sorted(launches, key=lambda l: l.order):
        p = index[l.iteration]
        g = l.n_generations * halo_depth_per_generation
        done[p] = sorted(done[p] + l.produced())
        for a, b in done[p]:
            if a <= frontier[p]:
                frontier[p] = max(frontier[p], b)
        if p >= 1 and frontier[p - 1] < H and l.out_row_end + g > frontier[p - 1]:
            raise ScheduleError("tiles", f"{l} of pass {p} ends less than {g} rows above row {frontier[p - 1]}, which "
                                         f"is as far as pass {p - 1} has come")

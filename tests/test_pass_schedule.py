"""The schedule checker of tests/pass_schedule.py on schedules built by hand: it accepts correct ones (one strip, two
strips with bands and with moving boundaries, row tiles behind an arriving source) and rejects, each for its own
reason, the ways a pass driver can be wrong.  No GPU, no library: a checker that cannot fail proves nothing about the
driver it is pointed at in tests/test_pass_driver_gpu.py."""
import dataclasses

import pytest

from pass_schedule import Launch, ScheduleError, check_schedule, check_tile_frontiers, halvings

H = 2048
SRC, DST, SCRATCH = (0x1000,), (0x2000,), (0x3000,)


def plan_depths(n, deep, cap=0):
    """The driver's greedy plan: the deepest compiled depth that fits what is left (and the cap)."""
    cap = cap or deep
    out = []
    while n > 0:
        t = deep
        while t > 1 and (t > n or t > cap):
            t //= 2
        out.append(t)
        n -= t
    return out


def targets(n_passes):
    """The last pass writes DST, alternating backwards from there."""
    return [DST if (n_passes - 1 - k) % 2 == 0 else SCRATCH for k in range(n_passes)]


class Recorder:
    def __init__(self, depths, offset=0):
        self.depths, self.offset, self.launches = depths, offset, []
        self.to = targets(len(depths))

    def launch(self, p, a, b, stream=1, **more):
        self.launches.append(Launch(order=len(self.launches), iteration=self.offset + sum(self.depths[:p]),
                                    n_generations=self.depths[p], out_row_begin=a, out_row_end=b,
                                    src=SRC if p == 0 else self.to[p - 1], dst=self.to[p], stream=stream,
                                    target_holds_constants=1 if p >= 2 else 0, **more))


def one_strip(depths, offset=0):
    r = Recorder(depths, offset)
    for p in range(len(depths)):
        r.launch(p, 0, H)
    return r.launches


def two_strips_with_bands(depths):
    """Fixed strips: per pass and strip the band next to the neighbour, then the interior."""
    r, mid = Recorder(depths), H // 2
    for p, g in enumerate(depths):
        r.launch(p, mid - g, mid, stream=3)
        r.launch(p, 0, mid - g, stream=1)
        r.launch(p, mid, mid + g, stream=4)
        r.launch(p, mid + g, H, stream=2)
    return r.launches


def two_strips_with_a_moving_boundary(depths, shift_of, ahead=True):
    """The boundary moves up by shift_of(g of this pass, g of the pass before) per pass; with `ahead` the upper strip is
    enqueued a pass ahead of the lower one (it waits for nothing the lower strip does, so a driver may)."""
    r, boundary, before = Recorder(depths), H // 2 + 256, 0
    bounds = []
    for g in depths:
        boundary -= shift_of(g, before)
        before = g
        bounds.append(boundary)
    n = len(depths)
    if not ahead:
        for p in range(n):
            r.launch(p, 0, bounds[p], stream=1)
            r.launch(p, bounds[p], H, stream=2)
        return r.launches
    r.launch(0, 0, bounds[0], stream=1)
    for p in range(n):
        if p + 1 < n:
            r.launch(p + 1, 0, bounds[p + 1], stream=1)
        r.launch(p, bounds[p], H, stream=2)
    return r.launches


def tiles_behind_a_source(depths, block_ends, n_tiled, reach=0):
    """Passes 0 .. n_tiled-1 as row tiles: when a block has arrived, pass p advances to g rows (less `reach`) above
    where the pass before it has come; the last block's column completes them.  Whole-grid passes follow."""
    r, g = Recorder(depths), depths[0]
    frontier = [0] * n_tiled
    for k, end in enumerate(block_ends):
        for p in range(n_tiled):
            above = end if p == 0 else frontier[p - 1]
            upto = H if above >= H else max(above - g + reach, 0)
            if upto <= frontier[p]:
                break
            r.launch(p, frontier[p], upto, stream=1 + k % 2)
            frontier[p] = upto
    assert frontier == [H] * n_tiled
    for p in range(n_tiled, len(depths)):
        r.launch(p, 0, H)
    return r.launches


def check(launches, n, offset=0, deep=16, **more):
    return check_schedule(launches, H, 1, SRC, DST, offset, n, 1, halvings(deep), **more)


def rejected(invariant, launches, n, **more):
    with pytest.raises(ScheduleError) as e:
        check(launches, n, **more)
    assert e.value.invariant == invariant, str(e.value)
    return str(e.value)


# ---------------------------------------------------------------- accepted
@pytest.mark.parametrize("n,offset", [(1, 0), (5, 7), (37, 0), (95, 7), (200, 0)])
def test_one_strip_is_accepted(n, offset):
    passes = check(one_strip(plan_depths(n, 16), offset), n, offset)
    assert sum(depth for _, depth, _ in passes) == n


def test_no_generations_no_launches():
    assert check([], 0) == []
    rejected("I3", one_strip([1]), 0)


@pytest.mark.parametrize("n", [1, 37, 95])
def test_two_strips_are_accepted(n):
    depths = plan_depths(n, 16)
    check(two_strips_with_bands(depths), n)
    for ahead in (False, True):
        check(two_strips_with_a_moving_boundary(depths, max, ahead), n)


def test_launch_with_a_row_hole_is_accepted():
    """Both bands of a strip as one launch with the interior left out, the interior as another."""
    r = Recorder(plan_depths(24, 16))
    for p, g in enumerate(r.depths):
        r.launch(p, 0, H, hole=(g, H - g), stream=2)
        r.launch(p, g, H - g, stream=1)
    check(r.launches, 24)
    assert r.launches[0].produced() == [(0, 16), (H - 16, H)]


def test_tiles_are_accepted():
    depths = plan_depths(40, 8)
    launches = tiles_behind_a_source(depths, [512, 1024, 1536, 2048], n_tiled=3)
    check(launches, 40, deep=8)
    check_tile_frontiers(launches, H, 0, 40, 1, halvings(8))
    assert len([l for l in launches if l.iteration == 8]) == 4  # pass 1 came in four tiles


# ---------------------------------------------------------------- rejected
def probing_plan(n, deep, alt, alt_wins, split_odd=True):
    """The plan of a call that times its first passes at two depths: three of `deep`, 2 * deep / alt of `alt`, the rest
    at the winner's.  The number of passes must not depend on the winner's parity: one pass of `alt` of the plan that
    continues at `alt` becomes two of alt // 2 where it would."""
    head = [deep] * 3 + [alt] * (2 * (deep // alt))
    left = n - 5 * deep
    rest_deep, rest_alt = plan_depths(left, deep), plan_depths(left, deep, alt)
    if split_odd and (len(rest_deep) + len(rest_alt)) % 2:
        i = rest_alt.index(alt)
        rest_alt[i:i + 1] = [alt // 2, alt // 2]
    return head + (rest_alt if alt_wins else rest_deep)


def driver_plan(n, deep, alt, alt_wins):
    """The depths of one call as the driver plans them (runtime.hip, ststhip_run_passes) for a family with a second
    depth and a key: measured only where `alt` divides `deep` (the probes time the same generations at both depths),
    one of the two is even and the call is long enough; the parity of the two plans is brought together by halving
    one pass of even depth -- of `alt`, or, where that is odd, of `deep`.  Everything else runs at `alt`."""
    if not (2 <= alt < deep and deep % alt == 0 and (alt % 2 == 0 or deep % 2 == 0) and n >= 6 * deep):
        return plan_depths(n, deep, alt)
    head = [deep] * 3 + [alt] * (2 * (deep // alt))
    left = n - 5 * deep
    rest_deep, rest_alt = plan_depths(left, deep), plan_depths(left, deep, alt)
    if (len(rest_deep) + len(rest_alt)) % 2:
        plan, whole = (rest_alt, alt) if alt % 2 == 0 else (rest_deep, deep)
        i = plan.index(whole)
        plan[i:i + 1] = [whole // 2, whole // 2]
    assert (len(rest_deep) + len(rest_alt)) % 2 == 0
    return head + (rest_alt if alt_wins else rest_deep)


def test_every_family_the_header_allows_advances_exactly():
    """Every max_generations up to 64 with every repeated halving of it as the second depth, calls around the lengths
    at which the probes begin, both winners: the plan is a chain of compiled depths that sums to the call.  Among them
    the halvings that do not divide (18 -> 9 -> 4, 14 -> 7 -> 3, 22 / 5, 28 / 3): probe passes of such a family
    would not cover five launches of max_generations (18 / 4: 54 + 32 = 86, not 90), so it is not measured; nor is
    27 -> 13 -> 6 -> 3 with 3, which divides but leaves no pass of even depth to halve for the parity."""
    probed, not_probed = set(), set()
    named = {(16, 8), (12, 6), (12, 3), (24, 3), (18, 4), (14, 3), (22, 5), (28, 3), (27, 3)}
    for deep in range(2, 65):
        for alt in sorted(halvings(deep) - {deep, 1}):
            for n in list(range(1, 8)) + list(range(6 * deep - 2, 10 * deep + 3)):
                for wins in (False, True):
                    depths = driver_plan(n, deep, alt, wins)
                    assert sum(depths) == n and set(depths) <= halvings(deep), (deep, alt, n, wins, depths)
                    if (deep, alt) in named and n % 7 == 0:  # (as a schedule, for the families named below)
                        check_schedule(one_strip(depths), H, 1, SRC, DST, 0, n, 1, halvings(deep))
                    if n >= 6 * deep:
                        (probed if depths[0] == deep else not_probed).add((deep, alt))
    assert {(16, 8), (12, 6), (12, 3), (24, 3)} <= probed
    assert {(18, 4), (14, 3), (22, 5), (28, 3), (27, 3)} <= not_probed and not probed & not_probed
    assert driver_plan(108, 18, 4, True) == [4] * 27
    # the plan that was refused: the probe's head for 18 / 4 with the rest at either depth is four generations short
    short = [18] * 3 + [4] * (2 * (18 // 4)) + plan_depths(108 - 90, 18)
    assert "advance 104 generations, not 108" in rejected("I1", one_strip(short), 108, deep=18)
    assert driver_plan(72, 12, 3, True) == [12] * 3 + [3] * 8 + [3] * 4
    assert driver_plan(72, 12, 3, False) == [12] * 3 + [3] * 8 + [6, 6]


def test_lost_generation_is_rejected():
    """Depths 12 and 3, 72 generations, the shallower depth wins: halving a pass of three generations gives 1 + 1."""
    depths = probing_plan(72, 12, 3, alt_wins=True)
    assert depths == [12] * 3 + [3] * 8 + [1, 1, 3, 3, 3] and sum(depths) == 71
    message = rejected("I1", one_strip(depths), 72, deep=12)
    assert "advance 71 generations, not 72" in message
    # the same family where the split is of an even depth, and where none is needed
    check(one_strip(probing_plan(72, 12, 6, alt_wins=True)), 72, deep=12)
    check(one_strip(probing_plan(78, 12, 3, alt_wins=True)), 78, deep=12)
    for n in range(96, 130):
        for wins in (False, True):
            check(one_strip(probing_plan(n, 16, 8, wins)), n)


def test_depth_that_is_not_compiled_is_rejected():
    """12 / 4: four is no repeated halving of twelve."""
    depths = [12] * 3 + [4] * 6 + [12]
    assert "depth 4 is not one of [1, 3, 6, 12]" in rejected("I1", one_strip(depths), 72, deep=12)


def test_pass_chain_with_a_gap_or_an_overlap_is_rejected():
    good = one_strip([8, 8, 8])
    late = [dataclasses.replace(l, iteration=l.iteration + 1) if l.order == 2 else l for l in good]
    assert "a gap" in rejected("I1", late, 24)
    early = [dataclasses.replace(l, iteration=l.iteration - 1) if l.order == 2 else l for l in good]
    assert "an overlap" in rejected("I1", early, 24)
    mixed = two_strips_with_bands([8, 8])
    mixed[1] = dataclasses.replace(mixed[1], n_generations=4)
    assert "another depth" in rejected("I1", mixed, 16)


def test_row_gap_is_rejected():
    launches = two_strips_with_bands([16, 16])
    launches[5] = dataclasses.replace(launches[5], out_row_end=launches[5].out_row_end - 1)
    message = rejected("I2", launches, 32)
    assert "rows [1007, 1008)" in message and "produced by no launch" in message
    short = one_strip([16])
    short[0] = dataclasses.replace(short[0], out_row_end=H - 3)
    assert f"rows [{H - 3}, {H})" in rejected("I2", short, 16)


def test_row_overlap_is_rejected():
    launches = two_strips_with_bands([16, 16])
    launches[3] = dataclasses.replace(launches[3], out_row_begin=launches[3].out_row_begin - 2)
    message = rejected("I2", launches, 32)
    assert "rows [1038, 1040)" in message and "produced twice" in message and "#3" in message


def test_final_pass_in_scratch_is_rejected():
    """A plan whose length changed after the targets' parity was fixed."""
    launches = one_strip([16, 16, 16])
    flipped = [dataclasses.replace(l, src=SRC if l.order == 0 else (DST if l.src == SCRATCH else SCRATCH),
                                   dst=DST if l.dst == SCRATCH else SCRATCH) for l in launches]
    assert "last pass does not write the call's target" in rejected("I3", flipped, 48)


def test_broken_ping_pong_is_rejected():
    launches = one_strip([16, 16, 16])
    assert "does not read what pass 0 wrote" in rejected(
        "I3", [dataclasses.replace(l, src=(0x4000,)) if l.order == 1 else l for l in launches], 48)
    assert "writes the call's source" in rejected(
        "I3", [dataclasses.replace(l, dst=SRC) if l.order == 1 else l for l in launches], 48)
    third = [dataclasses.replace(l, dst=(0x4000,)) if l.order == 1 else
             dataclasses.replace(l, src=(0x4000,)) if l.order == 2 else l for l in one_strip([8, 8, 8, 8])]
    assert "2 plane sets besides" in rejected("I3", third, 32)


def test_consumer_enqueued_before_its_producer_is_rejected():
    """A tile that reaches as far down as the pass before it has come: its ghost rows are not there yet."""
    depths = plan_depths(40, 8)
    launches = tiles_behind_a_source(depths, [512, 1024, 1536, 2048], n_tiled=3, reach=8)
    message = rejected("I4", launches, 40, deep=8)
    assert "enqueued before their producer" in message and "launch #1 " in message
    with pytest.raises(ScheduleError) as e:
        check_tile_frontiers(launches, H, 0, 40, 1, halvings(8))
    assert e.value.invariant == "tiles"


def test_early_overwrite_is_rejected():
    """Moving boundaries, the upper strip a pass ahead, a pass of 8 generations behind one of 16: a boundary that moves
    up by the new pass's ghost rows alone lets the upper strip overwrite rows the lower strip's deeper launch of the
    pass before still reads.  What it READS is fine (I4 holds): only the order of the write is wrong."""
    depths = [16, 16, 16, 8, 8]
    check(two_strips_with_a_moving_boundary(depths, max), 64)
    launches = two_strips_with_a_moving_boundary(depths, lambda g, before: g)
    message = rejected("I5", launches, 64)
    assert "enqueued before their reader" in message and "generation 48 + 8" in message


def test_constants_flag_on_a_fresh_target_is_rejected():
    launches = one_strip([16, 16, 16])
    early = [dataclasses.replace(l, target_holds_constants=1) if l.order == 1 else l for l in launches]
    assert "no earlier pass of the call wrote these planes" in rejected("I6", early, 48)
    # ... while the flag on the tiles of a third pass is right: the first pass stored these rows before
    r = Recorder([8, 8, 8])
    for p, (a, b) in ((0, (0, 1024)), (1, (0, 1016)), (2, (0, 1008)), (0, (1024, H)), (1, (1016, H)), (2, (1008, H))):
        r.launch(p, a, b)
    check(r.launches, 24, deep=8)


def test_values_table_of_another_call_is_rejected():
    good = [dataclasses.replace(l, tdv=(0x9000, 7, 24, 8)) for l in one_strip([8, 8, 8], offset=7)]
    check(good, 24, 7, expect_tdv=True)
    stale = [dataclasses.replace(l, tdv=(0x9000, 0, 24, 8)) if l.order == 1 else l for l in good]
    assert "values table" in rejected("I7", stale, 24, offset=7, expect_tdv=True)
    assert "values table" in rejected("I7", one_strip([8, 8, 8], offset=7), 24, offset=7, expect_tdv=True)

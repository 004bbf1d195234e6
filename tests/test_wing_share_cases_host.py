"""CPU-only checks of tests/wing_share_cases.py, the inputs and the numpy mirror behind
tests/test_gpu_wing_shares.py: that the mirror's constants are the headers', that every case
reaches what it is named for (parts, share shapes, batched trips, group starts, refused groups,
masked rows), that the mirror hands every line of every range to exactly one wavefront exactly
once, and -- a condition on the inputs, from the oracle alone -- that every line of the probe
tile's wing and clipped ranges carries at least 10 x the 1e-6 contract of every point of the tile
inside its window, so that the contract of the GPU test sees a single lost, doubled or wrongly
masked line."""
from pathlib import Path

import numpy as np
import pytest

from tests import wing_share_cases as ws
from tests.test_gpu_wing_batches import expected_batches

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pylbl_amd" / "csrc"


@pytest.fixture(scope="module")
def runs(oracle):
    return ws.Runs(oracle)


@pytest.fixture(scope="module")
def mirrors(runs):
    """key -> the mirror of level 0 at the level's own K = 8 (asserted below)."""
    return {key: ws.mirror(runs(key)) for key in ws.CASES}


def level_batches(oracle, run, level):
    case = run.case
    return expected_batches(oracle, run.table, *case.levels[level], case.v0, case.vn, case.npv,
                            case.cut_off)


def test_constants_are_the_headers():
    accumulate = (CSRC / "accumulate.h").read_text()
    plans = (CSRC / "lanes_plans.inc").read_text()
    assert "share_of(sc.lo, sc.a1, piece, pieces, inverse, clipped_in_groups ? %d : %d," % (
        ws.CLIPPED_SHIFT, ws.LINE_SHIFT) in accumulate
    assert "share_of(sc.a2, sc.hi, piece, pieces, inverse, clipped_in_groups ? %d : %d," % (
        ws.CLIPPED_SHIFT, ws.LINE_SHIFT) in accumulate
    assert "share_of(sc.c1, sc.c2, piece, pieces, inverse, %d," % ws.LINE_SHIFT in accumulate
    assert "share_of(sc.f1, sc.c1, piece, pieces, inverse, %d, fa0, fa1);" % ws.WING_SHIFT \
        in accumulate
    assert "share_of(sc.c2, sc.f2, piece, pieces, inverse, %d, fb0, fb1);" % ws.WING_SHIFT \
        in accumulate
    assert "const int piece = item.part*4 + wave, pieces = item.parts*4;" in accumulate
    assert "const bool clipped_in_groups = !a.inner_everywhere &&" in accumulate
    assert "int parts = (int)std::min<long long>(%d, (weight[t] + target - 1)/target);" % \
        ws.MOST_PARTS in plans
    assert "parts = (int)std::min<long long>(%d, (load + target - 1)/target);" % ws.MOST_PARTS \
        in plans
    assert "const long long floor_lines = n_tiles < %d ? %d : %d;" % (
        ws.LARGE_GRID, ws.FLOOR_SMALL, ws.FLOOR_LARGE) in plans
    assert "if (%d*clipped[t] > %d*target)" % ws.CLIPPED_FACTORS in plans
    assert "load += %d*clipped[t];" % ws.CLIPPED_FACTORS[0] in plans
    assert "const long long target = std::max<long long>(floor_lines, total/(8*1536) + 1);" in plans
    assert "const double radius = kFarRatio*0.5*(double)(i1 - i0)*g.dv + 0.6;" in plans
    stages = (CSRC / "compute_stages.inc").read_text()
    assert "return (rq.cut_off - 1. <= reach + tile_width + 1.) ? 1 : 0;" in stages


def test_tilings_parts_and_ranges_are_the_ones_named(runs, mirrors):
    teens = False
    for key, m in mirrors.items():
        case = m.case
        assert m.tiling.p == case.points, key
        assert m.tiling.aligned == (1 if (case.aligned or case.farfield) else 0), key
        assert 4 <= m.tiling.n_tiles <= 19 or key in ws.BATCH_CASES, (key, m.tiling.n_tiles)
        s = m.schedules[case.tile]
        placed = runs(key).placed
        # Every line lies in the range of the probe tile it was placed in.
        expect = np.full(placed.size, 7)
        for kind, (a, b) in enumerate(((s.lo, s.a1), (s.a1, s.f1), (s.f1, s.c1), (s.c1, s.c2),
                                       (s.c2, s.f2), (s.f2, s.a2), (s.a2, s.hi))):
            expect[a:b] = kind
        assert np.array_equal(placed, expect), key
        assert m.everywhere == (1 if key == "cut-off-2" else 0), key
        if case.farfield:
            assert s.f1 - s.a1 == case.series_left and s.a2 - s.f2 == case.series_right, key
            assert s.c1 - s.f1 == case.wing_left and s.f2 - s.c2 == case.wing_right, key
    for key, parts in ws.PARTS_OF.items():
        m = mirrors[key]
        assert m.parts[m.case.tile] == parts and m.tiling.p == 4, (key, m.parts)
        teens |= 13 <= parts <= 19
    assert teens
    cap = mirrors["parts-64"]
    assert cap.weight[cap.case.tile] > 63*cap.target and cap.target == ws.FLOOR_SMALL
    for key in ws.BATCH_CASES:
        m = mirrors[key]
        assert m.tiling.n_tiles >= ws.LARGE_GRID and m.target == ws.FLOOR_LARGE, key
        assert m.parts[m.case.tile] == 1 and m.tiling.p == 4, key
    # The clipped load raises parts above ceil(weight/target), and only in the case named for it.
    for key in ("series", "series-clipped"):
        m = mirrors[key]
        t = m.case.tile
        plain = max(1, -(-int(m.weight[t])//m.target))
        raised = 3*m.clipped[t] > 4*m.target
        assert raised == (key == "series-clipped"), key
        assert (m.parts[t] > plain) == raised, (key, m.parts[t], plain)
    assert mirrors["series-clipped"].parts[4] == 6
    # Accumulating calls: one whole tile, one split tile.
    adding = sorted(int(mirrors[key].parts[c.tile]) for key, c in ws.CASES.items() if c.accumulate)
    assert adding[0] == 1 and adding[-1] > 1
    # The last tile of the plain grids is clipped by the grid.
    last = mirrors["last-row"]
    s = last.schedules[last.case.tile]
    assert last.case.tile == last.tiling.n_tiles - 1 and s.i1 - s.i0 + 1 < last.tiling.length


def test_the_mirror_counts_every_line_once(runs, mirrors):
    """For every tile and range the shares of all pieces tile [j0, j1) exactly once; for every
    wavefront quads, left-overs, groups and single lines account for every line of its shares
    exactly once.  (Every level and every cap of K of the cases that have several.)"""
    checked = 0
    for key in ws.CASES:
        run = runs(key)
        variants = [(level, cap) for level in range(len(run.case.levels))
                    for cap in run.case.caps]
        for level, cap in variants:
            m = mirrors[key] if (level, cap) == (0, 8) else ws.mirror(run, level, cap)
            for t, s in m.schedules.items():
                count = np.zeros(m.nu.size, dtype=np.int64)
                for part in range(int(m.parts[t])):
                    for wave in range(4):
                        wing, clipped = m.walks[(t, part, wave)]
                        for (a, b) in (wing.fa, wing.fb):
                            assert s.f1 <= a <= b <= s.f2
                        mine = np.concatenate([np.arange(*wing.fa), np.arange(*wing.fb)])
                        assert np.array_equal(np.sort(wing.walked), mine), (key, t, part, wave)
                        assert sum(wing.trips) == wing.eights and all(
                            1 <= x <= cap for x in wing.trips)
                        assert 8*wing.eights + (4 if wing.closing is not None else 0) + \
                            wing.left_a[1] + wing.left_b[1] == mine.size
                        theirs = np.concatenate([
                            np.arange(b, b + c) for b, c in zip(clipped.begin, clipped.count)])
                        assert np.array_equal(np.sort(clipped.walked), theirs), (key, t, part)
                        # A group never joins the two ranges.
                        for g in clipped.groups:
                            assert g.k + 8 <= clipped.count[0] or g.k >= clipped.count[0]
                        np.add.at(count, mine, 1)
                        np.add.at(count, theirs, 1)
                        checked += mine.size + theirs.size
                expect = np.zeros(m.nu.size, dtype=np.int64)
                expect[s.lo:s.a1] = 1
                expect[s.f1:s.c1] = 1
                expect[s.c2:s.f2] = 1
                expect[s.a2:s.hi] = 1
                assert np.array_equal(count, expect), (key, t)
    print("(line, wavefront) pairs accounted for: %d" % checked)


def _share_features(m, side):
    """What the wavefronts of the probe tile show for one far-wing range."""
    s = m.schedules[m.case.tile]
    j0, j1 = (s.f1, s.c1) if side == "left" else (s.c2, s.f2)
    units, pieces = (j1 - j0) >> 2, int(m.parts[m.case.tile])*4
    seen = set()
    walks = ws.probe_walks(m)
    for part, wave, wing, _ in walks:
        a, b = wing.fa if side == "left" else wing.fb
        last = part*4 + wave == pieces - 1
        if b == a and units < pieces and units > 0:
            seen.add("empty")
        if b - a == 4:
            seen.add("one unit")
        if last and (b - a) & 3:
            seen.add("remainder %d" % ((b - a) & 3))
        assert last or (b - a) & 3 == 0
    return seen


def test_cases_reach_every_share_shape(mirrors):
    left, right, walk = set(), set(), set()
    for key, m in mirrors.items():
        left |= _share_features(m, "left")
        right |= _share_features(m, "right")
        for part, wave, wing, _ in ws.probe_walks(m):
            if wing.qa & 1 and wing.straddling:
                walk.add("qa odd, an eight from both ranges")
            if wing.qa and not wing.qa & 1 and wing.qb:
                walk.add("qa even")
                assert not wing.straddling
            walk.add("quads 0" if wing.quads == 0 else "quads 1" if wing.quads == 1 else
                     "quads odd" if wing.quads & 1 else "quads even")
            if wing.closing is not None:
                walk.add("closing four")
            for o in wing.straddling:
                a, b = wing.groups[o]
                assert a == wing.fa[1] - ((wing.fa[1] - wing.fa[0]) & 3) - 4 and b == wing.fb[0]
    print("left:", sorted(left), "right:", sorted(right), "walk:", sorted(walk))
    shapes = {"empty", "one unit", "remainder 1", "remainder 2", "remainder 3"}
    assert left == shapes and right == shapes
    assert walk == {"qa odd, an eight from both ranges", "qa even", "quads 0", "quads 1",
                    "quads odd", "quads even", "closing four"}
    # The forced tile sizes walk the plain eight-line groups and reach a closing four as well.
    for key in ("P1", "P2", "P8"):
        walks = ws.probe_walks(mirrors[key])
        assert not any(wing.batched for _, _, wing, _ in walks)
        assert any(wing.eights >= 2 for _, _, wing, _ in walks), key
        assert any(wing.closing is not None for _, _, wing, _ in walks), key
        assert any(clipped.groups for _, _, _, clipped in walks), key


def test_cases_reach_every_batch_shape(oracle, runs):
    """K = 8 at the level of the one-level cases; under each cap of the batch cases wavefronts
    with fewer eights than K, with a short last trip and with whole trips only."""
    for key in ws.CASES:
        if key != "two-levels":
            assert level_batches(oracle, runs(key), 0) == 8, key
    for cap in (2, 4, 8):
        seen = set()
        for key in ws.BATCH_CASES:
            assert cap in ws.CASES[key].caps
            for _, _, wing, _ in ws.probe_walks(ws.mirror(runs(key), 0, cap)):
                assert wing.batched
                if 0 < wing.eights < cap:
                    seen.add("fewer")
                if wing.eights > cap and wing.eights % cap:
                    seen.add("short last trip")
                    assert wing.trips[-1] == wing.eights % cap
                if wing.eights >= cap and wing.eights % cap == 0:
                    seen.add("whole trips")
        assert seen == {"fewer", "short last trip", "whole trips"}, (cap, seen)
    # Two levels of one call whose own K differ.
    run = runs("two-levels")
    narrow, tropospheric = level_batches(oracle, run, 0), level_batches(oracle, run, 1)
    print("two levels: K = %d and %d" % (narrow, tropospheric))
    assert tropospheric == 8 and narrow in (2, 4)
    assert any(wing.eights > narrow for _, _, wing, _ in
               ws.probe_walks(ws.mirror(run, 0, narrow)))


def test_cases_reach_every_clipped_shape(mirrors):
    counts, offsets, closes = set(), set(), set()
    both_short = False
    for key, m in mirrors.items():
        s = m.schedules[m.case.tile]
        for part, wave, _, clipped in ws.probe_walks(m):
            if key == "cut-off-2":
                assert not clipped.in_groups and not clipped.groups
                assert len(clipped.singles) == sum(clipped.count)
                continue
            counts |= set(clipped.count)
            offsets |= {offset for _, offset in clipped.refused}
            for _, offset in clipped.refused:
                assert 1 <= offset <= 7
            if 0 < clipped.count[0] < 8 and 0 < clipped.count[1] < 8 and sum(clipped.count) >= 8:
                both_short = True
                assert not clipped.groups and len(clipped.singles) == sum(clipped.count)
            for g in clipped.groups:
                masked = [p for p, row in enumerate(g.rows) if row == "masked"]
                assert len(masked) <= 2     # the row the window opens in and the one it closes in
                if g.last < s.i1:       # the window closes inside the tile
                    p, lane = (g.last - s.i0) >> 6, (g.last - s.i0) & 63
                    assert g.rows[p] == ("masked" if lane < 63 or g.first > s.i0 + 64*p
                                         else "whole")
                    assert all(row == "skipped" for row in g.rows[p + 1:])
                    closes.add((key, p, lane))
                if g.first > s.i0:      # ... or opens there
                    p = (g.first - s.i0) >> 6
                    assert all(row == "skipped" for row in g.rows[:p])
                    assert g.rows[p] == ("masked" if (g.first - s.i0) & 63 else "whole")
    print("clipped counts per wavefront:", sorted(counts))
    print("refused at offsets:", sorted(offsets))
    print("windows closing in a group at (row, lane):", sorted({c[1:] for c in closes}))
    assert {0, 1, 7, 8, 9, 15, 16, 17} <= counts
    assert offsets == set(range(1, 8))
    assert both_short
    for key, wanted in ws.ROW_CASES.items():
        for p, lane in wanted:
            assert (key, p, lane) in closes, (key, p, lane)
    # Lane 63 of the last row is the tile's last point: a window that closes there covers the tile.
    assert not any(p == 3 and lane == 63 for _, p, lane in closes)
    # The last row of the last tile, which the grid clips.
    m = mirrors["last-row"]
    s = m.schedules[m.case.tile]
    row = (s.i1 - s.i0) >> 6
    assert s.i0 + 64*row + 63 > s.i1 == m.case.n - 1
    assert any(key == "last-row" and p == row for key, p, _ in closes)


def test_every_wing_and_clipped_line_weighs_ten_contracts(runs, mirrors):
    """From the oracle alone: the Lorentz term of every line of [lo,c1) and [c2,hi) of the probe
    tile over the oracle's value, at every point of the tile inside the line's window."""
    for key in ws.CASES:
        run = runs(key)
        case = run.case
        for level in range(len(case.levels)):
            m = mirrors[key] if level == 0 else ws.mirror(run, level)
            s = m.schedules[case.tile]
            lines = np.concatenate([np.arange(s.lo, s.c1), np.arange(s.c2, s.hi)])
            terms, inside = ws.lorentz_terms(case, run.derived[level], lines, s.i0, s.i1)
            assert inside.any(axis=1).all(), key
            share = np.where(inside, terms/run.k_ref[level][None, s.i0:s.i1 + 1], np.inf)
            smallest = float(share.min())
            print("%-16s level %d: %5d lines, smallest share %.3g = %.1f x REL" % (
                key, level, run.table.num_lines, smallest, smallest/ws.REL))
            assert smallest >= ws.CONDITION, (key, level, smallest)


def test_one_line_less_moves_the_probe_tile(oracle, runs, mirrors):
    """The oracle without the first or the last line of each of the four ranges differs from the
    full run by more than 10 x REL somewhere on the probe tile."""
    for key in ws.CASES:
        run = runs(key)
        case, table = run.case, run.table
        s = mirrors[key].schedules[case.tile]
        index = np.arange(table.num_lines)
        full = run.k_ref[0][s.i0:s.i1 + 1]
        for a, b in ((s.lo, s.a1), (s.f1, s.c1), (s.c2, s.f2), (s.a2, s.hi)):
            for j in {a, b - 1} if b > a else ():
                less, _ = oracle.absorption_port(table.subset(index != j), *case.levels[0],
                                                 case.v0, case.vn, case.npv, cut_off=case.cut_off)
                moved = float(np.max(np.abs(less[s.i0:s.i1 + 1] - full)/full))
                assert moved > ws.CONDITION, (key, j, moved)

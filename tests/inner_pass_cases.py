"""Inputs for the tests of the inner-point pass of the accumulate kernel under load
(csrc/accumulate_lines.h: inner_ranges -> inner_batch -> inner_evaluate), and a numpy mirror of the
pass's bookkeeping that says, from the inputs of a call and the oracle's derived scalars alone,
what every wavefront of every work item is handed and what its lists hold.

Tables: every line weighs.  One isotopologue, no shift, no temperature exponent, air and self
widths equal and set so that y = repwid*gamma is one of Y_VALUES at (T, P, X) -- the values of
tests/test_gpu_core_quotient.py below 8.425, at which a single line's inner arithmetic is already
held to 1e-12 -- and strengths log-uniform within one decade: at a point N lines cover, each
carries at least about 1/(10 N) of the sum, so a (line, point) pair that is lost, doubled or put
into the wrong class moves the point by far more than any bound of the GPU tests.

The mirror restates
  * the tiling, the eight keys and clamps of schedule_tile and the level's core_reach (taken from
    tests/farfield_cases.py, which restates pick_tiling, tile_bounds, fill_level, schedule_tile);
  * the plan's split (lanes_plans.inc: plan_for, series off): weight, target, parts;
  * share_of (accumulate.h) in float32, and the five ranges of accumulate_tile's general list,
    of which the pass walks the core range alone unless inner_everywhere (cut_off <= 2);
  * inner_index_range (line_prep.h), clipped to the line's window and to the tile;
  * the pass: batches of 32 list positions, the segments laid end to end, chunks of 64 positions,
    take = |x| < xlim1, the class by inner_limits / inner_class (voigt_profile.h), a list flushed
    when it holds 64 or more and at the end of the batch.

A line's segment in a tile is never empty where its core range misses the tile: the inner range
[floor((c - near - v0) npv) - 1, floor((c + near - v0) npv) + 2] lies inside the core range, the
same expression with reach >= near (xlim1 <= xlim0), so inner_batch's candidate test removes
nothing the clipping would not.

Region counters of the oracle (oracle/lbl_oracle.c, wells_point and lbl_oracle_voigt): slot 0 far
wing, 1 w4 region 1, 2 w4 region 2, 3 w4 region 3, 4 and 5 the two CPF12 branches, 6 the points of
pure-Lorentz lines.  The pairs the pass takes are slots 2, 3, 4 and 5: regions[2:6].
"""
from types import SimpleNamespace

import numpy as np

from tests import farfield_cases as fc

T, P_LEVEL, X = 296., 101325., 4.e-4
Y_VALUES = (5.e-7, 1.e-3, 0.5, 0.9, 5., 8.42)
SW_LOW, SW_HIGH = 1.e-22, 1.e-21
MOST_LINES = 2000           # the sum bound of the GPU test is derived for N <= 2000
ROUNDING = 1.e-12           # series off (tests/test_gpu_core_quotient.py)
SERIES = 1.e-9              # series on
REL = 1.e-6                 # the contract

QUEUE = 32                  # accumulate_lines.h: kInnerQueue
LIST = 128                  # accumulate_lines.h: kInnerList
CLASSES = 3                 # voigt_profile.h: kInnerClasses
SQRLN2 = np.sqrt(np.log(2.))


# ---------------------------------------------------------------------------------------------
# Cases.
def _case(name, v0, vn, npv, points, table, farfield=0, cut_off=25, tile=None):
    return SimpleNamespace(name=name, v0=v0, vn=vn, npv=npv, cut_off=cut_off, points=points,
                           farfield=farfield, n=(vn - v0)*npv, table=table, tile=tile)


def tiling_of(case):
    return fc.pick_tiling(case.points, case.farfield, case.npv, case.n)


def _span(v0, npv, points, tile):
    """[v_lo, v_hi] of a plain tile."""
    return v0 + tile*64*points/npv, v0 + (tile*64*points + 64*points - 1)/npv


def _far(rng, lo, hi, each=20):
    """`each` lines 3 to 20 cm-1 below `lo` and as many above `hi`: beyond any core (asserted by
    the host test), inside the window at cut-off 25."""
    return np.concatenate([rng.uniform(lo - 20., lo - 3., each),
                           rng.uniform(hi + 3., hi + 20., each)])


def _lines(rng, cluster, far):
    centres = np.concatenate([cluster, far])
    is_cluster = np.concatenate([np.ones(cluster.size, bool), np.zeros(far.size, bool)])
    y = rng.choice(Y_VALUES, centres.size)
    sw = np.exp(rng.uniform(np.log(SW_LOW), np.log(SW_HIGH), centres.size))
    order = np.argsort(centres, kind="stable")
    return SimpleNamespace(centres=centres[order], y=y[order], sw=sw[order],
                           cluster=is_cluster[order])


def grid_a(points):
    """At least 1 024 plain tiles: 66 P cm-1 around 1000 cm-1 at 1000 points per cm-1."""
    return 1000 - 33*points, 1000 + 33*points, 1000


A_TILE = 516
B_GRID = (1967, 2033, 8000)     # 528 000 points: 1 032 tiles at P = 8, 2 063 at P = 4
B_TILE = 515
B_SEED = 3
D_GRID = (1000, 1002, 1000)
D_TILE = {1: 15, 2: 7, 4: 3, 8: 1}


def lines_a(n_cluster, points):
    v0, vn, npv = grid_a(points)
    rng = np.random.default_rng(100 + n_cluster + points)
    lo, hi = _span(v0, npv, points, A_TILE)
    return _lines(rng, rng.uniform(lo + 0.0005, hi - 0.0005, n_cluster), _far(rng, lo, hi))


def lines_b():
    v0, vn, npv = B_GRID
    rng = np.random.default_rng(B_SEED)
    lo, hi = _span(v0, npv, 8, B_TILE)
    return _lines(rng, rng.uniform(lo + 0.0005, hi - 0.0005, 600), _far(rng, lo, hi))


def lines_c(place, points):
    v0, vn, npv = grid_a(points)
    rng = np.random.default_rng(300 + points + len(place))
    if place == "boundary":
        # The boundary between tiles A_TILE - 1 and A_TILE.
        lo, hi = _span(v0, npv, points, A_TILE - 1)[0], _span(v0, npv, points, A_TILE)[1]
        edge = _span(v0, npv, points, A_TILE)[0] - 0.5/npv
        cluster = rng.uniform(edge - 0.02, edge + 0.02, 600)
    elif place == "first point":
        cluster = rng.uniform(v0 - 0.01, v0 + 0.02, 600)
        lo, hi = v0 - 0.01, _span(v0, npv, points, 0)[1]
    else:
        end = v0 + ((vn - v0)*npv - 1)/npv
        cluster = rng.uniform(end - 0.02, end + 0.01, 600)
        lo, hi = end - 64*points/npv, end + 0.01
    far = _far(rng, lo, hi)
    # (the range rule of absorption.c:80-83 must discard nothing)
    far = far[(far > v0 - 25.9) & (far < vn + 25.9)]
    return _lines(rng, cluster, far)


def lines_d(points):
    v0, vn, npv = D_GRID
    rng = np.random.default_rng(400 + points)
    lo, hi = _span(v0, npv, points, D_TILE[points])
    return _lines(rng, rng.uniform(lo + 0.0005, hi - 0.0005, 600), _far(rng, lo, hi))


def lines_e():
    rng = np.random.default_rng(500)
    cluster = np.concatenate([rng.uniform(1001. - 0.03, 1001. + 0.03, 400),
                              rng.uniform(1000.5 - 0.03, 1000.5 + 0.03, 300)])
    return _lines(rng, cluster, np.zeros(0))


def _cases():
    out = {}
    for n_cluster in (512, 516, 600):
        for points in (1, 2, 4, 8):
            v0, vn, npv = grid_a(points)
            out["A-%d-P%d" % (n_cluster, points)] = _case(
                "A: %d lines in one tile, P = %d" % (n_cluster, points), v0, vn, npv, points,
                ("a", n_cluster, points), tile=A_TILE)
    for points in (8, 4):
        out["B-P%d" % points] = _case("B: list carries and long segments, P = %d" % points,
                                      *B_GRID, points, ("b",),
                                      tile=B_TILE if points == 8 else None)
    for place in ("boundary", "first point", "last point"):
        for points in (1, 8):
            v0, vn, npv = grid_a(points)
            out["C-%s-P%d" % (place.replace(" ", "-"), points)] = _case(
                "C: cluster at the %s, P = %d" % (place, points), v0, vn, npv, points,
                ("c", place, points))
    for points in (1, 2, 4, 8):
        out["D-P%d" % points] = _case("D: split tile, P = %d" % points, *D_GRID, points,
                                      ("d", points), tile=D_TILE[points])
    for cut_off in (0, 1, 2):
        for points in (1, 8):
            out["E-cut%d-P%d" % (cut_off, points)] = _case(
                "E: every range, cut_off = %d, P = %d" % (cut_off, points), *D_GRID, points,
                ("e",), cut_off=cut_off)
    v0, vn, npv = grid_a(8)
    out["F-A-600-P8"] = _case("F: case A with the series", v0, vn, npv, 8, ("a", 600, 8),
                              farfield=1)
    for points in (1, 8):
        v0, vn, npv = grid_a(points)
        out["F-C-boundary-P%d" % points] = _case(
            "F: case C's boundary cluster with the series, P = %d" % points, v0, vn, npv, points,
            ("c", "boundary", points), farfield=1)
    return out


CASES = _cases()
SUM_OF_LINES = ("D-P1", "D-P2", "D-P4", "D-P8", "A-516-P1")
_BUILDERS = {"a": lines_a, "b": lines_b, "c": lines_c, "d": lines_d, "e": lines_e}


def lines_of(case):
    return _BUILDERS[case.table[0]](*case.table[1:])


# ---------------------------------------------------------------------------------------------
# Tables.
def make_table(lines, case, oracle):
    """tests/test_gpu_core_quotient.make_table with a y and a strength per line."""
    from pylbl_amd import synthetic
    n = lines.centres.size
    table = synthetic.line_table("CO2", case.v0 - 30., case.vn + 30., num_lines=n, seed=1,
                                 tips_range=(150, 400))
    table.nu = lines.centres.astype(np.float64)
    table.sw = lines.sw.copy()
    table.n_air = np.zeros(n)
    table.elower = np.full(n, 100.)
    table.delta_air = np.zeros(n)
    table.local_iso_id = np.ones(n, dtype=np.int32)
    table.gamma_air = np.full(n, 0.07)
    table.gamma_self = np.full(n, 0.07)
    _, extras = oracle.absorption_port(table, T, P_LEVEL, X, case.v0, case.vn, case.npv,
                                       cut_off=case.cut_off, want_derived=True)
    alpha = extras["derived"][:, 1]
    assert np.all(alpha > 0.), "a line the range rule refused"
    width = lines.y*alpha/SQRLN2/(P_LEVEL*9.86923e-6)
    table.gamma_air = width.copy()
    table.gamma_self = width.copy()
    return table


class Runs(object):
    """key -> (case, lines, table, k_ref, derived, regions), made on first use and kept: the
    reference of a case is computed once and never written to.  Cases that share a table and a
    grid share the oracle's run."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.tables = {}
        self.references = {}

    def __call__(self, key):
        case = CASES[key]
        grid = (case.v0, case.vn, case.npv, case.cut_off)
        at = (case.table, grid)
        if at not in self.tables:
            lines = lines_of(case)
            self.tables[at] = (lines, make_table(lines, case, self.oracle))
        lines, table = self.tables[at]
        if at not in self.references:
            k_ref, extras = self.oracle.absorption_port(
                table, T, P_LEVEL, X, case.v0, case.vn, case.npv, cut_off=case.cut_off,
                want_derived=True, want_regions=True)
            k_ref.setflags(write=False)
            self.references[at] = (k_ref, extras["derived"], extras["regions"])
        k_ref, derived, regions = self.references[at]
        return SimpleNamespace(case=case, lines=lines, table=table, k_ref=k_ref, derived=derived,
                               regions=regions)


# ---------------------------------------------------------------------------------------------
# The mirror.
def line_records(case, derived):
    """Per line what prepare_line (line_prep.h) stores for the pass, from the oracle's derived
    scalars: window, repwid, y, xlim1, the index range of inner_index_range, the class limits."""
    centre, alpha, gamma = derived[:, 0], derived[:, 1], derived[:, 2]
    first, last = derived[:, 4].astype(np.int64), derived[:, 5].astype(np.int64)
    status = derived[:, 6]
    live = (status == 1.) & (last >= first)
    with np.errstate(divide="ignore", invalid="ignore"):
        repwid = np.where(live, SQRLN2/alpha, 1.)
    y = np.where(live, repwid*gamma, 100.)
    yy = np.minimum(y, 70.)
    xlim0 = np.sqrt(15100. + yy*(40. - yy*3.6))
    xlim1 = np.where(yy >= 8.425, 0., np.sqrt(np.maximum(164. - yy*(4.3 + yy*1.8), 0.)))
    xlim1 = np.where(yy <= 0.000001, xlim0, xlim1)
    xlim1 = np.where(live & (y < 70.55), xlim1, 0.)
    xlim0 = np.where(live & (y < 70.55), xlim0, 0.)
    near = (xlim1/repwid)*(1. + 1.e-9)
    lo = np.floor((centre - near - float(case.v0))*case.npv) - 1.
    hi = np.floor((centre + near - float(case.v0))*case.npv) + 2.
    return SimpleNamespace(
        centre=centre, repwid=repwid, y=y, xlim0=xlim0, xlim1=xlim1, first=first, last=last,
        live=live, inner_first=lo.astype(np.int64), inner_last=hi.astype(np.int64),
        two=np.where(y <= 0.000001, 1.e300, 6.8 - y), four=18.1*y + 1.65)


def share_of(j0, j1, part, parts, unit_shift=0):
    """accumulate.h: share_of, the cuts in single precision."""
    f32 = np.float32
    units = (j1 - j0) >> unit_shift
    scale, inverse = f32(units), f32(1.)/f32(parts)
    cut0 = min(int(scale*(f32(part)*inverse)), units)
    cut1 = min(int(scale*(f32(part + 1)*inverse)), units)
    begin = j0 + (cut0 << unit_shift)
    end = j1 if part + 1 == parts else j0 + (cut1 << unit_shift)
    return begin, end


def inner_everywhere(case):
    """compute_stages.inc: inner_points_everywhere is 1 whenever cut_off <= 2, and 0 at the
    reference's 25 for every reach a line of these tables can have (< 1 cm-1, host test)."""
    assert case.cut_off <= 2 or case.cut_off >= 10
    return 1 if case.cut_off <= 2 else 0


def plan_parts(case, tiling, nu):
    """lanes_plans.inc: plan_for with the series off -- parts of every tile."""
    assert not case.farfield
    npv, v0, cut = case.npv, case.v0, case.cut_off
    weight = np.zeros(tiling.n_tiles, dtype=np.int64)
    for t in range(tiling.n_tiles):
        i0, i1 = fc.tile_bounds(tiling, t, npv, case.n)
        lo = float((i0 + npv - 1)//npv + v0 - cut - 1) - 0.05
        hi = float(i1//npv + v0 + cut) + 1.05
        weight[t] = np.searchsorted(nu, hi, "left") - np.searchsorted(nu, lo, "left")
    total = int(weight.sum())
    target = max(128 if tiling.n_tiles < 1024 else 2048, total//(8*1536) + 1)
    return np.maximum(np.minimum(64, -(-weight//target)), 1), weight, target


def wavefront_list(case, s, piece, pieces):
    """The line indices accumulate_tile hands inner_ranges for one wavefront, in the order of
    general_index: the core range's share, and with inner_everywhere the shares of the clipped
    ranges and the 0-3 left-over lines of the far-wing ranges as well."""
    core = share_of(s.c1, s.c2, piece, pieces)
    if not inner_everywhere(case):
        return np.arange(*core), core
    below = share_of(s.lo, s.a1, piece, pieces)
    above = share_of(s.a2, s.hi, piece, pieces)
    fa0, fa1 = share_of(s.f1, s.c1, piece, pieces, 2)
    fb0, fb1 = share_of(s.c2, s.f2, piece, pieces, 2)
    ranges = [below, core, above, (fa0 + ((fa1 - fa0) & ~3), fa1), (fb0 + ((fb1 - fb0) & ~3), fb1)]
    return np.concatenate([np.arange(a, max(a, b)) for a, b in ranges]).astype(np.int64), core


def wavefront_pass(case, rec, listed, i0, i1):
    """inner_ranges over one wavefront's list on the tile [i0, i1]."""
    out = SimpleNamespace(
        lines=len(listed), batch_sizes=[], adding=0, before=[[] for _ in range(CLASSES)],
        left=[[] for _ in range(CLASSES)], most_chunks=0, cut_by_tile=0, cut_by_window=0,
        first_inside=0, last_inside=0, begins_at_zero=0, ends_at_last=0, outside_grid=0,
        pairs=0, points=np.zeros(0, dtype=np.int64))
    dv = 1./case.npv
    points = []
    for base in range(0, len(listed), QUEUE):
        batch = np.asarray(listed[base:base + QUEUE], dtype=np.int64)
        out.batch_sizes.append(batch.size)
        has = rec.xlim1[batch] > 0.
        raw_first, raw_last = rec.inner_first[batch], rec.inner_last[batch]
        out.outside_grid += int(np.sum(has & ((raw_last < 0) | (raw_first > case.n - 1))))
        in_tile_first, in_tile_last = np.maximum(raw_first, i0), np.minimum(raw_last, i1)
        first = np.maximum(in_tile_first, rec.first[batch])
        last = np.minimum(in_tile_last, rec.last[batch])
        length = np.where(has & (last >= first), last - first + 1, 0)
        if not length.any():
            continue
        out.adding += 1
        taken = length > 0
        out.cut_by_tile += int(np.sum(taken & ((np.maximum(raw_first, rec.first[batch]) < i0) |
                                               (np.minimum(raw_last, rec.last[batch]) > i1))))
        first_cut = has & (in_tile_last >= in_tile_first) & (rec.first[batch] > in_tile_first) & \
            (rec.first[batch] <= in_tile_last)
        last_cut = has & (in_tile_last >= in_tile_first) & (rec.last[batch] < in_tile_last) & \
            (rec.last[batch] >= in_tile_first)
        out.first_inside += int(np.sum(first_cut))
        out.last_inside += int(np.sum(last_cut))
        out.cut_by_window += int(np.sum(first_cut | last_cut))
        out.begins_at_zero += int(np.sum(taken & (raw_first < 0) & (first == 0)))
        out.ends_at_last += int(np.sum(taken & (raw_last > case.n - 1) & (last == case.n - 1)))
        end = np.cumsum(length)
        begin = end - length
        out.most_chunks = max(out.most_chunks,
                              int(np.max(np.where(taken, (end - 1)//64 - begin//64 + 1, 0))))
        # The packed sequence: slot and grid point of every position.
        slot = np.repeat(np.arange(batch.size), length)
        point = np.concatenate([np.arange(f, f + n) for f, n in zip(first, length)])
        line = batch[slot]
        # absorption.c:39: v[i] = v0 + i*dv (product rounded, then the sum); voigt.c:76-78.
        v = float(case.v0) + point.astype(np.float64)*dv
        abx = np.abs((v - rec.centre[line])*rec.repwid[line])
        take = abx < rec.xlim1[line]
        cls = np.where(abx >= rec.two[line], 0, np.where(abx <= rec.four[line], 1, 2))
        count = [0]*CLASSES
        total = int(end[-1])
        for chunk in range(0, total, 64):
            for c in range(CLASSES):
                count[c] += int(np.sum(take[chunk:chunk + 64] & (cls[chunk:chunk + 64] == c)))
                assert count[c] < LIST
                if count[c] >= 64:
                    out.before[c].append(count[c])
                    count[c] -= 64
                    out.left[c].append(count[c])
        for c in range(CLASSES):
            if count[c] > 0:
                out.before[c].append(count[c])
                out.left[c].append(0)
        out.pairs += int(np.sum(take))
        points.append(point[take])
    if points:
        out.points = np.unique(np.concatenate(points))
    return out


def mirror(case, table, derived):
    """Every (tile, part, wavefront) of a call: {(tile, part, wave): wavefront_pass(...)} for the
    wavefronts whose list is not empty, with the schedule and the parts of every tile."""
    nu = np.asarray(table.nu, dtype=np.float64)
    assert np.all(np.diff(nu) >= 0.)
    tiling = tiling_of(case)
    lv = fc.level_scalars(table, T, P_LEVEL)
    rec = line_records(case, derived)
    if case.farfield:
        # plan_for's far-field form is not restated: on 1 024 tiles or more an item holds 2 048
        # lines at least (and a tile is cut by its clipped windows only beyond 4/3 of that), so a
        # table of at most MOST_LINES lines leaves every tile whole.
        assert tiling.n_tiles >= 1024 and nu.size <= MOST_LINES < 2048
        parts = np.ones(tiling.n_tiles, dtype=np.int64)
    else:
        parts = plan_parts(case, tiling, nu)[0]
    schedules, passes = [], {}
    for t in range(tiling.n_tiles):
        s = fc.schedule_tile(case, tiling, case.farfield, nu, lv, t)
        schedules.append(s)
        if s.hi == s.lo or (s.c2 == s.c1 and not inner_everywhere(case)):
            continue
        for part in range(int(parts[t])):
            for wave in range(4):
                listed, core = wavefront_list(case, s, part*4 + wave, int(parts[t])*4)
                if len(listed):
                    got = wavefront_pass(case, rec, listed, s.i0, s.i1)
                    got.core = core
                    passes[(t, part, wave)] = got
    return SimpleNamespace(case=case, tiling=tiling, level=lv, records=rec, parts=parts,
                           schedules=schedules, passes=passes, nu=nu)


def tile_of_index(tiling, case, index):
    for t in range(tiling.n_tiles):
        i0, i1 = fc.tile_bounds(tiling, t, case.npv, case.n)
        if i0 <= index <= i1:
            return t
    raise ValueError(index)

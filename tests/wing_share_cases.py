"""Inputs for the line-by-line tests of the far-wing and clipped-window loops of the accumulate
kernel (csrc/accumulate_lines.h: fast_ranges, clipped_ranges; csrc/accumulate.h: share_of and the
shares of accumulate_tile; csrc/lanes_plans.inc: plan_for), and a numpy mirror of their index
arithmetic that says, from the inputs of a call and the oracle's derived scalars alone, which lines
every wavefront of every work item walks and how.

Tables: every wing line weighs the same on one tile.  A case names a probe tile; v* is its centre.
One isotopologue, no shift, no temperature exponent, no lower-state energy, air and self widths of
0.07, T = 296 K (S(T) = sw) and sw = 1e-24 ((nu - v*)^2 + 0.07^2): the Lorentz term of every line
at v* is the same number, and over the tile it stays within the ratio (d*/d)^2.  A lost, doubled or
wrongly masked line moves the tile by about 1/N.  The lines of the probe tile's core range [c1,c2)
take max((nu - v*)^2, 1) instead: tests/test_gpu_inner_pass.py and tests/test_gpu_core_quotient.py
own that range, here it only must not hide the others.  A case states how many lines each of the
probe tile's ranges holds -- per 1 cm-1 cell in the clipped ranges, where the lines of a cell share
one window (spectra.c:48-62) -- so the share shapes are designed, not drawn.

The mirror restates nothing that tests/farfield_cases.py (pick_tiling, tile_bounds, level_scalars,
schedule_tile) and tests/inner_pass_cases.py (share_of in float32, plan_parts) hold already.  It
adds
  * plan_for with the series on: the near-lines weight, clipped[t], and 3 clipped > 4 target;
  * inner_points_everywhere (compute_stages.inc);
  * the wing walk of one wavefront (accumulate_tile + fast_ranges): the shares in units of four
    lines, qa, quads, eights, the batched trips for a given K, the eights that take their two
    quads from the two ranges, the closing lorentz_four, the 0-3 left-overs;
  * the clipped walk of one wavefront (clipped_ranges): the shares in units of eight lines (of one
    under inner_everywhere, where the loop is not used), `room`, the test that all eight windows
    agree, the slide by one line where they do not, and per group the rows skipped, taken whole
    and masked.
"""
from types import SimpleNamespace

import numpy as np

from tests import farfield_cases as fc
from tests.inner_pass_cases import plan_parts, share_of
from tests.test_gpu_core_quotient import ROUNDING, SERIES
from tests.test_gpu_parity import REL

T, P_LEVEL, X = 296., 101325., 4.e-4
LEVEL = (T, P_LEVEL, X)
WIDTH = 0.07
SW_UNIT = 1.e-24
MARGIN = 2.e-3              # the outermost lines of a range lie this far inside it [cm-1]
CONDITION = 10.*REL         # the smallest share a wing or clipped line may have on the probe tile

WING_SHIFT, CLIPPED_SHIFT, LINE_SHIFT = 2, 3, 0     # accumulate.h: the unit shifts of share_of
MOST_PARTS = 64                                     # lanes_plans.inc: plan_for
FLOOR_SMALL, FLOOR_LARGE, LARGE_GRID = 128, 2048, 1024
CLIPPED_FACTORS = (3, 4)                            # 3*clipped > 4*target

# Two levels whose far-wing bounds (line_prep.h: wing_batches) differ on one table: the level
# shapes of tests/test_gpu_wing_batches.CASES "narrow lines near 1 cm-1" and "tropospheric CO2".
NARROW = (200., 0.01, 1.e-5)
TROPOSPHERIC = (288.99, 98388., 3.6e-4)


def order(n):
    """Bound on re-ordering the sum of n positive terms (tests/test_gpu_inner_pass.py)."""
    return 2.*max(n - 1, 0)*2.**-53


def rounding_bound(n):
    """Series off: ROUNDING where order(n) is at most half of it, ROUNDING + order(n) beyond."""
    return ROUNDING if order(n) <= ROUNDING/2. else ROUNDING + order(n)


# ---------------------------------------------------------------------------------------------
# Cases.
def _case(name, tile, left=(), wing_left=0, core=0, wing_right=0, right=(), series_left=0,
          series_right=0, v0=1000, span=12, npv=100, points=4, cut_off=25, farfield=0, aligned=0,
          caps=(8,), levels=(LEVEL,), extra=(), accumulate=False):
    """`tile` is the probe tile.  `left` and `right` give the lines per 1 cm-1 cell of its clipped
    ranges [lo,a1) and [a2,hi), the other counts the lines of [a1,f1), [f1,c1), [c1,c2), [c2,f2)
    and [f2,a2); `extra` are centres outside [lo,hi).  `caps` are the values of the engine option
    wing_batches the case runs under."""
    return SimpleNamespace(
        name=name, tile=tile, left=tuple(left), wing_left=wing_left, core=core,
        wing_right=wing_right, right=tuple(right), series_left=series_left,
        series_right=series_right, v0=v0, vn=v0 + span, npv=npv, n=span*npv, points=points,
        cut_off=cut_off, farfield=farfield, aligned=aligned, caps=tuple(caps),
        levels=tuple(levels), extra=tuple(extra), accumulate=accumulate)


def _cases():
    out = {}
    # Parts 1, 2, 3, 5, 13 and the cap of 64: the plain tiling of 256 points at 100 points per
    # cm-1, five tiles, the last clipped by the grid; the probe tile 2 holds every line.
    out["parts-1"] = _case("parts 1: wing shares of 0, 1 and 2 units", 2, left=(1,),
                           wing_left=37, core=6, wing_right=10, right=(7,), accumulate=True)
    out["parts-1b"] = _case("parts 1: clipped counts 9 and 15, quads 0 and 1", 2, left=(4, 5),
                            wing_left=4, core=5, wing_right=7, right=(8, 7))
    out["parts-1c"] = _case("parts 1: clipped counts 8, 16 and 17", 2, left=(20, 21),
                            wing_left=9, core=4, wing_right=10, right=(30, 34))
    out["parts-1d"] = _case("parts 1: both clipped ranges below 8, together 11", 2, left=(2, 3),
                            wing_left=22, core=7, wing_right=27, right=(3, 3))
    out["parts-2"] = _case("parts 2: a window changes at every offset of a group", 2,
                           left=(7, 57), wing_left=45, core=8, wing_right=51, right=(35, 29),
                           accumulate=True)
    out["parts-3"] = _case("parts 3", 2, left=(19, 24), wing_left=110, core=10, wing_right=141,
                           right=(13, 30))
    out["parts-5"] = _case("parts 5: fewer units than pieces on the left", 2, left=(40, 41),
                           wing_left=70, core=12, wing_right=390, right=(33, 20))
    out["parts-13"] = _case("parts 13", 2, left=(33, 34), wing_left=701, core=83, wing_right=723,
                            right=(30, 25))
    out["parts-64"] = _case("parts 64, the cap", 2, left=(150, 151), wing_left=3500, core=430,
                            wing_right=3600, right=(140, 145))
    # Batches: 1 025 tiles, so an item holds up to 2 048 lines and a wavefront many eights.
    long_grid = dict(span=2624, caps=(2, 4, 8))
    out["batch-8"] = _case("batches: eights 8 per wavefront", 2, left=(8, 9), wing_left=256,
                           core=6, right=(9, 8), **long_grid)
    out["batch-1-2"] = _case("batches: eights 1 and 2 per wavefront", 2, left=(8, 8),
                             wing_left=32, core=6, wing_right=26, right=(8, 8), **long_grid)
    out["batch-5"] = _case("batches: eights 5 per wavefront, the eleventh quad alone", 2,
                           left=(8, 8), wing_left=83, core=6, wing_right=88, right=(8, 8),
                           **long_grid)
    out["batch-long"] = _case("batches: 1 990 lines in one item", 2, left=(66, 67), wing_left=801,
                              core=90, wing_right=853, right=(57, 56), **long_grid)
    # Two levels whose own K differ, near 30 cm-1 where the Doppler widths are small.
    out["two-levels"] = _case("two levels, K differs", 2, left=(16, 17), wing_left=160, core=0,
                              wing_right=174, right=(9, 24), v0=26, span=12,
                              levels=(NARROW, TROPOSPHERIC), extra=(0.3,))
    # Other P: the plain eight-line groups, 1, 2 and 8 rows.
    out["P1"] = _case("P = 1", 9, left=(17,), wing_left=45, core=5, wing_right=51, right=(10,),
                      points=1)
    out["P2"] = _case("P = 2", 3, left=(9, 16), wing_left=143, core=9, wing_right=170,
                      right=(8, 7), points=2)
    out["P8"] = _case("P = 8", 1, left=(8, 9, 16, 17, 8), wing_left=150, core=12, wing_right=133,
                      right=(16, 1, 15, 8, 8), points=8, span=24)
    # Windows that close in every row at lane 0 and at lane 63 (a window that closes at lane 63 of
    # the tile's last row covers the tile: it belongs to the fast ranges, not to the clipped ones).
    out["rows-lane0"] = _case("windows close at lane 0 of rows 0 to 3", 1, left=(16, 16, 16, 16),
                              wing_left=20, core=4, wing_right=20, right=(16, 16, 16),
                              npv=64, span=16)
    out["row0-lane63"] = _case("a window closes at lane 63 of row 0", 0,
                               left=(8, 16, 16, 16, 16), wing_left=3, core=4, wing_right=21,
                               right=(16, 16, 16, 16), npv=63, span=17)
    out["row1-lane63"] = _case("a window closes at lane 63 of row 1", 0, left=(8, 16, 16),
                               wing_left=5, core=4, wing_right=21, right=(16, 16), npv=127,
                               span=9)
    out["row2-lane63"] = _case("a window closes at lane 63 of row 2", 0, left=(8, 16),
                               wing_left=6, core=4, wing_right=21, right=(16,), npv=191,
                               span=6)
    out["last-row"] = _case("a window closes in the last row of the last tile", 4,
                            left=(16, 9), wing_left=21, core=4, wing_right=19,
                            right=(8, 8), npv=50, span=23)
    # cut_off 2: inner_everywhere, shares cut line by line, clipped_ranges not used.
    out["cut-off-2"] = _case("cut-off 2: inner_everywhere", 4, left=(9, 10), wing_left=5, core=20,
                             wing_right=11, right=(10, 9), cut_off=2, span=14)
    # Aligned tiles of 250 points, one per cell, without and with the series.
    aligned = dict(npv=250, span=8, aligned=1)
    out["aligned"] = _case("aligned tiles, series off", 4, left=(17,), wing_left=170, core=9,
                           wing_right=181, **aligned)
    out["series"] = _case("series on", 4, left=(16,), series_left=60, wing_left=23, core=6,
                          wing_right=17, series_right=70, farfield=1, **aligned)
    out["series-clipped"] = _case("series on: the clipped load raises parts", 4, left=(200,),
                                  series_left=60, wing_left=47, core=6, wing_right=38,
                                  series_right=70, farfield=1, **aligned)
    return out


CASES = _cases()
PARTS_OF = {"parts-1": 1, "parts-2": 2, "parts-3": 3, "parts-5": 5, "parts-13": 13,
            "parts-64": 64}
BATCH_CASES = ("batch-8", "batch-1-2", "batch-5", "batch-long")
ROW_CASES = {"rows-lane0": ((0, 0), (1, 0), (2, 0), (3, 0)), "row0-lane63": ((0, 63),),
             "row1-lane63": ((1, 63),), "row2-lane63": ((2, 63),)}


def tiling_of(case):
    return fc.pick_tiling(case.points, 1 if (case.farfield or case.aligned) else 0, case.npv,
                          case.n)


# ---------------------------------------------------------------------------------------------
# Tables.
def _blank_table(case, n):
    from pylbl_amd import synthetic
    table = synthetic.line_table("CO2", max(case.v0 - 30., 0.01), case.vn + 30., num_lines=n,
                                 seed=1, tips_range=(150, 400))
    table.gamma_air = np.full(n, WIDTH)
    table.gamma_self = np.full(n, WIDTH)
    table.n_air = np.zeros(n)
    table.elower = np.zeros(n)
    table.delta_air = np.zeros(n)
    table.local_iso_id = np.ones(n, dtype=np.int32)
    return table


def _spread(a, b, count):
    """`count` centres evenly over [a + MARGIN, b - MARGIN]."""
    if count == 0:
        return np.zeros(0)
    assert b - a > 4.*MARGIN, (a, b, count)
    return a + MARGIN + (b - a - 2.*MARGIN)*(np.arange(count) + 0.5)/count


def probe_keys(case):
    """The wavenumbers at which the probe tile's schedule cuts the sorted table at the widest
    level of the case (tile_schedule.h through fc.schedule_tile): lo, a1, f1, c1, c2, f2, a2, hi."""
    tiling = tiling_of(case)
    blank = _blank_table(case, 1)
    i0, i1 = fc.tile_bounds(tiling, case.tile, case.npv, case.n)
    v_lo, v_hi = float(fc.wavenumber(case, i0)), float(fc.wavenumber(case, i1))
    npv, v0, cut = case.npv, case.v0, case.cut_off
    keys = SimpleNamespace(
        lo=float((i0 + npv - 1)//npv + v0 - cut - 1), a1=float((i1 + npv - 1)//npv + v0 - cut - 1),
        a2=float(i0//npv + v0 + cut) + 1., hi=float(i1//npv + v0 + cut) + 1.,
        centre=0.5*(v_lo + v_hi), v_lo=v_lo, v_hi=v_hi)
    cores, radii = [], []
    for temperature, pressure, _ in case.levels:
        lv = fc.level_scalars(blank, temperature, pressure)
        _, radius, core, _, _ = fc.far_radius(lv, v_lo, v_hi)
        cores.append(core)
        radii.append(radius)
    keys.c1, keys.c2 = v_lo - max(cores), v_hi + max(cores)
    keys.f1, keys.f2 = keys.a1, keys.a2
    if case.farfield:
        keys.f1 = min(max(keys.centre - min(radii), keys.a1), keys.c1)
        keys.f2 = max(min(keys.centre + min(radii), keys.a2), keys.c2)
        keys.s1 = min(max(keys.centre - max(radii), keys.a1), keys.c1)
        keys.s2 = max(min(keys.centre + max(radii), keys.a2), keys.c2)
    return keys


def make_table(case):
    """The equal-weight table of a case and, per line, the range of the probe tile it was placed
    in: 0 [lo,a1), 1 [a1,f1), 2 [f1,c1), 3 [c1,c2), 4 [c2,f2), 5 [f2,a2), 6 [a2,hi), 7 elsewhere."""
    k = probe_keys(case)
    pieces = []
    cells_left = int(k.a1 - k.lo)
    cells_right = int(k.hi - k.a2)
    assert len(case.left) <= cells_left and len(case.right) <= cells_right, \
        (case.name, cells_left, cells_right)
    for cell, count in enumerate(case.left):
        pieces.append((0, _spread(k.lo + cell, k.lo + cell + 1., count)))
    if case.farfield:
        pieces.append((1, _spread(k.a1, k.s1, case.series_left)))
        pieces.append((5, _spread(k.s2, k.a2, case.series_right)))
    else:
        assert case.series_left == 0 and case.series_right == 0
    pieces.append((2, _spread(k.f1, k.c1, case.wing_left)))
    pieces.append((3, _spread(k.c1, k.c2, case.core)))
    pieces.append((4, _spread(k.c2, k.f2, case.wing_right)))
    for cell, count in enumerate(case.right):
        pieces.append((6, _spread(k.a2 + cell, k.a2 + cell + 1., count)))
    pieces.append((7, np.asarray(case.extra, dtype=np.float64)))
    nu = np.concatenate([x for _, x in pieces])
    placed = np.concatenate([np.full(x.size, r, dtype=np.int64) for r, x in pieces])
    at = np.argsort(nu, kind="stable")
    nu, placed = nu[at], placed[at]
    assert np.all(np.diff(nu) > 0.)
    # absorption.c:80-83 must refuse nothing, and no window may lie right of the grid.
    assert nu[0] > case.v0 - (case.cut_off + 1) and nu[-1] < case.vn + case.cut_off
    d = nu - k.centre
    table = _blank_table(case, nu.size)
    table.nu = nu
    table.sw = SW_UNIT*(np.where(placed == 3, np.maximum(d*d, 1.), d*d) + WIDTH*WIDTH)
    return table, placed


def second_table(table):
    """What an accumulating call finds in `out`: the spectrum of every other line, doubled."""
    other = table.subset(np.arange(table.num_lines) % 2 == 0)
    other.sw = 2.*other.sw
    return other


class Runs(object):
    """key -> (case, table, placed, per level k_ref and derived), made on first use and kept: the
    reference of a case is computed once and never written to."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.kept = {}

    def __call__(self, key):
        if key not in self.kept:
            case = CASES[key]
            table, placed = make_table(case)
            k_ref, derived = [], []
            for level in case.levels:
                k, extras = self.oracle.absorption_port(table, *level, case.v0, case.vn, case.npv,
                                                        cut_off=case.cut_off, want_derived=True)
                k.setflags(write=False)
                k_ref.append(k)
                derived.append(extras["derived"])
            self.kept[key] = SimpleNamespace(case=case, table=table, placed=placed,
                                             k_ref=k_ref, derived=derived)
        return self.kept[key]


def lorentz_terms(case, derived, lines, i0, i1):
    """[lines, points]: S gamma/pi / ((v - c)^2 + gamma^2) on the points i0..i1, zero outside
    the line's window."""
    index = np.arange(i0, i1 + 1)
    v = fc.wavenumber(case, index)
    centre, gamma, strength = (derived[lines, c][:, None] for c in (0, 2, 3))
    first, last = derived[lines, 4][:, None], derived[lines, 5][:, None]
    d = v[None, :] - centre
    inside = (index[None, :] >= first) & (index[None, :] <= last)
    return np.where(inside, strength*gamma/np.pi/(d*d + gamma*gamma), 0.), inside


def lines_covering(case, derived):
    """Per grid point the number of lines whose windows hold it."""
    first, last = derived[:, 4].astype(np.int64), derived[:, 5].astype(np.int64)
    live = (derived[:, 6] == 1.) & (last >= first)
    steps = np.zeros(case.n + 1, dtype=np.int64)
    np.add.at(steps, first[live], 1)
    np.add.at(steps, last[live] + 1, -1)
    return np.cumsum(steps)[:case.n]


# ---------------------------------------------------------------------------------------------
# The mirror.
def plan(case, tiling, nu):
    """lanes_plans.inc: plan_for -- (parts, weight, clipped, target) of every tile; with the series
    off tests/inner_pass_cases.plan_parts."""
    if not case.farfield:
        parts, weight, target = plan_parts(case, tiling, nu)
        return parts, weight, np.zeros_like(weight), target
    npv, v0, cut = case.npv, case.v0, case.cut_off
    below = lambda key: int(np.searchsorted(nu, key, "left"))
    weight = np.zeros(tiling.n_tiles, dtype=np.int64)
    clipped = np.zeros(tiling.n_tiles, dtype=np.int64)
    for t in range(tiling.n_tiles):
        i0, i1 = fc.tile_bounds(tiling, t, npv, case.n)
        lo = float((i0 + npv - 1)//npv + v0 - cut - 1) - 0.05
        hi = float(i1//npv + v0 + cut) + 1.05
        full_lo = float((i1 + npv - 1)//npv + v0 - cut - 1)
        full_hi = float(i0//npv + v0 + cut) + 1.
        clipped[t] = max(0, below(full_lo + 0.05) - below(lo)) + \
            max(0, below(hi) - below(full_hi - 0.05))
        u0 = 0.5*(float(fc.wavenumber(case, i0)) + float(fc.wavenumber(case, i1)))
        radius = fc.FAR_RATIO*0.5*float(i1 - i0)*(1./npv) + 0.6
        lo, hi = max(lo, u0 - radius), min(hi, u0 + radius)
        weight[t] = below(hi) - below(lo)
    total = int(weight.sum())
    floor_lines = FLOOR_SMALL if tiling.n_tiles < LARGE_GRID else FLOOR_LARGE
    target = max(floor_lines, total//(8*1536) + 1)
    parts = np.maximum(np.minimum(MOST_PARTS, -(-weight//target)), 1)
    a, b = CLIPPED_FACTORS
    raised = a*clipped > b*target
    parts = np.where(raised, np.minimum(MOST_PARTS, -(-(weight + a*clipped)//target)), parts)
    return parts, weight, clipped, target


def inner_everywhere(case, tiling, levels):
    """compute_stages.inc: inner_points_everywhere."""
    reach = 0.
    for lv in levels:
        kk = lv.core_reach
        reach = max(reach, kk*(case.vn + 1.)/(1. - kk) + 2.*lv.shift_max if kk < 0.5 else 1.e9)
    return 1 if case.cut_off - 1. <= reach + float(tiling.length)*(1./case.npv) + 1. else 0


def wing_walk(s, piece, pieces, batches, points):
    """accumulate_tile's far-wing shares and fast_ranges of one wavefront."""
    fa0, fa1 = share_of(s.f1, s.c1, piece, pieces, WING_SHIFT)
    fb0, fb1 = share_of(s.c2, s.f2, piece, pieces, WING_SHIFT)
    qa, qb = (fa1 - fa0) >> 2, (fb1 - fb0) >> 2
    quads = qa + qb
    start = lambda q: fa0 + 4*q if q < qa else fb0 + 4*(q - qa)
    eights = quads >> 1
    batched = points == 4 and batches > 1
    trips = [min(batches, eights - o) for o in range(0, eights, batches)] if batched \
        else [1]*eights
    groups = [(start(2*o), start(2*o + 1)) for o in range(eights)]
    straddling = [o for o in range(eights) if 2*o < qa <= 2*o + 1]
    closing = start(quads - 1) if quads & 1 else None
    left_a = (fa0 + ((fa1 - fa0) & ~3), (fa1 - fa0) & 3)
    left_b = (fb0 + ((fb1 - fb0) & ~3), (fb1 - fb0) & 3)
    walked = [np.arange(j, j + 4) for pair in groups for j in pair]
    if closing is not None:
        walked.append(np.arange(closing, closing + 4))
    walked += [np.arange(j, j + count) for j, count in (left_a, left_b)]
    return SimpleNamespace(
        fa=(fa0, fa1), fb=(fb0, fb1), qa=qa, qb=qb, quads=quads, eights=eights, trips=trips,
        batched=batched, groups=groups, straddling=straddling, closing=closing, left_a=left_a,
        left_b=left_b, walked=np.concatenate(walked).astype(np.int64) if walked
        else np.zeros(0, dtype=np.int64))


def clipped_walk(s, first, last, piece, pieces, everywhere, points):
    """accumulate_tile's clipped shares and clipped_ranges of one wavefront: `first`, `last` are
    the windows of every line (the oracle's derived columns)."""
    shift = LINE_SHIFT if everywhere else CLIPPED_SHIFT
    begin0, end0 = share_of(s.lo, s.a1, piece, pieces, shift)
    begin1, end1 = share_of(s.a2, s.hi, piece, pieces, shift)
    count0, count1 = end0 - begin0, end1 - begin1
    total = count0 + count1
    out = SimpleNamespace(begin=(begin0, begin1), count=(count0, count1), groups=[], singles=[],
                          refused=[], in_groups=not everywhere)
    k = 0
    while k < total:
        j = begin0 + k if k < count0 else begin1 + (k - count0)
        room = (k + 8 <= count0) if k < count0 else (k + 8 <= total)
        if room and not everywhere:
            same = (first[j:j + 8] == first[j]) & (last[j:j + 8] == last[j])
            if same.all():
                rows = []
                for p in range(points):
                    r0 = s.i0 + 64*p
                    if last[j] < r0 or first[j] > r0 + 63:
                        rows.append("skipped")
                    elif first[j] <= r0 and last[j] >= r0 + 63:
                        rows.append("whole")
                    else:
                        rows.append("masked")
                out.groups.append(SimpleNamespace(k=k, j=j, first=int(first[j]),
                                                  last=int(last[j]), rows=rows))
                k += 8
                continue
            out.refused.append((k, int(np.argmin(same))))
        out.singles.append(j)
        k += 1
    walked = [np.arange(g.j, g.j + 8) for g in out.groups] + [np.asarray(out.singles, np.int64)]
    out.walked = np.concatenate(walked).astype(np.int64)
    return out


def mirror(run, level=0, batches=8):
    """Every (tile, part, wavefront) of one level of a call: the schedule and the parts of every
    tile, and {(tile, part, wave): (wing_walk, clipped_walk)} for the tiles that hold a line."""
    case, table, derived = run.case, run.table, run.derived[level]
    nu = np.asarray(table.nu, dtype=np.float64)
    tiling = tiling_of(case)
    levels = [fc.level_scalars(table, t, p) for t, p, _ in case.levels]
    parts, weight, clipped, target = plan(case, tiling, nu)
    everywhere = inner_everywhere(case, tiling, levels)
    first, last = derived[:, 4].astype(np.int64), derived[:, 5].astype(np.int64)
    schedules, walks = {}, {}
    for t in range(tiling.n_tiles):
        s = fc.schedule_tile(case, tiling, case.farfield, nu, levels[level], t)
        if s.hi == s.lo:
            continue
        schedules[t] = s
        pieces = int(parts[t])*4
        for piece in range(pieces):
            walks[(t, piece >> 2, piece & 3)] = (
                wing_walk(s, piece, pieces, batches, tiling.p),
                clipped_walk(s, first, last, piece, pieces, everywhere, tiling.p))
    return SimpleNamespace(case=case, tiling=tiling, parts=parts, weight=weight, clipped=clipped,
                           target=target, everywhere=everywhere, schedules=schedules, walks=walks,
                           nu=nu)


def probe_walks(m):
    """[(part, wave, wing_walk, clipped_walk)] of the probe tile."""
    return [(part, wave, *m.walks[(t, part, wave)]) for (t, part, wave) in sorted(m.walks)
            if t == m.case.tile]

"""Inputs for the tests of the tile schedule's table searches (csrc/tile_schedule.h:
search_bracket, first_not_below, first_above; csrc/engine.hip: the cell_first block of
lbl_molecule_load), and a numpy mirror of them.

Every one of the eight searches of schedule_tile starts from a bracket: lbl_molecule_load records
where the sorted table reaches every 1/scale cm-1 (cell_first[i] = the first line with
nu >= base + i/scale), and search_bracket starts a search one cell either side of the cell its key
falls in.  scale is 8 for tables that span less than 131 072 cm-1, a coarser multiple of 1/8 (not a
power of two) for wider ones, and beyond 8 388 608 cm-1 there is no cell table: the whole table is
searched.  The mirror restates the builder and the bracket operation for operation, searches
inside the bracket with the kernel's own loops, and takes the keys and the clamps from
tests/farfield_cases.py, whose schedule_tile (np.searchsorted on the whole table) is what it is
held to.

One base table, and variants of it that differ in one inert line far outside every window, placed
for the scale it forces: what a call computes does not depend on it, how its searches are bracketed
does.  tests/test_schedule_search_cases_host.py checks all of this on the CPU;
tests/test_gpu_schedule_search.py runs the cases.
"""
import math
from types import SimpleNamespace

import numpy as np

from tests import farfield_cases as fc

CELL_LIMIT = 1048576.       # engine.hip: at most this many cells
FINEST = 8.                 # engine.hip: cells per cm-1, at most; scale is a multiple of 1/FINEST
SPAN_LIMIT = 1.e12          # engine.hip: no cell table from this span on
X = fc.X

MUTATIONS = ("lo from cell at + 1", "hi from cell at", "cell table built with <=",
             "scale 8 in the search", "lo index not clamped to last")
# What tests/test_schedule_search_cases_host.py finds: the first, second and fourth change the
# schedule of tiles the GPU test runs; the third and the fifth change brackets and never a
# schedule (test_two_mutants_change_brackets_and_no_schedule says why).
NO_MARGIN = "lo from cell at"

FIRST, LAST = 990., 1040.           # the base table's first and last line, both on integers
GAPS = ((1012., 1016.), (1021., 1025.))
DUPLICATES = (1007.125, 9)          # nine lines on one eighth
DENSE_CELL = (1010., 70)            # seventy lines in [1010, 1010.125)

# The 2-level calls pass their level scalars as kernel arguments, the 5-level calls through
# memory (kInlineLevels = 4); both hold ordinary and low pressures, so shift_max differs.
FIVE_LEVELS = fc.FIVE_LEVELS
TWO_LEVELS = (fc.FIVE_LEVELS[4], fc.FIVE_LEVELS[0])

# name -> (position of the inert line or None, scale or None)
VARIANTS = {
    "fine": (None, 8.),
    "switch": (FIRST + 131072.5, 7.875),
    "coarse": (FIRST + 305000.5, 3.375),
    "coarsest": (FIRST + 8300000.5, 0.125),
    "none": (FIRST + 8400000.5, None),
    "below": (-300000.5, 3.375),
}
ABOVE = ("switch", "coarse", "coarsest", "none")        # the inert line lies above the table


# ---------------------------------------------------------------------------------------------
# Tables.
def base_table():
    """About 300 lines of one strength and width between FIRST and LAST; what it holds is listed
    and checked by test_base_table_is_what_the_cases_need
    (tests/test_schedule_search_cases_host.py)."""
    rng = np.random.default_rng(950)
    up, down = (lambda x: np.nextafter(x, np.inf)), (lambda x: np.nextafter(x, -np.inf))
    centres, delta = [FIRST, LAST], [0., 0.]

    def add(at, shift=0.):
        centres.append(float(at))
        delta.append(shift)

    # Lines on eighths, and one ulp to either side of eighths.
    for eighth in (990.125, 991.5, 993.875, 996.25, 1000.125, 1003.375, 1009.5, 1011.875, 1016.,
                   1018.625, 1020.875, 1025., 1026.25, 1030.75, 1033.125, 1036.5, 1039.875):
        add(eighth)
    for eighth in (992.25, 997.625, 1002.5, 1008.75, 1017.375, 1019.125, 1028.875, 1034.25,
                   1038.625):
        add(up(eighth))
        add(down(eighth))
    for eighth in (995.5, 1005.125, 1027.75):
        add(down(eighth))
        add(eighth)
        add(up(eighth))
    for _ in range(DUPLICATES[1]):
        add(DUPLICATES[0])
    first, count = DENSE_CELL
    for k in range(count):
        add(first + 0.125*(k + 0.5)/count)
    # Lines within 0.002 cm-1 of integers with pressure shifts that carry them across at 1 atm
    # and not at 10 Pa, or never: where the windows of a tile's first and last cells begin and
    # end (the keys of lo and hi are integers -+ shift_max).
    integers = [i for i in range(int(FIRST) + 1, int(LAST))
                if not any(a <= i <= b for a, b in GAPS) and i != first]
    for k, integer in enumerate(integers):
        offset = (0.001, -0.001, 0.0015, -0.0005)[k % 4]
        shift = (-0.02, 0.02, 0.012, 0.02, 0.02, -0.02, -0.015, -0.004)[k % 8]
        add(integer + offset, shift)
        if k % 3 == 0:
            add(integer - offset, -shift)
    # A uniform fill outside the gaps, a third of it shifted.
    fill = rng.uniform(FIRST + 0.05, LAST - 0.05, 400)
    taken = 0
    for at in fill:
        if taken == 110:
            break
        if any(a - 0.01 <= at <= b + 0.01 for a, b in GAPS) or abs(at - round(at)) < 0.01 or \
                first - 0.01 <= at <= first + 0.135:
            continue
        add(at, float(rng.uniform(-0.02, 0.02)) if taken % 3 == 0 else 0.)
        taken += 1
    table = fc.make_table(centres, delta, 1000)
    for column in ("nu", "sw", "gamma_air", "gamma_self", "n_air", "elower", "delta_air"):
        getattr(table, column).setflags(write=False)
    return table


def variant_table(base, name):
    """The base table plus the variant's inert line: every column but nu copied from line 0, in
    sorted order (the inert line is the last row, or the first in `below`)."""
    at, _ = VARIANTS[name]
    if at is None:
        return base
    rows = np.concatenate([np.arange(base.num_lines), [0]])
    table = base.subset(rows)
    table.nu = table.nu.copy()
    table.nu[-1] = at
    if at < base.nu[0]:
        table = table.subset(np.roll(np.arange(table.num_lines), 1))
    assert np.all(np.diff(table.nu) >= 0.)
    return table


# ---------------------------------------------------------------------------------------------
# The mirror.
def cell_table(nu, mutation=None):
    """(base, scale, entries, cell_first) of lbl_molecule_load for the sorted positions nu, or None
    where the engine uploads none.  (The builder walks the table once, `while (j < n && nu[j] <
    edge) ++j`: for edges that do not decrease, which base + i/scale are, that is the first index
    with nu >= edge; test_cell_table_is_the_builders_loop runs the loop itself.)"""
    nu = np.asarray(nu, dtype=np.float64)
    if nu.size == 0:
        return None
    base = np.floor(nu[0])
    span = np.ceil(nu[-1]) - base + 1.
    if not (span >= 1. and span < SPAN_LIMIT):
        return None
    scale = min(FINEST, np.floor(CELL_LIMIT/span*FINEST)/FINEST)
    if not scale > 0.:
        return None
    entries = int(span*scale) + 1
    edges = base + np.arange(entries, dtype=np.float64)/scale
    side = "right" if mutation == "cell table built with <=" else "left"
    cell_first = np.searchsorted(nu, edges, side).astype(np.int32)
    return SimpleNamespace(base=float(base), scale=float(scale), entries=entries,
                           cell_first=cell_first, edges=edges)


def cell_of(table, x, mutation=None):
    """`at` of search_bracket: the cell x falls in, as the kernel computes it."""
    scale = FINEST if mutation == "scale 8 in the search" else table.scale
    return float(math.floor((x - table.base)*scale)) if math.isfinite(x) else \
        float(np.floor((x - table.base)*scale))


def search_bracket(table, n_lines, x, mutation=None):
    """[lo, hi] of search_bracket (tile_schedule.h) for the key x."""
    lo, hi = 0, int(n_lines)
    if table is None or not x == x:
        return lo, hi
    at = cell_of(table, x, mutation)
    last = table.entries - 1
    first = table.cell_first
    if at >= 1.:
        margin = {"lo from cell at + 1": 1, NO_MARGIN: 0}.get(mutation, -1)
        if mutation == "lo index not clamped to last":
            # (int)at - 1 past the table reads what lies behind it: modelled as n_lines.
            index = int(at) - 1
            lo = first.item(index) if index <= last else int(n_lines)
        else:
            lo = first.item(min(int(min(at, float(last))) + margin, last))
    if at + 2. <= float(last):
        margin = 0 if mutation == "hi from cell at" else 2
        hi = first.item(max(int(max(at, -2.)) + margin, 0))
    return lo, hi


def first_not_below(nu, lo, hi, x):
    trips = 0
    while lo < hi:
        mid = (lo + hi) >> 1
        if nu[mid] < x:
            lo = mid + 1
        else:
            hi = mid
        trips += 1
    return lo, trips


def first_above(nu, lo, hi, x):
    trips = 0
    while lo < hi:
        mid = (lo + hi) >> 1
        if nu[mid] <= x:
            lo = mid + 1
        else:
            hi = mid
        trips += 1
    return lo, trips


def call_tiling(case, farfield=True):
    """(tiling, farfield) of a call on `case` with or without the series asked for."""
    if farfield:
        return fc.call_tiling(case)
    return fc.pick_tiling(case.points, 0, case.npv, case.n), 0


def tile_keys(case, table, level, farfield=True):
    """[(s, keys)] of every tile of a call at `level` = (temperature, pressure): the same for every
    variant of a table (an inert line moves none of the level scalars)."""
    lv = fc.level_scalars(table, *level)
    tiling, _ = call_tiling(case, farfield)
    return [fc.schedule_keys(case, tiling, lv, t) for t in range(tiling.n_tiles)]


def scheduled(case, table, level, bracket=True, farfield=True, mutation=None, cells=False,
              keys=None):
    """The TileSchedule of every tile of a call on `case` at `level`: every key searched inside
    its mirrored bracket by the kernel's loops, then the clamps.  bracket=False:
    farfield_cases.schedule_tile.  `cells` and `keys`: cell_table(table.nu, mutation) and
    tile_keys(case, table, level, farfield), where the caller has them."""
    assert mutation is None or mutation in MUTATIONS + (NO_MARGIN,)
    nu = np.asarray(table.nu, dtype=np.float64)
    tiling, far = call_tiling(case, farfield)
    if not bracket:
        lv = fc.level_scalars(table, *level)
        return [fc.schedule_tile(case, tiling, far, nu, lv, t) for t in range(tiling.n_tiles)]
    if cells is False:
        cells = cell_table(nu, mutation)
    if keys is None:
        keys = tile_keys(case, table, level, farfield)
    out, positions = [], nu.tolist()
    for s, eight in keys:
        found = []
        for key, above in eight:
            lo, hi = search_bracket(cells, nu.size, key, mutation)
            found.append((first_above if above else first_not_below)(positions, lo, hi, key)[0])
        out.append(fc.clamp_schedule(SimpleNamespace(**vars(s)), found, far))
    return out


_VARIANTS = {}


def variants():
    """name -> (table, cell table or None), made once; the scales are the ones the names stand
    for."""
    if not _VARIANTS:
        base = base_table()
        for name, (_, scale) in VARIANTS.items():
            table = variant_table(base, name)
            cells = cell_table(table.nu)
            assert (cells.scale if cells is not None else None) == scale, (name, cells)
            _VARIANTS[name] = (table, cells)
    return _VARIANTS


# ---------------------------------------------------------------------------------------------
# Windows.  (a) inside the table across both gaps; (b) from more than cut_off + 2 below the first
# line; (c) to more than cut_off + 2 above the last; (d) and (e) out of the table's reach.
def _case(name, v0, span, npv, points, cut_off):
    return SimpleNamespace(name=name, v0=v0, vn=v0 + span, npv=npv, cut_off=cut_off,
                           points=points, n=span*npv)


def _b(cut_off):
    return int(FIRST) - cut_off - 5


def _c(cut_off):
    return int(LAST) + cut_off + 5 - 12


CASES = {
    "a aligned 500": _case("a: 1009-1028, aligned tiles of 500, cut-off 25", 1009, 19, 1000, 8, 25),
    "a unaligned 512": _case("a: 1009-1028, unaligned tiles of 512, cut-off 3", 1009, 19, 700, 8, 3),
    "a aligned 63": _case("a: 1009-1028, one point per lane, cut-off 3", 1009, 19, 1000, 1, 3),
    "a coarse grid": _case("a: 1009-1028, 100 points per cm-1, cut-off 25", 1009, 19, 100, 0, 25),
    "b cut 25": _case("b: 960-972 below the table, cut-off 25", _b(25), 12, 1000, 0, 25),
    "b cut 3": _case("b: 982-994 across the first line, cut-off 3", _b(3), 12, 700, 8, 3),
    "c cut 25": _case("c: 1058-1070 above the table, cut-off 25", _c(25), 12, 700, 0, 25),
    "c cut 3": _case("c: 1036-1048 across the last line, cut-off 3", _c(3), 12, 1000, 1, 3),
    "d cut 25": _case("d: 955-960, out of reach below, cut-off 25", 955, 5, 100, 0, 25),
    "d cut 3": _case("d: 975-985, out of reach below, cut-off 3", 975, 10, 1000, 0, 3),
    "e cut 25": _case("e: 1070-1075, out of reach above, cut-off 25", 1070, 5, 100, 0, 25),
    "e cut 3": _case("e: 1045-1055, out of reach above, cut-off 3", 1045, 10, 1000, 0, 3),
}
OUT_OF_REACH = ("d cut 25", "d cut 3", "e cut 25", "e cut 3")


def in_range(table, case):
    """The rows the skip policy accepts (absorption.c:80-83 without the break)."""
    return table.subset((table.nu >= case.v0 - (case.cut_off + 1)) &
                        (table.nu <= case.vn + case.cut_off + 1))

"""Inputs for the lines call (lbl_compute: csrc/compute_call.inc, csrc/compute_stages.inc) at its
two index limits, with the numpy mirrors that say what each input is.

Levels.  levels_per_pass() ends in min(chunk, n_levels, 65535) and every kernel of a pass takes the
level as blockIdx.y: a call of more levels runs in passes, the later ones at base = 65535, 131070.
The big calls here repeat K = 7 pattern levels (level l is pattern level l % 7; 7 does not divide
65535, so a later pass starts on another pattern level than level 0) on the smallest tables and
grids that still run the kernels in question: `small` (no split tile), `split` (plan_for cuts the
one tile into parts: combine_kernel), `scan` (more rows than kScanThreads: run_find_kernel's
look-back, and a split tile as well -- the tile that holds every line of the table is cut as soon
as it holds more than 128), `far` (a grid on which shape_of keeps the far-field series on) and
`pieces` (several tiles: a streamed call in pieces).

Grid points.  shape_of() takes grids of up to 2^30 - 1 points: BIG is 32 767 points short of that,
with clusters of lines whose windows cover index 0, both sides of 2^28, of 2^29 and of 3 2^28, and
the last tile.

tests/test_many_levels_cases_host.py proves on the CPU that each case is what
tests/test_gpu_many_levels.py takes it for and holds the expressions restated here against the
text of the sources."""
from collections import namedtuple
import math
import re

import numpy as np

from tests import pedestal_run_cases as runs
from tests.pedestal_run_cases import CSRC, Grid, PA_TO_ATM

ROW = 65535                 # compute_stages.inc: levels_per_pass's cap, gridDim.y of every kernel
INLINE_LEVELS = 4           # tile_schedule.h: kInlineLevels
SCAN_THREADS = 256          # pedestal_runs.h: kScanThreads
FAR_RATIO = 4.              # accumulate.h: LBL_FAR_RATIO
ITEM_FLOOR = 128            # lanes_plans.inc: floor_lines of a plan of fewer than 1024 tiles
MOST_PARTS = 64             # lanes_plans.inc: parts of a tile
WING_BYTES, CORE_BYTES, SCHEDULE_BYTES = 32, 128, 32    # LineWing, LineCore, TileSchedule
RUN_META_BYTES, RUN_LINK_BYTES, SWEEP_BUFFERS, RUN_CUT = 48, 48, 7, 1024    # pedestal.h
VLIGHT = 2.99792458e8
R2 = 2*math.log(2)*8314.472                             # spectra.c:14

# ---------------------------------------------------------------------------------------------
# Part 1: the pattern levels (T [K], P [Pa], x).
PATTERN = np.asarray([
    (220., 1.e-4, 4.e-4),       # 0 near vacuum: y <= 1e-6 (voigt.c:48-53, xlim1 = xlim0)
    (250., 30000., 4.e-4),      # 1 every line has y >= 8.425: inner_possible == 0
    (288., 120000., 4.e-4),     # 2 lines with y >= 70.55 (voigt.c:21-25: Lorentz everywhere)
    (288., 101325., 4.e-4),     # 3 1 atm: every row opens a pedestal run
    (230., 10., 4.e-4),         # 4 10 Pa: a window is one run
    (255., 3000., 4.e-4),       # 5 ordinary
    (240., 300., 0.01),         # 6 ordinary
])
K = PATTERN.shape[0]
NEAR_VACUUM, NO_INNER, LORENTZ, EVERY_ROW, ONE_RUN = 0, 1, 2, 3, 4
COUNTS = (ROW, ROW + 1, ROW + 12, 2*ROW + 3)
# Passes that hold all seven pattern levels (relax_launches follows the pass's max_runs).
WHOLE_PATTERN_COUNTS = (ROW, ROW + 12)

SMALL = Grid(2300, 2308, 4, 2)          # 32 points: one tile
FAR = Grid(2300, 2308, 64, 3)           # 512 points; the series stays on (far_series_kept)
GRIDS = {"small": SMALL, "split": SMALL, "scan": SMALL, "far": FAR, "pieces": FAR}
_PER_INTEGER = {"small": 3, "split": 21, "scan": 51, "far": 3, "pieces": 3}
_tables = {}


def table(name):
    """pedestal_run_cases.near_integer_table on every integer whose window reaches the grid: rows
    at N + (0.0005 .. 0.0035), delta_air alternating between -0.009 and +0.001 -- here from the
    first row of every N on, an odd number of rows to the integer: at 1 atm the rows of N fall
    into the windows N - 1, N, N - 1, ..., N - 1 and the first row of N + 1 into N, so that every
    row of the table opens a run, the first of an integer too."""
    if name not in _tables:
        g = GRIDS[name]
        per_integer = _PER_INTEGER[name]
        integers = np.arange(g.v0 - g.cut_off, g.vn + g.cut_off)
        made = runs.near_integer_table(integers, per_integer, seed=400 + per_integer + g.cut_off)
        assert per_integer % 2 == 1
        made.delta_air = np.where(np.arange(made.num_lines) % per_integer % 2 == 0, -0.009, 0.001)
        _tables[name] = made
    return _tables[name]


def levels(count):
    """(T, P, x) of a call of `count` levels: level l is pattern level l % K."""
    index = np.arange(count) % K
    return tuple(np.ascontiguousarray(PATTERN[index, c]) for c in range(3))


def points(grid):
    return (grid.vn - grid.v0)*grid.n_per_v


# -- prepare_line's y and bound_inner_regions, restated ---------------------------------------
def line_widths(tab, level):
    """(centre, alpha, gamma, y) per row: spectra.c:22-29 and voigt.c:13-14 as line_prep.h states
    them."""
    temperature, pressure, x = (float(v) for v in level)
    p_atm = pressure*PA_TO_ATM
    p_partial = p_atm*x
    tfact = 296./temperature
    iso = np.asarray(tab.local_iso_id, np.int64)
    slot = np.where(iso == 0, 10, iso) - 1
    doppler = np.sqrt(R2*temperature/tab.mass_by_slot()[slot])
    centre = tab.nu + p_atm*tab.delta_air
    power = np.asarray([math.pow(tfact, float(n)) for n in tab.n_air])
    gamma = (tab.gamma_air*(p_atm - p_partial) + tab.gamma_self*p_partial)*power
    alpha = (tab.nu/VLIGHT)*doppler
    y = (math.sqrt(math.log(2.))/alpha)*gamma
    return centre, alpha, gamma, y


def inner_possible(tab, level, grid):
    """bound_inner_regions (compute_stages.inc): 0 when no accepted line can have y < 8.425."""
    temperature, pressure, x = (float(v) for v in level)
    p_atm = pressure*PA_TO_ATM
    p_partial = p_atm*x
    foreign = p_atm - p_partial
    tfact = 296./temperature
    iso = np.asarray(tab.local_iso_id, np.int64)
    slot = np.where(iso == 0, 10, iso) - 1
    widest = float(np.max(np.sqrt(R2*temperature/tab.mass_by_slot()[np.unique(slot)])))
    power = min(math.pow(tfact, float(tab.n_air.min())), math.pow(tfact, float(tab.n_air.max())))
    gamma = (float(tab.gamma_air.min())*foreign + float(tab.gamma_self.min())*p_partial)*power
    alpha = ((grid.vn + grid.cut_off + 1)/VLIGHT)*widest
    y_lower = math.sqrt(math.log(2.))*gamma/alpha*(1. - 1.e-9)
    return 0 if (alpha > 0. and y_lower >= 8.425) else 1


INNER_TEXT = ("const double power = std::min(pow(lv.tfact, m.min_n_air), pow(lv.tfact, m.max_n_air));",
              "const double gamma = (m.min_gamma_air*foreign + m.min_gamma_self*lv.p_partial)*power;",
              "const double alpha = (rule.nu_max/2.99792458e8)*widest;",
              "const double y_lower = sqrt(log(2.))*gamma/alpha*(1. - 1.e-9);",
              "if (alpha > 0. && y_lower >= 8.425)")
Y_TEXT = ("const double centre = nu + lv.p_atm*delta_air;",
          "const double gamma = (gamma_air*(lv.p_atm - lv.p_partial) + gamma_self*lv.p_partial)*",
          "const double alpha = (nu/vlight)*lv.doppler[iso_slot];",
          "const double repwid = sqrln2/alpha;", "const double y = repwid*gamma;",
          "if (y < 70.55)", "double xlim1 = (y >= 8.425) ? 0. : sqrt(164. - y*(4.3 + y*1.8));",
          "if (y <= 0.000001) xlim1 = xlim0;")


# -- pick_tiling, plan_for's parts, shape_of's far-field condition -----------------------------
Tiling = namedtuple("Tiling", "points aligned per_cell length n_tiles")


def tiling(grid, farfield, forced=0, aligned_tiles=0):
    """pick_tiling (lanes_plans.inc)."""
    npv, n = grid.n_per_v, points(grid)
    is_forced = forced in (1, 2, 4, 8)
    for candidate in (8, 4, 2, 1):
        p = forced if is_forced else candidate
        width = 64*p
        per_cell = (npv + width - 1)//width
        waste = per_cell*width/npv - 1.
        if (aligned_tiles or farfield) and waste <= 0.06:
            return Tiling(p, 1, per_cell, (npv + per_cell - 1)//per_cell, (n//npv)*per_cell)
        if is_forced:
            break
    p = forced
    if not is_forced:
        p = 8 if (npv >= 400 and farfield) else 2 if (npv >= 100 and farfield) else \
            4 if npv >= 100 else 2 if npv >= 10 else 1
    return Tiling(p, 0, 0, 64*p, (n + 64*p - 1)//(64*p))


TILING_TEXT = ("p = (n_per_v >= 400 && farfield) ? 8 : (n_per_v >= 100 && farfield) ? 2",
               ": n_per_v >= 100 ? 4 : n_per_v >= 10 ? 2 : 1;",
               "if ((engine->aligned_tiles || farfield) && waste <= 0.06)",
               "const int candidates[4] = {8, 4, 2, 1};",
               "tiling.n_tiles = (int)((n + tiling.length - 1)/tiling.length);")


def far_series_kept(grid):
    """shape_of: the series is dropped where kFarRatio*0.5*length >= cut_off*n_per_v."""
    t = tiling(grid, 1)
    return not FAR_RATIO*0.5*t.length >= float(grid.cut_off)*grid.n_per_v


FAR_TEXT = "if (s.farfield && kFarRatio*0.5*(double)s.tiling.length >= (double)rq.cut_off*rq.n_per_v)"


def tile_bounds(t, tile, grid):
    """tile_bounds (accumulate.h)."""
    npv, n = grid.n_per_v, points(grid)
    if t.aligned:
        cell, sub = divmod(tile, t.per_cell)
        i0 = cell*npv + sub*t.length
        i1 = min(i0 + t.length - 1, (cell + 1)*npv - 1)
    else:
        i0 = tile*t.length
        i1 = i0 + t.length - 1
    return i0, min(i1, n - 1)


def plan_parts(tab, grid, farfield=0, forced=0):
    """plan_for's `parts` per tile of a plan without the far-field series (lanes_plans.inc):
    weight = rows with nu inside the tile's window, target = max(floor_lines, total/(8*1536) + 1),
    parts = min(64, ceil(weight/target))."""
    assert not farfield
    t = tiling(grid, farfield, forced)
    npv = grid.n_per_v
    weight = []
    for tile in range(t.n_tiles):
        i0, i1 = tile_bounds(t, tile, grid)
        lo = float((i0 + npv - 1)//npv + grid.v0 - grid.cut_off - 1) - 0.05
        hi = float(i1//npv + grid.v0 + grid.cut_off) + 1.05
        weight.append(int(np.searchsorted(tab.nu, hi, "left") - np.searchsorted(tab.nu, lo, "left")))
    floor_lines = ITEM_FLOOR if t.n_tiles < 1024 else 2048
    target = max(floor_lines, sum(weight)//(8*1536) + 1)
    return [max(1, min(MOST_PARTS, (w + target - 1)//target)) for w in weight]


PLAN_TEXT = ("const long long floor_lines = n_tiles < 1024 ? 128 : 2048;",
             "const long long target = std::max<long long>(floor_lines, total/(8*1536) + 1);",
             "int parts = (int)std::min<long long>(64, (weight[t] + target - 1)/target);",
             "double lo = (double)((i0 + g.n_per_v - 1)/g.n_per_v + g.v0 - g.cut_off - 1) - 0.05;",
             "double hi = (double)(i1/g.n_per_v + g.v0 + g.cut_off) + 1.05;")


def partial_slots(tab, grid):
    return sum(p for p in plan_parts(tab, grid) if p > 1)


# -- levels_per_pass ---------------------------------------------------------------------------
def pedestal_bytes_per_level(n_lines, n_cells, cut_off):
    """pedestal.h."""
    stride = 2*cut_off + 3
    run_count = min(n_lines, 4*(n_cells + 2*cut_off + 2) + n_lines//RUN_CUT)
    return n_lines*8 + run_count*(RUN_META_BYTES + RUN_LINK_BYTES + stride*8 + 16 +
                                  8*SWEEP_BUFFERS) + 4*(n_cells + stride)*8


def per_level_bound(tab, grid, farfield=0):
    """An upper bound of levels_per_pass's per_level over every variant of a call: MOST_PARTS
    partial slots for every tile, host output, the pedestal."""
    t = tiling(grid, farfield)
    return t.n_tiles*MOST_PARTS*64*t.points*8 + tab.num_lines*(WING_BYTES + CORE_BYTES) + \
        t.n_tiles*SCHEDULE_BYTES + points(grid)*8 + \
        pedestal_bytes_per_level(tab.num_lines, grid.vn - grid.v0, grid.cut_off)


def levels_per_pass(workspace_bytes, per_level, n_levels):
    chunk = max(1, workspace_bytes//max(per_level, 1))
    return min(min(chunk, n_levels), ROW)


PASS_TEXT = ("const long long per_level = plan.partial_slots*64*s.points*8 + n_lines*(long long)"
             "(sizeof(LineWing) + sizeof(LineCore)) +",
             "(long long)s.tiling.n_tiles*sizeof(TileSchedule) +",
             "(t.out_device ? 0 : s.n_long*8) +",
             "(rq.remove_pedestal ? pedestal_bytes_per_level(n_lines, rq.vn - rq.v0, rq.cut_off) : 0);",
             "const long long chunk = std::max(1ll, engine->workspace_bytes/std::max(per_level, 1ll));",
             "return std::min<long long>(std::min<long long>(chunk, rq.n_levels), 65535);")
PEDESTAL_TEXT = ("const long long stride = 2*cut_off + 3;",
                 "const long long runs = std::min<long long>(n_lines, 4ll*(n_cells + 2*cut_off + 2) + "
                 "n_lines/kRunCut);",
                 "return n_lines*8 + runs*((long long)(sizeof(RunMeta) + sizeof(RunLink)) + stride*8 + 16 +",
                 "8ll*kPedestalSweepBuffers) + 4ll*(n_cells + stride)*8;")

# workspace_bytes of the big calls: the cap of 65535 is what cuts their passes (the host test);
# and one that cuts passes of about 20 000 levels.
WORKSPACE = 64 << 30
DEFAULT_WORKSPACE = 4 << 30


def per_level(tab, grid, out_device, remove_pedestal):
    """levels_per_pass's per_level of a call without the far-field series, exactly."""
    t = tiling(grid, 0)
    return partial_slots(tab, grid)*64*t.points*8 + tab.num_lines*(WING_BYTES + CORE_BYTES) + \
        t.n_tiles*SCHEDULE_BYTES + (0 if out_device else points(grid)*8) + \
        (pedestal_bytes_per_level(tab.num_lines, grid.vn - grid.v0, grid.cut_off)
         if remove_pedestal else 0)


PASS_LEVELS = 20000
LEAST_WORKSPACE = 1 << 20       # engine.hip: lbl_set_option refuses less


def small_workspace(tab, grid, out_device, remove_pedestal):
    """workspace_bytes that cuts such a call into passes of exactly PASS_LEVELS levels."""
    return PASS_LEVELS*per_level(tab, grid, out_device, remove_pedestal)


def source(name):
    return (CSRC / name).read_text()


def in_text(text, statement):
    """`statement` in `text`, white space apart."""
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    return squeeze(statement) in squeeze(text)


# ---------------------------------------------------------------------------------------------
# Part 2: the largest grid the entry takes.  1 073 709 056 points, 32 767 short of the refusal
# (shape_of: more than 0x3fffffff points); one more point per cm-1 is refused.
BIG = Grid(2000, 2000 + 32768, 32767, 25)
REFUSED = Grid(2000, 2000 + 32768, 32768, 25)
MOST_POINTS = 0x3fffffff                            # compute_stages.inc: shape_of
BIG_LEVEL = (250., 1000., 4.e-4)        # 0.01 atm: y from 0.04 (34 768 cm-1) to 0.9 (2 000 cm-1)
# Offsets [cm-1] of a cluster's lines from its anchor; the anchors are the wavenumbers of the grid
# indices 0, 2^28, 2^29, 3 2^28 and n - 1.  Lines a few grid points from the anchor (cores that
# straddle the index), within a cm-1 (core-range rows on either side) and up to a dozen cm-1 away
# (windows that begin or end near it); the first and the last cluster also hold lines outside the
# grid whose windows reach into it.
_OFFSETS = (
    (-11.3, -0.41, 2.e-4, 0.013, 0.27, 3.6, 9.2, 14.8),
    (-9.7, -0.62, -3.e-4, 1.5e-4, 0.38, 4.4, 12.1),
    (-12.4, -5.3, -0.3, -1.e-4, 6.e-5, 0.004, 0.71, 7.7, 10.9),
    (-8.8, -0.05, 2.e-4, 0.9, 6.1, 11.5),
    (-13.6, -7.2, -2.9, -0.33, -0.004, -1.e-4, 0.19, 0.8, 5.5, 10.6),
)
ANCHOR_INDEX = (0, 1 << 28, 1 << 29, 3 << 28, points(BIG) - 1)


def big_table():
    """About 40 lines in five clusters (ascending), strengths within half a decade, half-widths of
    0.14 .. 0.18 cm-1/atm (the rescaling of pedestal_run_cases.near_integer_table)."""
    if "big" not in _tables:
        from pylbl_amd import synthetic
        nu = np.concatenate([BIG.v0 + index/BIG.n_per_v + np.asarray(offsets)
                             for index, offsets in zip(ANCHOR_INDEX, _OFFSETS)])
        assert np.all(np.diff(nu) > 0.)
        made = synthetic.line_table("CO2", float(nu[0]), float(nu[-1]) + 1., num_lines=nu.size,
                                    seed=431, tips_range=(150, 400))
        made.nu = nu
        made.sw = 10.**(-21. + (np.log10(made.sw) + 30.)/22.)
        made.gamma_air = 0.14 + (made.gamma_air - 0.03)*(0.04/0.09)
        _tables["big"] = made
    return _tables["big"]


def cluster_of_row():
    return np.repeat(np.arange(len(_OFFSETS)), [len(o) for o in _OFFSETS])


def windows(centre, grid):
    """[first, last] and status per line from its shifted centre: spectra.c:48-62 as prepare_line
    states it (status 0: the window begins right of the grid; last < first: it ends left of it)."""
    n = points(grid)
    fl = np.floor(centre)
    first = np.trunc((fl - grid.cut_off - float(grid.v0))*grid.n_per_v).astype(np.int64)
    status = np.where(first >= n, 0, 1)
    last = np.trunc((fl + grid.cut_off + 1 - float(grid.v0))*grid.n_per_v).astype(np.int64)
    first = np.where(status == 1, np.maximum(first, 0), first)
    last = np.where(status == 1, np.minimum(last, n - 1), 0)
    return first, last, status


WINDOW_TEXT = ("const double fl = floor(centre);",
               "int first = (int)((fl - g.cut_off - (double)g.v0)*g.n_per_v);",
               "if (first >= g.n)", "if (first < 0) first = 0;",
               "last = (int)((fl + g.cut_off + 1 - (double)g.v0)*g.n_per_v);",
               "if (last >= g.n) last = g.n - 1;")


def line_limits(tab, level, grid):
    """Per line, from prepare_line's limits: the half-widths [cm-1] of the inner regions
    (|x| < xlim1) and of the core range (|x| < xlim0) around the centre, and y."""
    centre, alpha, gamma, y = line_widths(tab, level)
    repwid = math.sqrt(math.log(2.))/alpha
    xlim0 = np.sqrt(15100. + y*(40. - y*3.6))
    xlim1 = np.where(y >= 8.425, 0., np.sqrt(np.maximum(164. - y*(4.3 + y*1.8), 0.)))
    xlim1 = np.where(y <= 1.e-6, xlim0, xlim1)
    assert np.all(y < 70.55)
    return centre, xlim1/repwid, xlim0/repwid, y


def covered(first, last, status, n):
    """Sorted, merged [a, b] index ranges that some window covers, and the gaps between them."""
    live = (status == 1) & (last >= first)
    spans = sorted(zip(first[live].tolist(), last[live].tolist()))
    merged = []
    for a, b in spans:
        if merged and a <= merged[-1][1] + 1:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    gaps, at = [], 0
    for a, b in merged:
        if a > at:
            gaps.append((at, a - 1))
        at = b + 1
    if at <= n - 1:
        gaps.append((at, n - 1))
    return [tuple(m) for m in merged], gaps


def wavenumbers(grid, first, last):
    """v[i] = v0 + i*dv as absorption.c:36-40 forms it (product rounded, then the sum)."""
    dv = 1./grid.n_per_v
    return float(grid.v0) + np.arange(first, last + 1, dtype=np.float64)*dv

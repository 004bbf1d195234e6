"""CPU checks behind tests/test_gpu_many_levels.py: the expressions tests/many_levels_cases.py
restates are the sources' (held against their text), every pattern level is the kind of level it
is listed as (from prepare_line's y, restated and held against the oracle's own widths), every
table and grid reaches the kernels it is named for, the cap of 65535 levels -- not workspace_bytes
-- is what cuts the passes of the big calls, and the clusters of the 2^30-point grid lie where the
GPU test looks for them, with rows of every kind."""
import re

import numpy as np
import pytest

from tests import many_levels_cases as cases
from tests import pedestal_run_cases as runs

NAMES = tuple(cases.GRIDS)


def test_constants_and_expressions_are_the_sources():
    stages = cases.source("compute_stages.inc")
    prep = cases.source("line_prep.h")
    plans = cases.source("lanes_plans.inc")
    pedestal = cases.source("pedestal.h")
    accumulate = cases.source("accumulate.h")
    schedule = cases.source("tile_schedule.h")
    for text, statements in ((stages, cases.INNER_TEXT + cases.PASS_TEXT + (cases.FAR_TEXT,)),
                             (prep, cases.Y_TEXT), (plans, cases.TILING_TEXT + cases.PLAN_TEXT),
                             (pedestal, cases.PEDESTAL_TEXT)):
        for statement in statements:
            assert cases.in_text(text, statement), statement
    assert "constexpr int kInlineLevels = %d;" % cases.INLINE_LEVELS in schedule
    assert runs.constant(cases.source("pedestal_runs.h"), "kScanThreads") == cases.SCAN_THREADS
    assert "#define LBL_FAR_RATIO %s\n" % repr(cases.FAR_RATIO).rstrip("0") in accumulate
    assert runs.constant(pedestal, "kRunCut") == cases.RUN_CUT
    assert runs.constant(pedestal, "kPedestalSweepBuffers") == cases.SWEEP_BUFFERS
    # the record sizes of per_level
    assert "struct alignas(32) LineWing" in prep and cases.WING_BYTES == 32
    assert "static_assert(sizeof(LineCore) == %d," % cases.CORE_BYTES in prep
    assert "struct alignas(32) TileSchedule" in accumulate and cases.SCHEDULE_BYTES == 32
    assert "static_assert(sizeof(RunLink) == %d," % cases.RUN_LINK_BYTES in pedestal
    body = re.search(r"struct RunMeta\s*\{(.*?)\};", pedestal, re.S).group(1)
    fields = re.findall(r"^\s*(int|double)\s+([^;]+);", body, re.M)
    size = sum((4 if kind == "int" else 8)*len(names.split(",")) for kind, names in fields)
    assert size == cases.RUN_META_BYTES and size % 8 == 0
    # the level is a launch row of every kernel of a pass
    for text, kernel in ((schedule, "prologue_kernel"), (schedule, "schedule_kernel")):
        at = text.index("void %s(" % kernel)
        assert "const int level = blockIdx.y;" in text[at:at + 1500], kernel
    at = pedestal.index("void pedestal_apply_kernel(")
    assert "const int level = blockIdx.y;" in pedestal[at:at + 1500]


def test_counts_and_passes():
    assert cases.ROW % cases.K != 0 and (2*cases.ROW) % cases.K != 0    # later passes start elsewhere
    passes = {count: [min(cases.ROW, count - base) for base in range(0, count, cases.ROW)]
              for count in cases.COUNTS}
    assert passes[cases.ROW] == [cases.ROW]
    assert passes[cases.ROW + 1] == [cases.ROW, 1] and 1 <= cases.INLINE_LEVELS
    assert passes[cases.ROW + 12] == [cases.ROW, 12] and 12 > cases.INLINE_LEVELS
    assert passes[2*cases.ROW + 3] == [cases.ROW, cases.ROW, 3]
    for count in cases.WHOLE_PATTERN_COUNTS:
        assert min(passes[count]) >= cases.K
    t, p, x = cases.levels(cases.ROW + 12)
    assert (t[cases.ROW], p[cases.ROW], x[cases.ROW]) == tuple(cases.PATTERN[cases.ROW % cases.K])


@pytest.mark.parametrize("name", NAMES)
def test_pattern_levels_are_what_they_are_listed_as(oracle, name):
    table, grid = cases.table(name), cases.GRIDS[name]
    nu = table.nu
    assert np.all(np.diff(nu) > 0.)
    assert np.all((nu <= grid.vn + grid.cut_off + 1) & (nu >= grid.v0 - (grid.cut_off + 1)))
    y = {}
    for level in range(cases.K):
        centre, alpha, gamma, y[level] = cases.line_widths(table, cases.PATTERN[level])
        # the restatement against the oracle's own scalars (spectra.c:22-29), to rounding
        t, p, x = cases.PATTERN[level]
        _, extras = oracle.absorption_port(table, t, p, x, grid.v0, grid.vn, grid.n_per_v,
                                           cut_off=grid.cut_off, want_derived=True)
        derived = extras["derived"]
        assert np.array_equal(derived[:, 0], centre)
        assert np.allclose(derived[:, 1], alpha, rtol=1e-14, atol=0.)
        assert np.allclose(derived[:, 2], gamma, rtol=1e-14, atol=0.)
        assert np.min(np.abs(centre - np.round(centre))) >= runs.INTEGER_MARGIN
    assert y[cases.NEAR_VACUUM].max() <= 1.e-6/2.
    assert y[cases.NO_INNER].min() >= 8.425*1.01 and y[cases.NO_INNER].max() < 70.55
    assert cases.inner_possible(table, cases.PATTERN[cases.NO_INNER], grid) == 0
    assert y[cases.LORENTZ].max() >= 70.55*1.01
    for level in (5, 6):        # ordinary: inner regions, far wing, nothing special
        assert 1.e-6 < y[level].min() and y[level].max() < 8.425
        assert cases.inner_possible(table, cases.PATTERN[level], grid) == 1
    # the pedestal's runs: every row opens one at 1 atm, a window is one at 10 Pa
    top = runs.mirror(table, cases.PATTERN[cases.EVERY_ROW, 1], grid)
    assert top.run_count == table.num_lines and top.opens.all()
    low = runs.mirror(table, cases.PATTERN[cases.ONE_RUN, 1], grid)
    windows = {(a, b) for a, b in zip(low.first, low.last) if a <= b}
    assert low.run_count == len(windows) < table.num_lines//2 + 1
    assert table.num_lines < runs.RUN_CUT


def test_pattern_levels_give_different_rows(oracle):
    """A row taken from another level of the call is a visibly different row."""
    table, grid = cases.table("small"), cases.SMALL
    rows = [oracle.absorption_port(table, t, p, x, grid.v0, grid.vn, grid.n_per_v,
                                   cut_off=grid.cut_off)[0] for t, p, x in cases.PATTERN]
    for a in range(cases.K):
        for b in range(a):
            apart = np.abs(rows[a] - rows[b])/np.maximum(rows[a], rows[b])
            assert np.median(apart) > 1.e-2, (a, b)


def test_tables_reach_the_kernels_they_are_named_for():
    small, split, scan = (cases.table(name) for name in ("small", "split", "scan"))
    assert 1 <= cases.tiling(cases.SMALL, 0).n_tiles <= 2
    assert small.num_lines == 36 and cases.plan_parts(small, cases.SMALL) == [1]
    assert cases.partial_slots(small, cases.SMALL) == 0
    # split: one tile cut into parts, combine_kernel at every level; one block of run_find_kernel
    assert cases.plan_parts(split, cases.SMALL) == [2] and cases.partial_slots(split, cases.SMALL) == 2
    assert split.num_lines == 252 <= cases.SCAN_THREADS
    # scan: more than one block of run_find_kernel per level
    assert scan.num_lines == 612 and -(-scan.num_lines//cases.SCAN_THREADS) == 3
    assert cases.partial_slots(scan, cases.SMALL) == 5
    # far: the series stays on, and some line of every tile is left to it
    assert cases.far_series_kept(cases.FAR) and not cases.far_series_kept(cases.SMALL)
    far = cases.tiling(cases.FAR, 1)
    assert far.aligned and far.length == 64 and far.n_tiles == 8
    half = 0.5*(far.length - 1)/cases.FAR.n_per_v
    for tile in range(far.n_tiles):
        i0, i1 = cases.tile_bounds(far, tile, cases.FAR)
        centre = cases.FAR.v0 + 0.5*(i0 + i1)/cases.FAR.n_per_v
        away = np.abs(cases.table("far").nu - centre)
        assert np.any((away > cases.FAR_RATIO*half + 0.1) & (away < cases.FAR.cut_off))
    # pieces: a streamed call has more than one run of tiles to deliver
    assert cases.tiling(cases.FAR, 0).n_tiles == 4


@pytest.mark.parametrize("name", NAMES)
def test_the_cap_of_65535_cuts_the_passes(name):
    table, grid = cases.table(name), cases.GRIDS[name]
    for farfield in (0, 1):
        bound = cases.per_level_bound(table, grid, farfield)
        assert cases.WORKSPACE//bound >= cases.ROW, (name, farfield)
        for out_device in (False, True):
            for pedestal in (False, True):
                exact = cases.per_level(table, grid, out_device, pedestal)
                assert exact <= cases.per_level_bound(table, grid, 0)
    for count in cases.COUNTS:
        for per_level in (1, cases.per_level_bound(table, grid, 0), cases.per_level_bound(table, grid, 1)):
            assert cases.levels_per_pass(cases.WORKSPACE, per_level, count) == min(count, cases.ROW)
    # and the budget that cuts passes of 20 000 levels
    for out_device in (False, True):
        for pedestal in (False, True):
            budget = cases.small_workspace(table, grid, out_device, pedestal)
            assert budget >= cases.LEAST_WORKSPACE
            exact = cases.per_level(table, grid, out_device, pedestal)
            assert cases.levels_per_pass(budget, exact, cases.ROW + 12) == cases.PASS_LEVELS
    assert "value >= (1 << 20)" in cases.source("engine.hip")


# ---------------------------------------------------------------------------------------------
# The largest grid.
def test_largest_grid_is_the_largest():
    n = cases.points(cases.BIG)
    assert n == 1073709056 and cases.MOST_POINTS - n == 32767
    assert cases.points(cases.REFUSED) == cases.MOST_POINTS + 1
    stages = cases.source("compute_stages.inc")
    assert cases.in_text(stages, "if (s.n_long > 0x%x)" % cases.MOST_POINTS)
    assert cases.in_text(stages, 's.n_long = (long long)(rq.vn - rq.v0)*rq.n_per_v;')
    for statement in cases.WINDOW_TEXT:
        assert cases.in_text(cases.source("line_prep.h"), statement), statement
    # the two tilings the GPU test runs: four points per lane, and eight with the series
    plain, far = cases.tiling(cases.BIG, 0, forced=4), cases.tiling(cases.BIG, 1)
    assert (plain.points, plain.aligned, plain.length) == (4, 0, 256) and plain.n_tiles > 4000000
    assert (far.points, far.aligned, far.length) == (8, 1, 512) and cases.far_series_kept(cases.BIG)
    assert cases.tiling(cases.BIG, 0, forced=8).length == 512


def test_restated_windows_are_the_references(oracle):
    """first / last of spectra.c:48-62 through the oracle's own derived scalars: on the big grid's
    wavenumbers at one point per cm-1 -- where the restated formula, scaled by prepare_line's
    n_per_v, is the big grid's -- and on a grid of seven points per cm-1 that clips windows at
    both ends."""
    table = cases.big_table()
    t, p, x = cases.BIG_LEVEL
    coarse = cases.Grid(cases.BIG.v0, cases.BIG.vn, 1, cases.BIG.cut_off)
    _, extras = oracle.absorption_port(table, t, p, x, coarse.v0, coarse.vn, 1,
                                       cut_off=coarse.cut_off, want_derived=True)
    derived = extras["derived"]
    centre = cases.line_widths(table, cases.BIG_LEVEL)[0]
    assert np.array_equal(derived[:, 0], centre) and np.all(derived[:, 6] == 1.)
    first, last, status = cases.windows(centre, coarse)
    assert np.array_equal(first, derived[:, 4]) and np.array_equal(last, derived[:, 5])
    # scaled as prepare_line scales them: cells to points, the last cell's end to n - 1
    big_first, big_last, big_status = cases.windows(centre, cases.BIG)
    n, npv = cases.points(cases.BIG), cases.BIG.n_per_v
    assert np.array_equal(big_first, first*npv) and np.all(big_status == 1)
    assert np.array_equal(big_last, np.minimum((np.floor(centre) + coarse.cut_off + 1 - coarse.v0)
                                               .astype(np.int64)*npv, n - 1))
    assert np.array_equal(big_last == n - 1, last == cases.points(coarse) - 1)
    small = cases.Grid(2298, 2309, 7, 2)
    narrow = cases.table("small")
    for level in cases.PATTERN:
        _, extras = oracle.absorption_port(narrow, *level, small.v0, small.vn, small.n_per_v,
                                           cut_off=small.cut_off, want_derived=True)
        derived = extras["derived"]
        first, last, status = cases.windows(derived[:, 0], small)
        assert np.array_equal(status, derived[:, 6])
        live = status == 1
        assert np.array_equal(first[live], derived[live, 4])
        assert np.array_equal(last[live], derived[live, 5])
        assert (first[live] == 0).any() and (last[live] == cases.points(small) - 1).any()


def test_clusters_lie_on_the_index_limits():
    table, grid = cases.big_table(), cases.BIG
    n, npv = cases.points(grid), grid.n_per_v
    assert 35 <= table.num_lines <= 45 and np.all(np.diff(table.nu) > 0.)
    assert np.all((table.nu <= grid.vn + grid.cut_off + 1) & (table.nu >= grid.v0 - grid.cut_off - 1))
    centre, inner, core, y = cases.line_limits(table, cases.BIG_LEVEL, grid)
    first, last, status = cases.windows(centre, grid)
    merged, gaps = cases.covered(first, last, status, n)
    assert len(merged) == 5 and len(gaps) == 4          # the clusters' windows do not meet
    assert sum(b - a + 1 for a, b in gaps) > 0.98*n     # nearly all of the grid lies outside them
    cluster = cases.cluster_of_row()
    at = (centre - grid.v0)*npv                         # the centres as (fractional) grid indices
    for c, (a, b) in enumerate(merged):
        rows = np.flatnonzero(cluster == c)
        assert 6 <= rows.size <= 10
        anchor = cases.ANCHOR_INDEX[c]
        assert a <= anchor <= b
        if 0 < anchor < n - 1:
            # windows on both sides of the limit, and rows that begin or end within a tile of it
            assert a < anchor - 300000 and b > anchor + 300000
            assert anchor < 1 << 30 and anchor % (1 << 28) == 0
        # inner points (|x| < xlim1) on both sides of the anchor, of one line
        straddles = (np.abs(at[rows] - anchor) < 0.5*inner[rows]*npv) & (inner[rows]*npv > 100)
        assert straddles.any(), c
        for row in rows:
            lo, hi = max(first[row], 0), min(last[row], n - 1)
            reach_inner, reach_core = inner[row]*npv, core[row]*npv
            # far-wing rows: the window reaches more than a tile beyond the core range
            assert max(at[row] - reach_core - lo, hi - at[row] - reach_core) > 10*512, row
            # core-range rows: whole rows of 64 points between xlim1 and xlim0
            assert reach_core - reach_inner > 10*512, row
            assert 0. < y[row] < 8.425 and reach_inner > 100, row
    # the first and last clusters: lines outside the grid whose windows reach in, windows clipped
    assert (table.nu[cluster == 0] < grid.v0).sum() >= 2 and np.all(first[cluster == 0] == 0)
    assert (table.nu[cluster == 4] > grid.vn).sum() >= 2 and np.all(last[cluster == 4] == n - 1)
    assert n - 1 > 10**9        # the last cluster lies past index 1e9 (line_prep.h clamps there)

"""CPU-only checks of tests/inner_pass_cases.py, the inputs and the numpy mirror behind
tests/test_gpu_inner_pass.py: that the tables are the ones described (y values, one decade of
strengths, far lines beyond any core), that the mirror takes exactly the (line, point) pairs the
oracle counts in w4 regions 2-3 and CPF12 (regions[2:6], see inner_pass_cases), and that every
case reaches what it is named for -- batch counts, list lengths and carries, segments cut by tiles,
windows and the ends of the grid, tiles split into parts whose wavefronts all have work."""
from pathlib import Path

import numpy as np
import pytest

from tests import farfield_cases as fc
from tests import inner_pass_cases as ip

CSRC = Path(__file__).resolve().parents[1] / "pylbl_amd" / "csrc"


@pytest.fixture(scope="module")
def mirrors(oracle):
    runs = ip.Runs(oracle)
    kept = {}

    def get(key):
        if key not in kept:
            run = runs(key)
            kept[key] = (run, ip.mirror(run.case, run.table, run.derived))
        return kept[key]
    return get


def waves_of(m, tile, part=0):
    return [m.passes[(tile, part, wave)] for wave in range(4)]


def test_constants_are_the_kernels():
    lines = (CSRC / "accumulate_lines.h").read_text()
    assert "constexpr int kInnerQueue = %d;" % ip.QUEUE in lines
    assert "constexpr int kInnerList = %d;" % ip.LIST in lines
    assert "count[c] >= 64 || (drain && count[c] > 0)" in lines
    profile = (CSRC / "voigt_profile.h").read_text()
    assert "constexpr int kInnerClasses = %d;" % ip.CLASSES in profile
    assert "return abx >= lim.two ? 0 : (abx <= lim.four ? 1 : 2);" in profile
    assert "lim.two = (y <= 0.000001) ? 1.e300 : 6.8 - y;" in profile
    assert "lim.four = 18.1*y + 1.65;" in profile
    plans = (CSRC / "lanes_plans.inc").read_text()
    assert "const long long floor_lines = n_tiles < 1024 ? 128 : 2048;" in plans
    assert "total/(8*1536) + 1" in plans
    stages = (CSRC / "compute_stages.inc").read_text()
    assert "return (rq.cut_off - 1. <= reach + tile_width + 1.) ? 1 : 0;" in stages


@pytest.mark.parametrize("key", sorted(ip.CASES))
def test_tables_and_pair_counts(mirrors, key):
    run, m = mirrors(key)
    case, table, rec = run.case, run.table, m.records
    # The table: at most 2 000 lines, one decade of strengths, the y values asked for, every line
    # inside the range rule (absorption.c:80-83) and evaluated.
    assert table.num_lines <= ip.MOST_LINES
    assert ip.SW_LOW <= table.sw.min() and table.sw.max() <= ip.SW_HIGH
    assert table.nu.min() >= case.v0 - case.cut_off - 1
    assert table.nu.max() <= case.vn + case.cut_off + 1
    assert np.all(run.derived[:, 6] != -1.)
    live = rec.live
    assert np.all(np.abs(rec.y[live] - run.lines.y[live]) <= 1.e-5*run.lines.y[live])
    assert set(run.lines.y) == set(ip.Y_VALUES)
    assert np.all(rec.y[live & (run.lines.y == 5.e-7)] <= 0.000001)
    assert np.all(rec.y[live & (run.lines.y == 8.42)] < 8.425)
    assert np.all(rec.xlim1[live] > 0.)
    # Beyond any core: the reach of a line is below 1 cm-1 (so is the level's bound on it), the
    # far lines lie 3 cm-1 or more from the cluster's tile.
    reach = np.max(rec.xlim0[live]/rec.repwid[live])
    assert reach < 1.
    assert m.level.core_reach*(case.vn + 1.) < 1.
    far = table.nu[~run.lines.cluster]
    near = table.nu[run.lines.cluster]
    if far.size:
        assert np.min(np.abs(far[:, None] - near[None, :])) >= 3.
    # No line so near a search key of a tile's core range that the rounding of the level's
    # core_reach could move it across (the keys carry a margin of 1e-9 themselves), nor so near an
    # integer that shift_max (1e-12) could.
    for s in m.schedules:
        for key_value in (s.v_lo - s.core, s.v_hi + s.core):
            assert np.min(np.abs(m.nu - key_value)) > 1.e-9
    assert np.min(np.abs(m.nu - np.round(m.nu))) > 1.e-9
    # Every list is what share_of promises: the shares of a tile tile its core range.
    for t, s in enumerate(m.schedules):
        cuts = [ip.share_of(s.c1, s.c2, piece, int(m.parts[t])*4)
                for piece in range(int(m.parts[t])*4)]
        assert cuts[0][0] == s.c1 and cuts[-1][1] == s.c2
        assert all(a[1] == b[0] for a, b in zip(cuts[:-1], cuts[1:]))
    # The pairs the pass takes are the oracle's evaluations in regions 2, 3 and CPF12.
    pairs = sum(p.pairs for p in m.passes.values())
    print("%s: %d tiles, %d (line, point) pairs" % (case.name, m.tiling.n_tiles, pairs))
    assert pairs == int(run.regions[2:6].sum())
    assert pairs > 1000


@pytest.mark.parametrize("n_cluster,adding,last", [(512, 4, 32), (516, 5, 1), (600, 5, 22)])
@pytest.mark.parametrize("points", [1, 2, 4, 8])
def test_a_many_batches_in_an_unsplit_tile(mirrors, n_cluster, adding, last, points):
    run, m = mirrors("A-%d-P%d" % (n_cluster, points))
    assert m.tiling.n_tiles >= 1024 and not m.tiling.aligned
    tile = run.case.tile
    s = m.schedules[tile]
    assert m.parts[tile] == 1
    # The cluster lies inside the tile's own span: its core range is the cluster.
    assert s.c2 - s.c1 == n_cluster and np.all(run.lines.cluster[s.c1:s.c2])
    assert np.all((m.nu[s.c1:s.c2] > s.v_lo) & (m.nu[s.c1:s.c2] < s.v_hi))
    for p in waves_of(m, tile):
        assert p.lines == n_cluster//4
        assert len(p.batch_sizes) == adding and p.adding == adding
        assert p.batch_sizes[-1] == last and p.batch_sizes[:-1] == [32]*(adding - 1)


def test_b_list_carries_and_long_segments(mirrors):
    run, m = mirrors("B-P8")
    assert m.tiling.n_tiles == 1032 and run.case.n == 528000
    tile = run.case.tile
    assert m.parts[tile] == 1 and m.schedules[tile].c2 - m.schedules[tile].c1 == 600
    waves = waves_of(m, tile)
    before = [b for p in waves for c in range(ip.CLASSES) for b in p.before[c]]
    left = [l for p in waves for c in range(ip.CLASSES) for l in p.left[c]]
    print("B: list lengths before a flush up to %d, left behind up to %d, %d flushes, segments "
          "over up to %d chunks" % (max(before), max(left), len(before),
                                    max(p.most_chunks for p in waves)))
    for p in waves:
        assert p.adding == 5 and p.lines == 150
        assert max(max(b) for b in p.before) == ip.LIST - 1
    assert (64, 0) in list(zip(before, left))
    assert 63 in left
    assert max(p.most_chunks for p in waves) >= 4
    for c in range(ip.CLASSES):
        assert any(l > 0 for p in waves for l in p.left[c]), c
    # Other tile cuts on the same grid and table.
    run4, m4 = mirrors("B-P4")
    assert m4.tiling.n_tiles == 2063 and run4.table is run.table
    busiest = max(m4.passes.values(), key=lambda p: p.pairs)
    assert busiest.adding >= 4 and max(max(b) for b in busiest.before if b) == ip.LIST - 1
    assert sum(p.cut_by_tile for p in m4.passes.values()) > 0


@pytest.mark.parametrize("points", [1, 8])
def test_c_tile_cuts_and_grid_edges(mirrors, points):
    run, m = mirrors("C-boundary-P%d" % points)
    assert m.tiling.n_tiles >= 1024
    for tile in (ip.A_TILE - 1, ip.A_TILE):
        waves = waves_of(m, tile)
        assert sum(p.cut_by_tile for p in waves) > 0, tile
        assert sum(p.adding for p in waves) >= 8
    s0, s1 = m.schedules[ip.A_TILE - 1], m.schedules[ip.A_TILE]
    inside = run.table.nu[run.lines.cluster]
    assert np.any(inside < s0.v_hi) and np.any(inside > s1.v_lo)

    run, m = mirrors("C-first-point-P%d" % points)
    waves = waves_of(m, 0)
    assert np.any(run.table.nu < run.case.v0)
    assert sum(p.begins_at_zero for p in waves) > 0
    assert sum(p.outside_grid for p in waves) > 0
    assert sum(p.adding for p in waves) >= 8

    run, m = mirrors("C-last-point-P%d" % points)
    last = m.tiling.n_tiles - 1
    waves = waves_of(m, last)
    assert m.schedules[last].i1 == run.case.n - 1
    assert sum(p.ends_at_last for p in waves) > 0
    assert sum(p.outside_grid for p in waves) > 0
    assert sum(p.adding for p in waves) >= 8


@pytest.mark.parametrize("points", [1, 2, 4, 8])
def test_d_split_tiles(mirrors, points):
    run, m = mirrors("D-P%d" % points)
    assert m.tiling.n_tiles < 1024
    tile = run.case.tile
    parts = int(m.parts[tile])
    s = m.schedules[tile]
    assert parts >= 5
    assert s.c2 - s.c1 >= 600 and np.all((m.nu[run.lines.cluster] > s.v_lo) &
                                         (m.nu[run.lines.cluster] < s.v_hi))
    points_of = []
    for part in range(parts):
        for p in waves_of(m, tile, part):
            assert p.core[1] > p.core[0] and np.all(run.lines.cluster[p.core[0]:p.core[1]])
            assert p.pairs > 0
        points_of.append(np.unique(np.concatenate([p.points for p in waves_of(m, tile, part)])))
    shared = sum(np.intersect1d(points_of[a], points_of[b]).size > 0
                 for a in range(parts) for b in range(a + 1, parts))
    print("D, P = %d: %d parts, %d pairs of parts share a grid point" % (points, parts, shared))
    assert shared >= 1


@pytest.mark.parametrize("cut_off", [0, 1, 2])
@pytest.mark.parametrize("points", [1, 8])
def test_e_every_range_at_small_cut_offs(mirrors, cut_off, points):
    run, m = mirrors("E-cut%d-P%d" % (cut_off, points))
    assert ip.inner_everywhere(run.case) == 1
    passes = list(m.passes.values())
    nu = run.table.nu
    assert np.any((nu > 1000.97) & (nu < 1001.)) and np.any((nu > 1001.) & (nu < 1001.03))
    if cut_off > 0:
        # A window ends cut_off cm-1 or more from its line (spectra.c:48-62) and an inner range
        # reaches 0.14 cm-1: only at cut_off = 0 can a window cut a segment, or a line of a
        # clipped range have inner points in the tile its window ends in.  On this grid the
        # windows of cut-offs 1 and 2 are the whole grid.
        assert sum(p.cut_by_window for p in passes) == 0
        return
    # The walk covers every range: lists longer than the share of the core range.
    assert any(p.lines > p.core[1] - p.core[0] for p in passes)
    assert sum(p.cut_by_window for p in passes) > 0
    assert sum(p.first_inside for p in passes) > 0
    assert sum(p.last_inside for p in passes) > 0
    # Lines either side of 1001 have different windows, and the tile that holds index 1000 has
    # lines with inner points in its clipped ranges [lo, a1) and [a2, hi).
    assert len(set(m.records.first)) > 1 and len(set(m.records.last)) > 1
    tile = ip.tile_of_index(m.tiling, run.case, 1000)
    s = m.schedules[tile]
    rec = m.records
    for clipped in (np.arange(s.lo, s.a1), np.arange(s.a2, s.hi)):
        assert clipped.size > 0
        reaches = (np.minimum(rec.inner_last[clipped], np.minimum(rec.last[clipped], s.i1)) >=
                   np.maximum(rec.inner_first[clipped], np.maximum(rec.first[clipped], s.i0)))
        assert reaches.any()


def test_f_the_series_on(mirrors):
    for key in ("F-A-600-P8", "F-C-boundary-P1", "F-C-boundary-P8"):
        run, m = mirrors(key)
        assert m.tiling.aligned == 1 and m.tiling.n_tiles >= 1024
        # (the series stays on: farfield_cases.call_tiling)
        assert fc.FAR_RATIO*0.5*m.tiling.length < run.case.cut_off*run.case.npv
        busiest = max(m.passes.values(), key=lambda p: p.pairs)
        assert busiest.adding >= 4, key
        assert sum(p.cut_by_tile for p in m.passes.values()) > 0
        # The far lines either side are the series' on the busiest tile.
        t = max(m.passes, key=lambda k: m.passes[k].pairs)[0]
        s = m.schedules[t]
        assert s.f1 > s.a1 and s.f2 < s.a2

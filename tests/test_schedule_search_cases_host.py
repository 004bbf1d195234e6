"""CPU-only checks of tests/schedule_search_cases.py, the inputs and the numpy mirror behind
tests/test_gpu_schedule_search.py: that the constants the mirror copies stand in the source, that
the base table and its variants are what the cases need, that the mirrored bracket of every key
contains the answer of a search of the whole table, that the mirrored schedule is
farfield_cases.schedule_tile field by field, that the keys reach every branch of search_bracket
(a census, printed), and what five mutants of the bracket and one of its margin do to the
schedules of the cases the GPU test runs."""
from pathlib import Path

import numpy as np
import pytest

from tests import farfield_cases as fc
from tests import schedule_search_cases as sc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pylbl_amd" / "csrc"
UP, DOWN = (lambda x: np.nextafter(x, np.inf)), (lambda x: np.nextafter(x, -np.inf))
CALLS = [(key, level, far) for key in sc.CASES for level in range(len(sc.FIVE_LEVELS))
         for far in (True, False)]
# The levels of the GPU test's two-level calls: what the mutants are run on.
TWO = [sc.FIVE_LEVELS.index(level) for level in sc.TWO_LEVELS]


@pytest.fixture(scope="module")
def keys():
    """(case key, level, farfield) -> [(s, eight keys)] of every tile: what every call of the GPU
    test searches for (its two levels are two of the five)."""
    base = sc.variants()["fine"][0]
    return {(key, level, far): sc.tile_keys(sc.CASES[key], base, sc.FIVE_LEVELS[level], far)
            for key, level, far in CALLS}


@pytest.fixture(scope="module")
def tile_key_values(keys):
    return np.unique([key for tiles in keys.values() for _, eight in tiles for key, _ in eight])


def sweep(name, tile_key_values):
    """The keys of the containment sweep of one variant: the keys of every tile, every cell edge
    within 200 cm-1 of the base table and every line position, each and one ulp either side, and
    keys far outside."""
    table, cells = sc.variants()[name]
    values = [tile_key_values, table.nu]
    if cells is not None:
        near = cells.edges[(cells.edges >= sc.FIRST - 200.) & (cells.edges <= sc.LAST + 200.)]
        values.append(near)
        top = cells.edges[-1]
        values.append(np.array([cells.base - 100., cells.base - 1.e7, top + 1.e7,
                                cells.base - 0.25, cells.base - 0.125, cells.base - 0.375,
                                top - 0.125, top, top + 0.125, top + 17.]))
    else:
        values.append(np.array([table.nu[0] - 100., table.nu[-1] + 1.e7]))
    values = np.concatenate(values)
    return np.unique(np.concatenate([values, UP(values), DOWN(values)]))


def test_constants_stand_in_the_source():
    engine = (CSRC / "engine.hip").read_text()
    assert "const double base = std::floor(sorted_nu.front());" in engine
    assert "const double span = std::ceil(sorted_nu.back()) - base + 1.;" in engine
    assert "if (span >= 1. && span < 1.e12)" in engine and sc.SPAN_LIMIT == 1.e12
    assert "const double scale = std::min(8., std::floor(1048576./span*8.)/8.);" in engine
    assert (sc.FINEST, sc.CELL_LIMIT) == (8., 1048576.)
    assert "if (scale > 0.)" in engine
    assert "const long long entries = (long long)(span*scale) + 1;" in engine
    assert "const double edge = base + (double)i/scale;" in engine
    assert "while (j < n_lines && sorted_nu[(size_t)j] < edge) ++j;" in engine
    schedule = (CSRC / "tile_schedule.h").read_text()
    assert "if (t.cell_first == nullptr || !(x == x)) return;" in schedule
    assert "const double at = floor((x - t.cell_base)*t.cell_scale);" in schedule
    assert "const int last = t.cell_entries - 1;" in schedule
    assert "if (at >= 1.) lo = t.cell_first[min((int)fmin(at, (double)last) - 1, last)];" in schedule
    assert "if (at + 2. <= (double)last) hi = t.cell_first[max((int)fmax(at, -2.) + 2, 0)];" in \
        schedule
    assert "if (nu[mid] < x) lo = mid + 1; else hi = mid;" in schedule
    assert "if (nu[mid] <= x) lo = mid + 1; else hi = mid;" in schedule
    assert "constexpr int kInlineLevels = %d;" % fc.INLINE_LEVELS in schedule
    assert len(sc.TWO_LEVELS) <= fc.INLINE_LEVELS < len(sc.FIVE_LEVELS)
    assert "v.cell_first = cell_entries > 0 ? d_cell_first.data : nullptr;" in \
        (CSRC / "engine_core.h").read_text()


def test_base_table_is_what_the_cases_need():
    table = sc.base_table()
    nu = table.nu
    assert 150 <= table.num_lines <= 400 and np.all(np.diff(nu) >= 0.)
    for column in ("sw", "gamma_air", "gamma_self", "n_air", "elower"):
        assert len(set(getattr(table, column))) == 1
    assert set(table.local_iso_id) == {1}
    shifted = table.delta_air != 0.
    assert 0.28 <= shifted.mean() <= 0.4, shifted.mean()
    assert np.max(np.abs(table.delta_air)) == 0.02
    # Lines on eighths, and one ulp either side of an eighth.
    eighths = nu[nu*8. == np.round(nu*8.)]
    assert eighths.size >= 20
    assert sum(1 for x in nu if UP(x)*8. == np.round(UP(x)*8.)) >= 10
    assert sum(1 for x in nu if DOWN(x)*8. == np.round(DOWN(x)*8.)) >= 10
    # The first and the last line on integers: base is a line position, ceil(back) == back.
    assert nu[0] == sc.FIRST == np.floor(nu[0]) and nu[-1] == sc.LAST == np.ceil(nu[-1])
    values, counts = np.unique(nu, return_counts=True)
    assert counts.max() == sc.DUPLICATES[1] >= 8 and values[counts.argmax()] == sc.DUPLICATES[0]
    cell = np.floor((nu - sc.FIRST)*8.).astype(int)
    assert np.bincount(cell).max() == sc.DENSE_CELL[1] > 64
    # Two gaps of 24 empty cells and more, inside window (a).
    for a, b in sc.GAPS:
        assert b - a >= 3. and not np.any((nu > a) & (nu < b))
        for key in ("a aligned 500", "a unaligned 512", "a aligned 63", "a coarse grid"):
            assert sc.CASES[key].v0 < a and b < sc.CASES[key].vn
    # Lines that cross an integer at some levels only.
    crossed = np.array([np.floor(nu + p*9.86923e-6*table.delta_air) != np.floor(nu)
                        for _, p in sc.FIVE_LEVELS])
    assert np.sum(crossed.any(axis=0) & ~crossed.all(axis=0)) >= 10


def test_variants_and_windows_are_the_ones_named():
    variants = sc.variants()            # (asserts the scales by value)
    base = variants["fine"][0]
    assert [variants[name][1].scale if variants[name][1] else None for name in sc.VARIANTS] == \
        [8., 7.875, 3.375, 0.125, None, 3.375]
    for name, (table, cells) in variants.items():
        at = sc.VARIANTS[name][0]
        extra = table.num_lines - base.num_lines
        assert extra == (0 if at is None else 1)
        where = 0 if name == "below" else table.num_lines - 1
        rest = np.arange(table.num_lines) != where if extra else slice(None)
        for column in ("nu", "sw", "gamma_air", "gamma_self", "n_air", "elower", "delta_air",
                       "local_iso_id"):
            assert np.array_equal(getattr(table, column)[rest], getattr(base, column))
            if extra and column != "nu":
                assert getattr(table, column)[where] == getattr(base, column)[0]
        # The level scalars do not move.
        for level in sc.FIVE_LEVELS:
            assert vars(fc.level_scalars(table, *level)) == vars(fc.level_scalars(base, *level))
        if cells is not None:
            assert cells.entries <= sc.CELL_LIMIT + 1 and cells.cell_first.nbytes <= 4 << 20
    assert variants["below"][1].base < 0.
    first_cell = (sc.FIRST - variants["below"][1].base)*variants["below"][1].scale
    assert 1.e6 <= first_cell <= 1.05e6
    span = lambda name: np.ceil(variants[name][0].nu[-1]) - np.floor(variants[name][0].nu[0]) + 1.
    assert 131072. < span("switch") < 131072. + 8. and span("fine") < 131072.
    assert 8388608. < span("none") and span("coarsest") <= 8388608.
    for key, case in sc.CASES.items():
        assert case.n <= 20000 and case.cut_off in (25, 3)
        low, high = case.v0 - (case.cut_off + 1), case.vn + case.cut_off + 1
        accepted = sc.in_range(base, case).num_lines
        if key[0] == "a":
            assert sc.FIRST < case.v0 and case.vn < sc.LAST and accepted > 100
        if key[0] == "b":
            assert case.v0 < sc.FIRST - (case.cut_off + 2) and 10 < accepted < base.num_lines
        if key[0] == "c":
            assert case.vn > sc.LAST + case.cut_off + 2 and 10 < accepted < base.num_lines
        if key[0] == "d":
            assert high < sc.FIRST and accepted == 0
        if key[0] == "e":
            assert low > sc.LAST and accepted == 0
        for name in sc.VARIANTS:
            at = sc.VARIANTS[name][0]
            assert at is None or not low - 1000. <= at <= high + 1000.
    tilings = {key: sc.call_tiling(case) for key, case in sc.CASES.items()}
    assert (tilings["a aligned 500"][0].aligned, tilings["a aligned 500"][0].length) == (1, 500)
    assert (tilings["a unaligned 512"][0].aligned, tilings["a unaligned 512"][0].length) == (0, 512)
    assert (tilings["a aligned 63"][0].aligned, tilings["a aligned 63"][0].length) == (1, 63)
    assert {sc.CASES[key].points for key in sc.CASES if key[0] == "a"} >= {1, 8}
    assert 1 in {far for _, far in tilings.values()}


def test_cell_table_is_the_builders_loop():
    """The loop of lbl_molecule_load itself, on the finest table and on the one with a negative
    base and a fractional scale."""
    for name in ("fine", "below"):
        table, cells = sc.variants()[name]
        nu = table.nu.tolist()
        n, j, first = len(nu), 0, []
        base, scale = cells.base, cells.scale
        for i in range(cells.entries):
            edge = base + float(i)/scale
            while j < n and nu[j] < edge:
                j += 1
            first.append(j)
        assert np.array_equal(np.array(first), cells.cell_first), name
        assert cells.cell_first[-1] == n
    assert sc.cell_table(np.array([])) is None
    assert sc.cell_table(np.array([1., 1.e12])) is None
    assert sc.cell_table(np.array([1., 8388608.5])) is None
    assert sc.cell_table(np.array([1.5, 8388607.5])).scale == 0.125


def test_every_bracket_contains_the_answer(tile_key_values):
    for name, (table, cells) in sc.variants().items():
        nu, n = table.nu, table.num_lines
        values = sweep(name, tile_key_values)
        left = np.searchsorted(nu, values, "left")
        right = np.searchsorted(nu, values, "right")
        for x, l, r in zip(values.tolist(), left.tolist(), right.tolist()):
            lo, hi = sc.search_bracket(cells, n, x)
            assert 0 <= lo <= l <= r <= hi <= n, (name, x, lo, l, r, hi)
            assert sc.first_not_below(nu, lo, hi, x)[0] == l
            assert sc.first_above(nu, lo, hi, x)[0] == r
        assert sc.search_bracket(cells, n, float("nan")) == (0, n)
        print("%-9s %6d keys" % (name, values.size))


def test_the_mirrored_schedule_is_the_plain_one(keys):
    """scheduled(bracket=True) against farfield_cases.schedule_tile, field by field, for every
    tile, level, case and variant, with and without the series."""
    tiles = 0
    for name, (table, cells) in sc.variants().items():
        for key, level, far in CALLS:
            case = sc.CASES[key]
            mine = sc.scheduled(case, table, sc.FIVE_LEVELS[level], True, far, cells=cells,
                                keys=keys[key, level, far])
            plain = sc.scheduled(case, table, sc.FIVE_LEVELS[level], False, far)
            assert len(mine) == len(plain) > 0
            for t, (a, b) in enumerate(zip(mine, plain)):
                assert vars(a) == vars(b), (name, key, level, far, t)
            tiles += len(mine)
    print("(variant, call, tile) schedules compared: %d" % tiles)


CENSUS = ("at < -2", "-2 <= at < 1", "at in the table", "at + 2 > last", "at > last", "lo == hi",
          "bracket wider than 64 lines", "key on a cell edge", "key on a line position")


def census_of(name, values):
    table, cells = sc.variants()[name]
    count = dict.fromkeys(CENSUS, 0)
    if cells is None:
        return count
    last = cells.entries - 1
    edges, lines = set(cells.edges.tolist()), set(table.nu.tolist())
    for x in values.tolist():
        at = sc.cell_of(cells, x)
        lo, hi = sc.search_bracket(cells, table.num_lines, x)
        count["at < -2"] += at < -2.
        count["-2 <= at < 1"] += -2. <= at < 1.
        count["at in the table"] += 1. <= at and at + 2. <= last
        count["at + 2 > last"] += at + 2. > last
        count["at > last"] += at > last
        count["lo == hi"] += lo == hi
        count["bracket wider than 64 lines"] += hi - lo > 64
        count["key on a cell edge"] += x in edges
        count["key on a line position"] += x in lines
    return count


def test_the_keys_reach_every_branch(tile_key_values):
    """The census of the containment sweep per variant, and of the keys of the tiles alone (what
    the GPU runs): no entry of the sweep's total is zero; the keys of the tiles reach every branch
    of search_bracket, empty brackets and wide ones (they lie on no cell edge or line: integers
    -+ shift_max and the like)."""
    total, tiles = dict.fromkeys(CENSUS, 0), dict.fromkeys(CENSUS, 0)
    print("%-28s %s" % ("keys with", "  ".join("%9s" % name for name in sc.VARIANTS)))
    rows = {name: census_of(name, sweep(name, tile_key_values)) for name in sc.VARIANTS}
    mine = {name: census_of(name, tile_key_values) for name in sc.VARIANTS}
    for entry in CENSUS:
        print("%-28s %s" % (entry, "  ".join("%5d/%-5d" % (mine[name][entry], rows[name][entry])
                                             for name in sc.VARIANTS)))
        total[entry] = sum(rows[name][entry] for name in sc.VARIANTS)
        tiles[entry] = sum(mine[name][entry] for name in sc.VARIANTS)
    print("(keys of the tiles / keys of the sweep; %d keys of tiles)" % tile_key_values.size)
    print("total of the sweep: %s" % total)
    print("total of the tiles: %s" % tiles)
    assert all(total[entry] > 0 for entry in CENSUS), total
    assert all(tiles[entry] > 0 for entry in CENSUS[:7]), tiles
    # In the finest variant the windows below the table reach at < -2, the ones above at > last.
    assert mine["fine"]["at < -2"] > 0 and mine["fine"]["at > last"] > 0
    # With the inert line below, every key lies far up the cell table, or beyond its end.
    assert mine["below"]["at < -2"] == 0 and mine["below"]["at > last"] > 0


def seen_lines(case, table, level, s):
    """Mask of the lines the skip policy accepts whose window (spectra.c:48-62: b = floor(nu +
    p delta), [b - cut, b + cut + 1] both ends included) holds a point of the tile."""
    p_atm = sc.FIVE_LEVELS[level][1]*9.86923e-6
    b = np.floor(table.nu + p_atm*table.delta_air)
    first = (b - case.cut_off - case.v0)*case.npv
    last = (b + case.cut_off + 1 - case.v0)*case.npv
    accepted = (table.nu >= case.v0 - (case.cut_off + 1)) & (table.nu <= case.vn + case.cut_off + 1)
    return accepted & (first <= s.i1) & (last >= s.i0)


_RIGHT = {}      # (variant, case key, level, farfield) -> the mirrored schedule, made once


def mutant_effects(mutation, keys, stop_at_first=False):
    """(changed schedules, [(variant, case, level, farfield, tile, dropped lines)]) of a mutant
    over every two-level call of the GPU test: a witness is a tile from whose [lo, hi) the mutant drops a
    line that the tile's spectrum sees.  (A line cannot be doubled: the clamps keep lo <= a1 <=
    ... <= hi whatever the searches return.)"""
    changed, witnesses = 0, []
    for name, (table, cells) in sc.variants().items():
        mutated = sc.cell_table(table.nu, mutation)
        for key, level, far in CALLS:
            if level not in TWO:
                continue
            case = sc.CASES[key]
            if (name, key, level, far) not in _RIGHT:
                _RIGHT[name, key, level, far] = sc.scheduled(
                    case, table, sc.FIVE_LEVELS[level], True, far, cells=cells,
                    keys=keys[key, level, far])
            right = _RIGHT[name, key, level, far]
            wrong = sc.scheduled(case, table, sc.FIVE_LEVELS[level], True, far, mutation,
                                 cells=mutated, keys=keys[key, level, far])
            for t, (a, b) in enumerate(zip(right, wrong)):
                if vars(a) == vars(b):
                    continue
                changed += 1
                index = np.arange(table.num_lines)
                dropped = (index >= a.lo) & (index < a.hi) & ~((index >= b.lo) & (index < b.hi))
                dropped &= seen_lines(case, table, level, a)
                if dropped.any():
                    witnesses.append((name, key, level, far, t, np.flatnonzero(dropped).tolist()))
                    if stop_at_first:
                        return changed, witnesses
    return changed, witnesses


@pytest.mark.parametrize("mutation", [sc.MUTATIONS[0], sc.MUTATIONS[1], sc.MUTATIONS[3]])
def test_mutants_drop_lines_the_spectrum_sees(keys, mutation):
    """A bracket one cell towards the key at either end, and the finest scale in the search of a
    coarse table: each changes the mirrored schedule of tiles the GPU test runs, and at some of
    them [lo, hi) loses a line whose window holds a point of the tile."""
    changed, witnesses = mutant_effects(mutation, keys)
    print("%-24s %5d schedules changed, %4d tiles lose a line they see; first: %s" % (
        mutation, changed, len(witnesses), witnesses[:1]))
    by_variant = sorted({w[0] for w in witnesses})
    print("%-24s in variants %s, cases %s" % (mutation, by_variant, sorted({w[1] for w in witnesses})))
    assert witnesses
    if mutation == "scale 8 in the search":
        assert "fine" not in by_variant and set(by_variant) >= {"coarse", "coarsest", "below"}
    else:
        assert "fine" in by_variant


@pytest.mark.parametrize("mutation", [sc.MUTATIONS[2], sc.MUTATIONS[4]])
def test_two_mutants_change_brackets_and_no_schedule(keys, tile_key_values, mutation):
    """A cell table built with <= and a lo index that is not clamped to `last` change brackets and
    can change no schedule, here or on any table:
      * with <=, cell_first[i] is the first line ABOVE edge i instead of the first not below it.
        lo is read one cell below the key's (edge at-1 < key, so every line on that edge is below
        the key and in front of the answer either way) and hi two above it (a later index
        contains as much); where a rounded `at` is one cell off the margin still holds by a
        cell.  The mutant is wrong only together with a missing margin (the last assertion).
      * the clamp acts on keys with at > last, which lie above the last edge and so above every
        line: the answer is n_lines, which is what the read behind the table is modelled as.
        In the kernel that read is out of bounds, which no test of values can stand for.
    So the mirror shows the brackets moving and every schedule unchanged: neither mutant is one
    the GPU test can catch, and none of the checks there rests on them."""
    moved = 0
    for name, (table, cells) in sc.variants().items():
        if cells is None:
            continue
        mutated = sc.cell_table(table.nu, mutation)
        for x in sweep(name, tile_key_values).tolist():
            a = sc.search_bracket(cells, table.num_lines, x)
            b = sc.search_bracket(mutated, table.num_lines, x, mutation)
            moved += a != b
            l, r = np.searchsorted(table.nu, x, "left"), np.searchsorted(table.nu, x, "right")
            assert b[0] <= l <= r <= b[1], (mutation, name, x)
    changed, witnesses = mutant_effects(mutation, keys)
    print("%-30s %5d brackets of the sweep moved, %d schedules changed" % (mutation, moved, changed))
    assert moved > 0 and changed == 0 and not witnesses
    if mutation == "cell table built with <=":
        # Without the margin the same table does drop lines: a key on an edge that holds a line.
        table, _ = sc.variants()["fine"]
        mutated = sc.cell_table(table.nu, mutation)
        x = sc.DUPLICATES[0]
        lo = int(mutated.cell_first[int(sc.cell_of(mutated, x))])
        assert lo == np.searchsorted(table.nu, x, "right") > np.searchsorted(table.nu, x, "left")


def test_the_margin_below_is_for_rounding_alone(keys, tile_key_values):
    """lo from cell `at` itself (no margin) is right wherever `at` is the cell the key lies in:
    edge at <= key.  Measured here, per variant, over the sweep and over the keys of the tiles:
    how many keys search_bracket puts in the cell above their own (edge at > key: what the margin
    below is for), how many in the cell below (edge at+1 <= key: why hi is read two cells up and
    not one), and how many searches come out wrong without the margin below.
      * Scale 8 and 0.125 (powers of two): the product is exact, no key is misplaced.
      * 7.875 and 3.375 with the base at 990: several hundred keys of the sweep, all within an
        ulp of an edge, land in the cell below their own; none above.
      * 3.375 with the base at -300001: keys within an ulp of an edge land on either side.
      * No key of the tiles lies within an ulp of an edge: none is misplaced in any variant.
    So no key of the sweep NEEDS the margin below -- between a misplaced key and its edge lies
    no line of these tables -- and without it no schedule of the GPU cases changes: the GPU test
    cannot tell that mutant from the kernel, and the margin stands for keys these cases do not
    hold."""
    above, below, wrong = {}, {}, {}
    for name, (table, cells) in sc.variants().items():
        if cells is None:
            continue
        last = cells.entries - 1
        edges = cells.edges
        for label, values in (("sweep", sweep(name, tile_key_values)), ("tiles", tile_key_values)):
            up = down = bad = 0
            for x in values.tolist():
                at = int(sc.cell_of(cells, x))
                up += 0 <= at <= last and edges[at] > x
                down += 0 <= at + 1 <= last and edges[at + 1] <= x
                lo, _ = sc.search_bracket(cells, table.num_lines, x, sc.NO_MARGIN)
                bad += lo > np.searchsorted(table.nu, x, "left")
            above[name, label], below[name, label], wrong[name, label] = int(up), int(down), int(bad)
    print("keys put in the cell above their own: %s" % above)
    print("keys put in the cell below their own: %s" % below)
    print("searches that go wrong without the margin below: %s" % wrong)
    changed, _ = mutant_effects(sc.NO_MARGIN, keys)
    print("no margin below: %d schedules of the GPU cases changed" % changed)
    for name in ("fine", "coarsest"):
        assert above[name, "sweep"] == below[name, "sweep"] == 0
    for name in ("switch", "coarse"):
        assert above[name, "sweep"] == 0 and below[name, "sweep"] > 100
    assert above["below", "sweep"] > 100 and below["below", "sweep"] > 100
    assert not any(above[name, "tiles"] or below[name, "tiles"] for name, _ in above)
    assert not any(wrong.values()) and changed == 0

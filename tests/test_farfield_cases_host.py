"""CPU-only checks of tests/farfield_cases.py, the inputs and the numpy mirror behind
tests/test_gpu_farfield_lines.py: that the tilings are the ones the cases are named for, that the
mirrored partition counts every (line, tile) once and agrees with the window rule of the oracle
(and that three mutants of it do not), that truncation(rho) bounds the 21-term series, the
float64-vs-long-double scan of the series mirror that measures E_cpu (printed; farfield_cases.E_CPU
records it and the GPU tests take their bound from it), that the cases reach every class and branch
they are meant to, and that every line of the table cases weighs at least 1000 tolerances on every
tile whose series takes it."""
from pathlib import Path

import numpy as np
import pytest

from tests import farfield_cases as fc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pylbl_amd" / "csrc"
F64, LD = np.float64, np.longdouble


def derived_of(oracle, case, table, temperature, pressure):
    _, extras = oracle.absorption_port(table, temperature, pressure, fc.X, case.v0, case.vn,
                                       case.npv, cut_off=case.cut_off, want_derived=True)
    return extras["derived"]


@pytest.fixture(scope="module")
def one_line_runs(oracle):
    """[(case key, label, what, index, where, level, partition, derived)] of every one-line
    table of the GPU test."""
    runs = []
    for key in fc.ONE_LINE_CASES:
        case = fc.CASES[key]
        for temperature, pressure in fc.ONE_LINE_LEVELS:
            lv = fc.level_scalars(fc.make_table([case.v0 + 0.5], v0=case.v0), temperature, pressure)
            for label, at, what, index, where in fc.handover_positions(case, lv):
                table = fc.make_table([at], v0=case.v0)
                part = fc.partition(case, table, temperature, pressure)
                derived = derived_of(oracle, case, table, temperature, pressure)
                runs.append((key, label, what, index, where, (temperature, pressure), part,
                             derived))
    return runs


@pytest.fixture(scope="module")
def table_runs(oracle):
    """[(name, case, table, level, partition, derived)]: the table cases at five levels, and
    cases A and B at the small cut-offs."""
    runs = []
    cases = [(key, fc.CASES[key]) for key in fc.TABLE_CASES]
    cases += [("%s cut_off %d" % (key, cut), fc.with_cut_off(fc.CASES[key], cut))
              for key in ("A", "B") for cut in fc.CUT_OFFS]
    for name, case in cases:
        table = fc.table_for(case)
        for level in fc.FIVE_LEVELS:
            runs.append((name, case, table, level, fc.partition(case, table, *level),
                         derived_of(oracle, case, table, *level)))
    return runs


def test_constants_and_tilings_are_the_ones_named():
    accumulate = (CSRC / "accumulate.h").read_text()
    assert "#define LBL_FAR_TERMS %d\n" % fc.FAR_TERMS in accumulate
    assert "#define LBL_FAR_RATIO %d.\n" % fc.FAR_RATIO in accumulate
    assert "constexpr int kFarGroup = %d;" % fc.FAR_GROUP in (CSRC / "farfield.h").read_text()
    assert "constexpr int kInlineLevels = %d;" % fc.INLINE_LEVELS in \
        (CSRC / "tile_schedule.h").read_text()
    assert len(fc.FIVE_LEVELS) > fc.INLINE_LEVELS
    for case in fc.CASES.values():
        tiling, farfield = fc.call_tiling(case)
        got = dict(aligned=tiling.aligned, length=tiling.length, n_tiles=tiling.n_tiles,
                   n_groups=fc.n_groups_of(tiling), p=tiling.p)
        assert farfield == 1 and got == case.expect, (case.name, got)
        assert case.n <= 20000
    # The last tiles: clipped by the grid (D, E), short at the end of a cell (A, C).
    d, e = fc.CASES["D"], fc.CASES["E"]
    i0, i1 = fc.tile_bounds(fc.call_tiling(d)[0], 9, d.npv, d.n)
    assert i1 - i0 + 1 == 292
    i0, i1 = fc.tile_bounds(fc.call_tiling(e)[0], 31, e.npv, e.n)
    assert i1 - i0 + 1 == 32
    c = fc.CASES["C"]
    lengths = [np.diff(fc.tile_bounds(fc.call_tiling(c)[0], t, c.npv, c.n))[0] + 1
               for t in range(16)]
    assert lengths == [63]*15 + [55]
    # cut_off = 1 switches the series off and the tiling back; 2 and wider keep it.
    for key in ("A", "B"):
        tiling, farfield = fc.call_tiling(fc.with_cut_off(fc.CASES[key], 1))
        assert (farfield, tiling.aligned, tiling.length) == (0, 0, 512)
        assert all(fc.call_tiling(fc.with_cut_off(fc.CASES[key], cut))[1] == 1
                   for cut in fc.CUT_OFFS[1:])


def test_tables_are_what_the_gpu_tests_need():
    for key in fc.TABLE_CASES:
        case = fc.CASES[key]
        table = fc.table_for(case)
        assert 60 <= table.num_lines <= 120, (key, table.num_lines)
        assert np.min(np.diff(table.nu)) >= 0.02
        assert table.nu[0] >= case.v0 - case.cut_off - 1 and table.nu[-1] <= case.vn + case.cut_off + 1
        shifted = table.delta_air != 0.
        assert 0.25 <= shifted.mean() <= 0.4, (key, shifted.mean())
        assert np.max(np.abs(table.delta_air)) == 0.02
        assert np.all(np.abs(table.nu[shifted] - np.round(table.nu[shifted])) <= 0.002)
        assert np.all(table.nu != np.round(table.nu))
        assert len(set(table.sw)) == 1 and len(set(table.gamma_air)) == 1


def test_partition_counts_every_pair_once_and_keeps_the_window_rule(one_line_runs, table_runs):
    checked = 0
    for key, label, _, _, _, level, part, derived in one_line_runs:
        problems = fc.partition_problems(part, derived)
        assert not problems, (key, label, level, problems[:3])
        checked += part.count.size
    for name, case, table, level, part, derived in table_runs:
        problems = fc.partition_problems(part, derived)
        assert not problems, (name, level, problems[:3])
        checked += part.count.size
    print("(line, tile, level) triples checked: %d" % checked)


def test_handover_lines_fall_where_they_are_placed(one_line_runs):
    """Beyond a tile's limit the tile's own series has the line, beyond a group's the group's on
    every tile of the group; the same step inside, the direct kernel (a tile) or the tiles' own
    series (a group)."""
    for key, label, what, index, where, level, part, derived in one_line_runs:
        # (Where core + half sets both radii, the limits of a group and of its outer tiles lie
        # within a few 1e-5 cm-1 of each other -- both are the edge minus the core -- and the
        # neighbouring class may have the line.)
        if what == "tile":
            expect = {fc.TILE_NEAR} if where == "beyond" else {fc.DIRECT}
            got = {int(part.classes[index, 0])}
            if part.tiles[index].side == "core" and where == "beyond":
                got -= {fc.GROUP}
                expect = set() if not got else expect
        elif what == "group":
            g = part.groups[index]
            expect = {fc.GROUP} if where == "beyond" else {fc.TILE_NEAR}
            got = {int(x) for x in part.classes[g.t0:g.t1, 0]}
            if g.side == "core" and where == "inside":
                got -= {fc.DIRECT}
        else:
            continue
        assert got == expect, (key, label, level, [fc.CLASS_NAMES[x] for x in got])
        if where == "beyond" and what == "tile" and part.tiles[index].side == "ratio":
            assert 0.2499 <= fc.pair_ratio(part, derived, index, 0) <= 0.25
        if where == "beyond" and what == "group" and part.groups[index].side == "ratio":
            assert 0.2499 <= fc.group_ratio(part, derived, index, 0) <= 0.25


def test_mutants_of_the_partition_are_caught(table_runs):
    """Moving g1 by one line, swapping l1 and l2, ignoring shift_max: each is found by the
    checks above in at least one table case (and the first two in case A itself)."""
    for mutation in fc.MUTATIONS:
        caught = []
        for name, case, table, level, _, derived in table_runs:
            if name not in fc.TABLE_CASES:
                continue
            mutant = fc.partition(case, table, *level, mutation=mutation)
            if fc.partition_problems(mutant, derived):
                caught.append(name)
        print("%-20s caught in %s" % (mutation, sorted(set(caught))))
        assert "A" in caught, (mutation, caught)


def series_error(gamma, a, u):
    """|21-term series - exact|/exact of 1/((a - u)^2 + gamma^2) about u = 0, in long double."""
    a, gamma, u = LD(a), LD(gamma), np.asarray(u, LD)
    q = fc._line_terms(LD, [a], [gamma*gamma], [1.], 0.)[0]
    value = np.full(u.shape, q[-1], LD)
    for k in range(fc.FAR_TERMS - 2, -1, -1):
        value = value*u + q[k]
    exact = LD(1)/((a - u)*(a - u) + gamma*gamma)
    return np.abs(value - exact)/exact


def test_truncation_bounds_the_series_and_is_attained():
    assert abs(fc.truncation(0.25)/6.2e-12 - 1.) < 0.01
    assert abs(0.25**21*(22 - 21*0.25)/3.8e-12 - 1.) < 0.01
    for rho in (0.25, 0.2, 0.1):
        for a in (1., -1., 0.17, 4.):
            u = np.linspace(-rho*abs(a), rho*abs(a), 2001)
            for gamma in (1.e-6, 1.e-4, 1.e-2, 0.07, 0.3, 1., 3.):
                error = series_error(gamma, a, u)
                # (long double carries 64 bits: 1e-18 of rounding on either side)
                assert np.max(error) <= fc.truncation(rho)*(1. + 1.e-6) + 1.e-17, (rho, a, gamma)
            worst = np.max(series_error(1.e-6, a, u))
            if fc.truncation(rho) > 1.e-15:
                assert 0.99 <= worst/fc.truncation(rho) <= 1. + 1.e-6, (rho, a, worst)
    print("truncation(1/4) = %.4g, near side %.4g" % (fc.truncation(0.25),
                                                      0.25**21*(22 - 21*0.25)))


def test_rounding_allowance_of_the_series(one_line_runs):
    """E_cpu: the worst |float64 mirror - long-double mirror|/value over every series tile of the
    one-line cases, printed; and the float64 mirror within truncation(rho) + E_cpu + 1e-15 of the
    exact Lorentz term there, which a mirror without the last term of the Taylor shift is not."""
    worst, closest, pairs = 0., 0., 0
    dropped = 0.
    per_case = {}
    for key, label, what, index, where, level, part, derived in one_line_runs:
        for t in range(part.tiling.n_tiles):
            kind = part.classes[t, 0]
            if kind not in fc.SERIES_CLASSES or derived[0, 6] != 1.:
                continue
            s = part.tiles[t]
            double = fc.series_values(F64, part, fc.series_coefficients(F64, part, derived, t), t)
            longer = fc.series_values(LD, part, fc.series_coefficients(LD, part, derived, t), t)
            error = float(np.max(np.abs(double - longer)/np.abs(longer)))
            worst = max(worst, error)
            exact = fc.lorentz(part.case, derived, 0, s.i0, s.i1)
            bound = fc.truncation(fc.pair_ratio(part, derived, t, 0)) + fc.E_CPU + 1.e-15
            ratio = float(np.max(np.abs(double - exact)/exact))/bound
            closest = max(closest, ratio)
            per_case[key] = max(per_case.get(key, 0.), ratio)
            pairs += 1
            if kind == fc.GROUP and t % fc.FAR_GROUP in (0, 3):
                short = fc.series_values(F64, part, fc.series_coefficients(
                    F64, part, derived, t, drop_last_taylor=True), t)
                dropped = max(dropped, float(np.max(np.abs(short - exact)/exact))/bound)
    print("series pairs of the one-line cases: %d" % pairs)
    print("E_cpu = %.3g" % worst)
    print("float64 mirror against the exact term, worst/bound per case: %s" % {
        k: "%.3f" % v for k, v in per_case.items()})
    print("without the last Taylor term: %.3g x the bound" % dropped)
    assert pairs > 500
    assert worst <= fc.E_CPU <= 2.*worst, "farfield_cases.E_CPU no longer records the measured value"
    assert fc.truncation(0.25) + 4.*fc.E_CPU <= 1.e-11
    assert closest <= 1.
    # The lines sit where the truncation peaks: the ratio-governed cases come close to the bound.
    assert per_case["A"] >= 0.5 and per_case["D"] >= 0.5
    assert dropped > 1.


def test_cases_reach_every_class_and_branch(one_line_runs, table_runs):
    classes = np.zeros(6, dtype=np.int64)
    tile_sides, group_sides, group_counts = set(), set(), set()
    partial_group = clipped_last = short_last = False
    crossing_some_levels = 0
    small = {}
    runs = [(key, part, derived) for key, _, _, _, _, _, part, derived in one_line_runs]
    runs += [(name, part, derived) for name, _, _, _, part, derived in table_runs]
    for name, part, derived in runs:
        live = (derived[:, 6] == 1.) & (derived[:, 5] >= derived[:, 4])
        classes += np.bincount(part.classes[:, live].ravel(), minlength=6)
        if not part.farfield:
            continue
        tile_sides |= {s.side for s in part.tiles}
        group_sides |= {g.side for g in part.groups}
        group_counts.add(len(part.groups))
        partial_group |= part.groups[-1].t1 - part.groups[-1].t0 < fc.FAR_GROUP
        last = part.tiles[-1]
        if last.i1 - last.i0 + 1 < part.tiling.length:
            if part.tiling.aligned:
                short_last = True
            else:
                clipped_last = True
        if "cut_off" in name:
            # (Apart: the groups of four tiles, and the last group of A and of B, which is one
            # cell wide -- lines two cells away cover it even at cut_off = 2.)
            full = fc.FAR_GROUP*(part.tiling.n_tiles//fc.FAR_GROUP)
            small.setdefault(name, [0, 0])
            small[name][0] += int(np.sum(part.classes[:full, live] == fc.GROUP))
            small[name][1] += int(np.sum(part.classes[full:, live] == fc.GROUP))
    for key in fc.TABLE_CASES:
        table = fc.table_for(fc.CASES[key])
        crossed = np.array([np.floor(table.nu + p*9.86923e-6*table.delta_air) != np.floor(table.nu)
                            for _, p in fc.FIVE_LEVELS])
        crossing_some_levels += int(np.sum(crossed.any(axis=0) & ~crossed.all(axis=0)))
    print("class coverage over every case and level:")
    for name, n in zip(fc.CLASS_NAMES, classes):
        print("  %-12s %8d" % (name, n))
    print("radius set by: tiles %s, groups %s; group counts %s" % (
        sorted(tile_sides), sorted(group_sides), sorted(group_counts)))
    print("lines that cross an integer at some levels only: %d" % crossing_some_levels)
    print("group-series pairs at small cut-offs [full groups, partial last group]: %s" % small)
    assert np.all(classes > 0), dict(zip(fc.CLASS_NAMES, classes))
    assert tile_sides == {"core", "ratio"} and group_sides == {"core", "ratio"}
    assert partial_group and clipped_last and short_last
    assert min(group_counts) < 8 and 8 in group_counts and max(group_counts) > 8
    assert any(n % 8 for n in group_counts if n > 8)
    assert crossing_some_levels >= 1
    for key in ("A", "B"):
        for cut in (2, 3):
            assert small["%s cut_off %d" % (key, cut)][0] == 0
            assert small["%s cut_off %d" % (key, cut)][1] > 0
        for cut in (5, 6):
            assert small["%s cut_off %d" % (key, cut)][0] > 0
    # Case C's tiles and case H's tiles and groups take core + half; A's take the ratio.
    by_case = {}
    for key, _, _, _, _, _, part, _ in one_line_runs:
        by_case.setdefault(key, (set(), set()))
        by_case[key][0].update(s.side for s in part.tiles)
        by_case[key][1].update(g.side for g in part.groups)
    assert by_case["A"] == ({"ratio"}, {"ratio"})
    assert by_case["C"] == ({"core"}, {"ratio"})
    assert by_case["H"] == ({"core"}, {"core"})


def test_every_line_weighs_a_thousand_tolerances_where_a_series_takes_it(oracle, table_runs):
    """From the oracle alone: the spectrum of every line by itself over the spectrum of the table,
    at its largest over the points of every tile whose series takes the line."""
    smallest = np.inf
    for name, case, table, level, part, derived in table_runs:
        if not part.farfield:
            continue
        total, _ = oracle.absorption_port(table, *level, fc.X, case.v0, case.vn, case.npv,
                                          cut_off=case.cut_off)
        series = np.isin(part.classes, fc.SERIES_CLASSES)
        for j in np.flatnonzero(series.any(axis=0)):
            alone, _ = oracle.absorption_port(table.subset(np.arange(table.num_lines) == j),
                                              *level, fc.X, case.v0, case.vn, case.npv,
                                              cut_off=case.cut_off)
            with np.errstate(divide="ignore", invalid="ignore"):
                share = np.where(total > 0., alone/total, 0.)
            for t in np.flatnonzero(series[:, j]):
                s = part.tiles[t]
                smallest = min(smallest, float(np.max(share[s.i0:s.i1 + 1])))
    print("smallest line share on a series tile: %.3g = %.3g table tolerances" % (
        smallest, smallest/fc.TABLE_TOLERANCE))
    assert smallest >= 1000.*fc.TABLE_TOLERANCE

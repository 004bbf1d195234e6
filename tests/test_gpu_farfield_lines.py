"""The far-field series (csrc/farfield.h, the cuts of csrc/tile_schedule.h, the Horner evaluation
of csrc/accumulate.h) line by line: one line at every hand-over distance, tables in which every
line weighs on every tile that sums it, small cut-offs, and the levels of a call beyond
kInlineLevels.  Inputs, the partition mirror that names the class of every (line, tile, level) and
the series mirror are tests/farfield_cases.py; tests/test_farfield_cases_host.py checks them on
the CPU.

Bounds, none taken from the code under test.
  * On a tile whose only line is summed by a series the output is that series: within
    truncation(rho) + 4*E_cpu + 1e-15 relative of the exact Lorentz term S gamma/pi /
    ((v - c)^2 + gamma^2), in long double from the oracle's centre, gamma and strength.
    truncation(rho) = rho^21 (22 + 21 rho) is the remainder of the 21 terms at the far edge of the
    tile, rho = max |u|/|a| <= 1/4 the mirror's ratio of the pair (6.2e-12 at 1/4); E_cpu = 1.02e-15
    is the worst |float64 - long double|/value of the series mirror over these very cases
    (test_rounding_allowance_of_the_series prints it, farfield_cases.E_CPU records it), 4 the
    project's margin for device against host rounding.
  * On every other tile, and on whole tables without the series: ROUNDING = 1e-12 relative of the
    CPU oracle (tests/test_gpu_core_quotient.py).
  * Tables with the series: truncation(1/4) + ROUNDING relative of the oracle at every point (all
    terms are positive); with the pedestal removed, assert_spectrum of tests/test_gpu_parity.py.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import farfield_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def levels_of(levels):
    t = np.array([l[0] for l in levels])
    p = np.array([l[1] for l in levels])
    return t, p, np.full(len(levels), fc.X)


def run(engine, case, table, levels, farfield=1, remove_pedestal=False):
    """[levels, n] of one call with the case's points per lane; the options are put back."""
    t, p, x = levels_of(levels)
    engine.set_option("points_per_lane", case.points)
    engine.set_option("farfield", farfield)
    try:
        molecule = engine.load(table)
        try:
            return engine.compute(molecule, t, p, x, case.v0, case.vn, case.npv,
                                  cut_off=case.cut_off, remove_pedestal=remove_pedestal).copy()
        finally:
            engine.free(molecule)
    finally:
        engine.set_option("points_per_lane", 0)
        engine.set_option("farfield", 0)


def reference(oracle, case, table, levels, remove_pedestal=False):
    out = np.array([oracle.absorption_port(table, t, p, fc.X, case.v0, case.vn, case.npv,
                                           cut_off=case.cut_off,
                                           remove_pedestal=remove_pedestal)[0]
                    for t, p in levels])
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def tables(oracle):
    """case key -> (case, table, oracle spectra of FIVE_LEVELS): made once, never written to."""
    out = {}
    for key in fc.TABLE_CASES:
        case = fc.CASES[key]
        table = fc.table_for(case)
        out[key] = (case, table, reference(oracle, case, table, fc.FIVE_LEVELS))
    return out


def worst_relative(k, k_ref):
    nz = k_ref != 0
    assert np.array_equal(k[~nz], k_ref[~nz]), "non-zero where the reference is zero"
    return float(np.max(np.abs(k[nz] - k_ref[nz])/np.abs(k_ref[nz]))) if nz.any() else 0.


@pytest.mark.parametrize("key", fc.ONE_LINE_CASES)
def test_one_line_at_the_hand_over(engine, oracle, key):
    case = fc.CASES[key]
    worst_series, worst_direct, pairs = 0., 0., 0
    for temperature, pressure in fc.ONE_LINE_LEVELS:
        lv = fc.level_scalars(fc.make_table([case.v0 + 0.5], v0=case.v0), temperature, pressure)
        for label, at, what, index, where in fc.handover_positions(case, lv):
            table = fc.make_table([at], v0=case.v0)
            k_ref, extras = oracle.absorption_port(table, temperature, pressure, fc.X, case.v0,
                                                   case.vn, case.npv, cut_off=case.cut_off,
                                                   want_derived=True)
            derived = extras["derived"]
            part = fc.partition(case, table, temperature, pressure)
            k = run(engine, case, table, [(temperature, pressure)])[0]
            live = derived[0, 6] == 1. and derived[0, 5] >= derived[0, 4]
            name = "%s, %s, %g Pa" % (key, label, pressure)
            for t, s in enumerate(part.tiles):
                got, expect = k[s.i0:s.i1 + 1], k_ref[s.i0:s.i1 + 1]
                kind = part.classes[t, 0]
                if not live or kind == fc.OUTSIDE:
                    assert not np.any(expect) and not np.any(got), (name, t)
                elif kind in fc.SERIES_CLASSES:
                    exact = fc.lorentz(case, derived, 0, s.i0, s.i1)
                    error = float(np.max(np.abs(got - exact)/exact))
                    bound = fc.truncation(fc.pair_ratio(part, derived, t, 0)) + 4.*fc.E_CPU + 1.e-15
                    worst_series = max(worst_series, error/bound)
                    pairs += 1
                    assert error <= bound, "%s, tile %d (%s): %.4g against %.4g" % (
                        name, t, fc.CLASS_NAMES[kind], error, bound)
                else:
                    error = worst_relative(got, expect)
                    worst_direct = max(worst_direct, error/fc.ROUNDING)
                    assert error <= fc.ROUNDING, "%s, tile %d (%s): %.4g" % (
                        name, t, fc.CLASS_NAMES[kind], error)
    print("%s: %d series pairs, worst/bound %.4f; direct and clipped tiles worst/bound %.3g" % (
        key, pairs, worst_series, worst_direct))
    # The lines sit where the truncation peaks: far below the bound they did not reach the series.
    assert pairs > 0 and worst_series >= 0.1


@pytest.mark.parametrize("key", fc.TABLE_CASES)
def test_tables_every_line_once(engine, oracle, tables, key):
    from tests.test_gpu_parity import assert_spectrum
    case, table, k_ref = tables[key]
    k = run(engine, case, table, fc.FIVE_LEVELS)
    worst = max(worst_relative(k[l], k_ref[l]) for l in range(len(fc.FIVE_LEVELS)))
    print("%s: worst/bound %.4f of %.3g" % (key, worst/fc.TABLE_TOLERANCE, fc.TABLE_TOLERANCE))
    assert worst <= fc.TABLE_TOLERANCE, key
    ped_ref = reference(oracle, case, table, fc.FIVE_LEVELS, remove_pedestal=True)
    ped = run(engine, case, table, fc.FIVE_LEVELS, remove_pedestal=True)
    described = SimpleNamespace(remove_pedestal=True, n_per_v=case.npv, cut_off=case.cut_off)
    for l in range(len(fc.FIVE_LEVELS)):
        assert_spectrum(ped[l], ped_ref[l], described, "far-field lines %s level %d" % (key, l),
                        k_plain=k_ref[l])


@pytest.mark.parametrize("key", ("A", "B"))
@pytest.mark.parametrize("cut_off", fc.CUT_OFFS)
def test_small_cut_offs(engine, oracle, key, cut_off):
    case = fc.with_cut_off(fc.CASES[key], cut_off)
    table = fc.table_for(case)
    part = fc.partition(case, table, *fc.FIVE_LEVELS[-1])
    k = run(engine, case, table, fc.FIVE_LEVELS)
    if cut_off == 1:
        # Tiles so wide that no line of a window is four half-widths away: the series is off.
        assert part.farfield == 0
        off = run(engine, case, table, fc.FIVE_LEVELS, farfield=0)
        assert np.array_equal(k, off)
        bound = fc.ROUNDING
    else:
        assert part.farfield == 1 and np.any(np.isin(part.classes, fc.SERIES_CLASSES))
        bound = fc.TABLE_TOLERANCE
    k_ref = reference(oracle, case, table, fc.FIVE_LEVELS)
    worst = max(worst_relative(k[l], k_ref[l]) for l in range(len(fc.FIVE_LEVELS)))
    print("%s cut_off %d: worst/bound %.4f of %.3g" % (key, cut_off, worst/bound, bound))
    assert worst <= bound


@pytest.mark.parametrize("key", ("A", "D"))
def test_a_level_depends_on_nothing_but_itself(engine, tables, key):
    """Level l of the five-level call (more than kInlineLevels: the level scalars go through the
    pinned block, far_series and the schedule are offset by level) against a call with that level
    alone, bit for bit."""
    case, table, _ = tables[key]
    together = run(engine, case, table, fc.FIVE_LEVELS)
    for l, level in enumerate(fc.FIVE_LEVELS):
        alone = run(engine, case, table, [level])[0]
        assert np.array_equal(together[l], alone), (key, l, float(np.max(
            np.abs(together[l] - alone))/np.max(alone)))

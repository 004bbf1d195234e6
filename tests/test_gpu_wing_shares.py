"""The far-wing and clipped-window loops of the accumulate kernel line by line
(accumulate_lines.h: fast_ranges, clipped_ranges; accumulate.h: share_of and the 4*parts wavefront
shares of accumulate_tile; lanes_plans.inc: plan_for): parts 1, 2, 3, 5, 13 and the cap of 64,
shares that are empty, one unit long or carry 1 to 3 left-over lines, eights that take their quads
from both ranges, closing fours, batched trips of every length under caps of 2, 4 and 8, two levels
of one call whose own K differ, the plain eight-line groups at P = 1, 2 and 8, clipped windows
grouped, refused at every offset and closing in every row at lane 0 and lane 63, the last row of
the last tile, cut-off 2, aligned tiles, the series on (with the clipped load raising parts) and
accumulating calls.  tests/wing_share_cases.py holds the inputs and a numpy mirror of the index
arithmetic; tests/test_wing_share_cases_host.py proves on the CPU that every case reaches what it
is named for and that every wing or clipped line of the probe tile carries at least 10 x the 1e-6
contract of every point inside its window: the contract sees one lost, doubled or wrongly masked
line.

Bounds, none from the kernel's output: against the CPU oracle zero exactly where it is zero and
the contract REL = 1e-6 elsewhere; with the series off ROUNDING = 1e-12
(tests/test_gpu_core_quotient.py) where N lines cover the point and order(N) = 2 (N - 1) 2^-53 <=
ROUNDING/2, ROUNDING + order(N) beyond (both sides add the same N positive terms in another order:
the argument of tests/test_gpu_inner_pass.py); with the series on SERIES = 1e-9.  Two runs give
the same bits; a cap of wing_batches at or above the level's K leaves every bit unchanged; every
row of a two-level call equals its single-level call bit for bit; an accumulating call leaves
prefill + spectrum within ROUNDING relative of the sum.

Measured on the MI355X, worst relative difference against the oracle per group of cases: the
parts cases 1.1e-14 (parts 64, where 7 971 lines cover a point and the bound is 2.8e-12), parts 13
6.0e-15, the others at most 3.0e-15; the batch cases 5.0e-15 under every cap (1 990 lines in one
item); P = 1, 2, 8 and the aligned tiles 2.3e-15; the row, last-row and cut-off 2 cases 2.0e-15;
the two levels 3.3e-15; the series on 8.7e-15; the accumulating calls 1.2e-15 of the sum.  No
tight bound came within a factor of 150, and no bug was found.

Mutants of the library, one change each, against this file (wrong values only; the figures are
the worst relative difference on the probe tile alone, which the condition of the host test
speaks for -- other tiles, where single lines weigh more, fail as well):
  * fast_ranges without the closing lorentz_four: all 26 oracle tests and both accumulating tests
    fail; on the probe tile 0.4 to 34 per cent in the 21 cases whose probe tile the mirror gives a
    closing four, rounding level in the other five (batch-8, parts-1b, parts-1c, parts-5,
    rows-lane0);
  * share_of's last share ending at its float cut instead of j1: the same 28 tests fail; on the
    probe tile 0.07 (parts 64) to 19 per cent, rounding level only where no range of the probe tile
    leaves a remainder (rows-lane0);
  * clipped_ranges masking with i < last: 22 oracle tests and the parts 2 accumulating test fail,
    on the probe tile by 1.0 to 28 per cent; the four cases that pass (cut-off-2, parts-1,
    parts-1b, parts-1d) are those in which the mirror forms no group whose window closes
    inside its tile.
In all three the mirror names the cases a mutant leaves alone.
"""
import numpy as np
import pytest

from tests import farfield_cases as fc
from tests import wing_share_cases as ws
from tests.test_gpu_wing_batches import expected_batches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def runs(oracle):
    """key -> table and references, each made once and never written to."""
    return ws.Runs(oracle)


class options(object):
    """points_per_lane, farfield, aligned_tiles and wing_batches of a case, put back on the way
    out."""

    def __init__(self, engine, case):
        self.engine, self.case = engine, case

    def __enter__(self):
        self.engine.set_option("points_per_lane", self.case.points)
        self.engine.set_option("farfield", self.case.farfield)
        self.engine.set_option("aligned_tiles", self.case.aligned)
        return self

    def cap(self, batches):
        self.engine.set_option("wing_batches", batches)

    def __exit__(self, *exc):
        self.engine.set_option("points_per_lane", 0)
        self.engine.set_option("farfield", 0)
        self.engine.set_option("aligned_tiles", 0)
        self.engine.set_option("wing_batches", 8)


def compute(engine, molecule, case, levels=None, **more):
    t, p, x = (np.array(column, dtype=np.float64)
               for column in zip(*(case.levels if levels is None else levels)))
    return engine.compute(molecule, t, p, x, case.v0, case.vn, case.npv, cut_off=case.cut_off,
                          **more).copy()


def deviation(k, k_ref):
    """|k - k_ref|/k_ref where the reference is not zero (0 elsewhere); exact zeros asserted."""
    nz = k_ref != 0
    assert np.array_equal(k[~nz], k_ref[~nz]), "non-zero where the reference is zero"
    out = np.zeros(k.shape)
    out[nz] = np.abs(k[nz] - k_ref[nz])/np.abs(k_ref[nz])
    return out


def bound_of(run, level):
    """Per point: SERIES with the series on, else rounding_bound(lines whose windows hold it)."""
    case = run.case
    if case.farfield:
        return np.full(case.n, ws.SERIES)
    covering = ws.lines_covering(case, run.derived[level])
    return np.array([ws.rounding_bound(n) for n in range(int(covering.max()) + 1)])[covering]


def held(run, k, label):
    """One spectrum per level against the oracle: the contract, then the tight bound."""
    worst = 0.
    for level in range(len(run.case.levels)):
        error = deviation(k[level], run.k_ref[level])
        bound = bound_of(run, level)
        ratio = float(np.max(error/bound))
        i0, i1 = fc.tile_bounds(ws.tiling_of(run.case), run.case.tile, run.case.npv, run.case.n)
        print("%s, level %d: worst relative difference %.3g, %.3g x the bound; probe tile %.3g" % (
            label, level, float(error.max()), ratio, float(error[i0:i1 + 1].max())))
        assert error.max() <= ws.REL, label
        assert ratio <= 1., label
        worst = max(worst, float(error.max()))
    return worst


@pytest.mark.parametrize("key", sorted(ws.CASES))
def test_against_the_oracle_and_twice_the_same_bits(engine, runs, key):
    run = runs(key)
    case = run.case
    molecule = engine.load(run.table)
    try:
        with options(engine, case) as chosen:
            for cap in case.caps:
                chosen.cap(cap)
                k = compute(engine, molecule, case)
                again = compute(engine, molecule, case)
                assert np.array_equal(k, again), (case.name, cap)
                held(run, k, "%s, cap %d" % (case.name, cap))
    finally:
        engine.free(molecule)


@pytest.mark.parametrize("key", sorted(ws.BATCH_CASES + ("two-levels",)))
def test_a_cap_at_or_above_the_levels_batches_changes_no_bit(engine, oracle, runs, key):
    run = runs(key)
    case = run.case
    molecule = engine.load(run.table)
    try:
        with options(engine, case) as chosen:
            for level in case.levels:
                batches = expected_batches(oracle, run.table, *level, case.v0, case.vn, case.npv,
                                           case.cut_off)
                chosen.cap(8)
                uncapped = compute(engine, molecule, case, levels=(level,))
                for cap in (2, 4, 8):
                    chosen.cap(cap)
                    capped = compute(engine, molecule, case, levels=(level,))
                    if cap >= batches:
                        assert np.array_equal(capped, uncapped), (case.name, level, cap)
                    elif key == "batch-long":
                        # (The cap is in force: hundreds of eights per wavefront merged otherwise.)
                        assert not np.array_equal(capped, uncapped), (case.name, level, cap)
    finally:
        engine.free(molecule)


def test_every_row_of_a_two_level_call_is_its_single_level_call(engine, runs):
    run = runs("two-levels")
    case = run.case
    molecule = engine.load(run.table)
    try:
        with options(engine, case):
            for levels in (case.levels, case.levels[::-1]):
                together = compute(engine, molecule, case, levels=levels)
                for row, level in enumerate(levels):
                    alone = compute(engine, molecule, case, levels=(level,))
                    assert np.array_equal(together[row], alone[0]), level
    finally:
        engine.free(molecule)


@pytest.mark.parametrize("key", sorted(k for k, c in ws.CASES.items() if c.accumulate))
def test_an_accumulating_call_adds_every_item_once(engine, oracle, runs, key):
    run = runs(key)
    case = run.case
    assert len(case.levels) == 1
    prefill, _ = oracle.absorption_port(ws.second_table(run.table), *case.levels[0], case.v0,
                                        case.vn, case.npv, cut_off=case.cut_off)
    assert prefill.min() > 0.
    out = prefill.reshape(1, -1).copy()
    molecule = engine.load(run.table)
    try:
        with options(engine, case):
            got = compute(engine, molecule, case, out=out, accumulate=True)
    finally:
        engine.free(molecule)
    expect = prefill + run.k_ref[0]
    worst = float(np.max(np.abs(got[0] - expect)/expect))
    print("%s: accumulated against prefill + spectrum %.3g" % (case.name, worst))
    assert worst <= ws.ROUNDING, case.name

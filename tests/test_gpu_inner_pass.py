"""The inner-point pass of the accumulate kernel under load (accumulate_lines.h: inner_ranges ->
inner_batch -> inner_evaluate): several batches of 32 lines per wavefront, class lists filled to
127 entries and carried over flushes, segments over many chunks, segments cut by tiles, by windows
and by the ends of the grid, tiles split into parts (partial slots and combine_kernel), every
range at small cut-offs, with and without the far-field series.  tests/inner_pass_cases.py holds
the inputs and a numpy mirror of the bookkeeping; tests/test_inner_pass_cases_host.py proves on
the CPU that every case reaches what it is named for.  Every line of these tables weighs: a lost,
doubled or misclassified (line, point) pair moves a point by ~1/(10 N) of its value.

Bounds (tests/test_gpu_core_quotient.py's, for this very comparison): against the CPU oracle zero
exactly where it is zero, elsewhere 1e-12 relative with the series off and 1e-9 with it on, never
above the 1e-6 contract; two runs give the same bits; the table against the sum of its lines each
computed alone (one batch of one line, the path the merged suite pins) 1e-12: both sides add the
same N <= 2 000 positive terms in another order, 2 (N - 1) 2^-53 <= 4.5e-13, and the terms differ
by a few roundings (a grouped against a single reciprocal in the wings).

Measured on the MI355X: against the oracle at most 2.0e-14 with the series off (case B), 4.7e-12
with it on; the table against the sum of its lines at most 4.3e-15.  With the last carried entry
of a flushed list left unmoved (one pair lost and one doubled per carry) every test here fails,
by 2 to 700 per cent."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import inner_pass_cases as ip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def runs(oracle):
    """key -> tables and references, each made once and never written to."""
    return ip.Runs(oracle)


def worst_relative(k, k_ref):
    nz = k_ref != 0
    assert np.array_equal(k[~nz], k_ref[~nz]), "non-zero where the reference is zero"
    return float(np.max(np.abs(k[nz] - k_ref[nz])/np.abs(k_ref[nz]))) if nz.any() else 0.


def compute(engine, table, case, **more):
    molecule = engine.load(table)
    try:
        return engine.compute(molecule, ip.T, ip.P_LEVEL, ip.X, case.v0, case.vn, case.npv,
                              cut_off=case.cut_off, **more)[0].copy()
    finally:
        engine.free(molecule)


class options(object):
    """points_per_lane and farfield of a case, put back on the way out."""

    def __init__(self, engine, case):
        self.engine, self.case = engine, case

    def __enter__(self):
        self.engine.set_option("points_per_lane", self.case.points)
        self.engine.set_option("farfield", self.case.farfield)

    def __exit__(self, *exc):
        self.engine.set_option("points_per_lane", 0)
        self.engine.set_option("farfield", 0)


@pytest.mark.parametrize("key", sorted(ip.CASES))
def test_against_the_oracle_and_twice_the_same_bits(engine, runs, key):
    run = runs(key)
    case = run.case
    with options(engine, case):
        k = compute(engine, run.table, case)
        again = compute(engine, run.table, case)
    assert np.array_equal(k, again), case.name
    worst = worst_relative(k, run.k_ref)
    bound = ip.SERIES if case.farfield else ip.ROUNDING
    print("%s: worst relative difference %.3g = %.3g x the bound" % (case.name, worst, worst/bound))
    assert worst <= ip.REL, case.name
    assert worst <= bound, case.name


@pytest.mark.parametrize("key", ip.SUM_OF_LINES)
def test_a_table_is_the_sum_of_its_lines(engine, runs, key):
    run = runs(key)
    case, table = run.case, run.table
    assert not case.farfield and table.num_lines <= ip.MOST_LINES
    index = np.arange(table.num_lines)
    with options(engine, case):
        together = compute(engine, table, case)
        alone = np.zeros_like(together)
        if not run.lines.cluster.all():
            alone += compute(engine, table.subset(~run.lines.cluster), case)
        for j in np.flatnonzero(run.lines.cluster):
            alone += compute(engine, table.subset(index == j), case)
    worst = worst_relative(together, alone)
    print("%s: table against the sum of its lines %.3g" % (case.name, worst))
    assert worst <= ip.ROUNDING, case.name


def test_host_and_device_records_agree(engine, runs):
    run = runs("B-P8")
    case = run.case
    molecule = engine.load(run.table)
    results = []
    try:
        with options(engine, case):
            for prep in (0, 1):
                engine.set_option("prep", prep)
                results.append(engine.compute(molecule, ip.T, ip.P_LEVEL, ip.X, case.v0, case.vn,
                                              case.npv, cut_off=case.cut_off)[0].copy())
    finally:
        engine.set_option("prep", 0)
        engine.free(molecule)
    assert np.array_equal(results[0], results[1])
    assert worst_relative(results[1], run.k_ref) <= ip.ROUNDING


@pytest.mark.parametrize("key", sorted(k for k in ip.CASES if k.startswith("E-")))
def test_every_range_with_the_pedestal_removed(engine, runs, oracle, key):
    from tests.test_gpu_parity import assert_spectrum
    run = runs(key)
    case = run.case
    k_ref, _ = oracle.absorption_port(run.table, ip.T, ip.P_LEVEL, ip.X, case.v0, case.vn,
                                      case.npv, cut_off=case.cut_off, remove_pedestal=True)
    with options(engine, case):
        k = compute(engine, run.table, case, remove_pedestal=True)
    described = SimpleNamespace(remove_pedestal=True, n_per_v=case.npv, cut_off=case.cut_off)
    assert_spectrum(k, k_ref, described, "inner pass %s, pedestal removed" % case.name, run.k_ref)

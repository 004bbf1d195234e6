"""The scaled eights of the far-wing loop of accumulate_kernel<4> on the GPU
(accumulate_lines.h: scaled_ranges; tests/wing_scaled_cases.py holds the cases and the mirror,
tests/test_wing_scaled_host.py proves on the CPU that every case reaches what it is named for).
Bounds, none from the kernel's output and none redefined here (tests/wing_share_cases.py): against
the CPU oracle zero exactly where it is zero, the contract REL elsewhere, then ROUNDING where N
lines cover a point and order(N) <= ROUNDING/2, ROUNDING + order(N) beyond.  Two runs give the
same bits; LBL_PREP_HOST and device prep give the same bits; a cap of wing_batches at or above the
level's K changes no bit and, where K >= 4, a cap of K/4 does; every row of a two-level call is
its single-level call; accumulate and scale_density hold; points_per_lane 1, 2 and 8 go through
the old loop and still hold."""
import numpy as np
import pytest

from tests import wing_scaled_cases as wc
from tests import wing_share_cases as ws
from tests.test_gpu_wing_shares import deviation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import Engine
    e = Engine(0)
    yield e
    e.set_option("prep", 0)
    e.set_option("points_per_lane", 0)
    e.set_option("wing_batches", 8)
    e.close()


@pytest.fixture(scope="module")
def runs(oracle):
    return wc.Runs(oracle)


def compute(engine, molecule, case, levels=None, cap=8, prep=0, **more):
    engine.set_option("points_per_lane", case.points)
    engine.set_option("wing_batches", cap)
    engine.set_option("prep", prep)
    try:
        t, p, x = (np.array(column, dtype=np.float64)
                   for column in zip(*(case.levels if levels is None else levels)))
        return engine.compute(molecule, t, p, x, case.v0, case.vn, case.npv,
                              cut_off=case.cut_off, **more).copy()
    finally:
        engine.set_option("points_per_lane", 0)
        engine.set_option("wing_batches", 8)
        engine.set_option("prep", 0)


def held(run, k, label):
    for level in range(len(run.case.levels)):
        error = deviation(k[level], run.k_ref[level])
        covering = ws.lines_covering(run.case, run.derived[level])
        bound = np.array([ws.rounding_bound(n) for n in range(int(covering.max()) + 1)])[covering]
        print("%s, level %d: worst relative difference %.3g, %.3g x the bound" % (
            label, level, float(error.max()), float(np.max(error/bound))))
        assert error.max() <= ws.REL, label
        assert np.max(error/bound) <= 1., label


@pytest.mark.parametrize("key", sorted(wc.CASES))
def test_against_the_oracle_twice_and_under_both_preps(engine, runs, key):
    run = runs(key)
    case = run.case
    molecule = engine.load(run.table)
    try:
        for cap in case.caps:
            k = compute(engine, molecule, case, cap=cap)
            assert np.array_equal(k, compute(engine, molecule, case, cap=cap)), (key, cap)
            assert np.array_equal(k, compute(engine, molecule, case, cap=cap, prep=1)), (key, cap)
            held(run, k, "%s, cap %d" % (case.name, cap))
    finally:
        engine.free(molecule)


@pytest.mark.parametrize("key, batches", [("parts-5", 8), ("K-4", 4), ("K-2", 2), ("K-1", 1)])
def test_caps(engine, runs, key, batches):
    run = runs(key)
    molecule = engine.load(run.table)
    try:
        uncapped = compute(engine, molecule, run.case, cap=8)
        for cap in (2, 4, 8):
            capped = compute(engine, molecule, run.case, cap=cap)
            if cap >= batches:
                assert np.array_equal(capped, uncapped), (key, cap)
        if batches >= 4:
            quarter = compute(engine, molecule, run.case, cap=batches//4)
            assert not np.array_equal(quarter, uncapped), key
            held(run, quarter, "%s, cap %d" % (key, batches//4))
    finally:
        engine.free(molecule)


def test_every_row_of_a_two_level_call_is_its_single_level_call(engine, runs):
    run = runs("two-levels")
    case = run.case
    molecule = engine.load(run.table)
    try:
        for levels in (case.levels, case.levels[::-1]):
            together = compute(engine, molecule, case, levels=levels)
            for row, level in enumerate(levels):
                alone = compute(engine, molecule, case, levels=(level,))
                assert np.array_equal(together[row], alone[0]), level
    finally:
        engine.free(molecule)


def test_accumulate_and_scale_density(engine, oracle, runs):
    run = runs("parts-2")
    case = run.case
    level = case.levels[0]
    other = run.table.subset(np.arange(run.table.num_lines) % 2 == 0)
    prefill, _ = oracle.absorption_port(other, *level, case.v0, case.vn, case.npv,
                                        cut_off=case.cut_off)
    molecule = engine.load(run.table)
    try:
        out = prefill.reshape(1, -1).copy()
        got = compute(engine, molecule, case, out=out, accumulate=True)
        expect = prefill + run.k_ref[0]
        assert np.max(np.abs(got[0] - expect)/expect) <= ws.ROUNDING
        plain = compute(engine, molecule, case)
        scaled = compute(engine, molecule, case, scale_density=True)
        ratio = scaled[0][plain[0] > 0]/plain[0][plain[0] > 0]
        assert np.max(np.abs(ratio/ratio[0] - 1.)) <= 4.*2.**-53 and ratio[0] > 1.
    finally:
        engine.free(molecule)

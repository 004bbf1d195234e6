"""The per-line scalars (csrc/line_prep.h: prepare_line, fed by fill_level of csrc/lanes_plans.inc,
run by prologue_kernel or, with prep = 1, on the host; returned in the reference's row order by
derived_to_host) through Engine.line_scalars and Engine.compute: by isotopologue slot, at the
extremes of the line parameters, at every edge of the window rule, with the shifted centre on an
integer, on permuted tables under both range policies, at the wave and block edges of
prepare_block and with rows that have no mass or no partition-function row.  Inputs and the two
mirrors are tests/line_scalar_cases.py; tests/test_line_scalar_cases_host.py checks them on the CPU.

Bounds, none taken from the code under test.
  * status, first, last: exact against the float64 mirror, both prep values.
  * prep = 1 (the host's own prepare_line): the CPU oracle's `derived` bit for bit, every column.
  * prep = 0 (the device): centre and alpha bit-equal (one product and one sum, one quotient and
    one product, nothing fused: a fused centre moves the windows of family F by n_per_v points);
    gamma and strength within (4 E_cpu + 1) u K of the long-double mirror per line, u = 2^-53,
    K_g = 1 + |n_air ln(tfact)|, K_s = 1 + |elower c2 (T - 296)/(T 296)| + 1/|1 - gg| +
    1/|1 - gref|, E_cpu = 2.94 (gamma) and 1.68 (strength) the float64 mirror's own worst error
    in these units over these very cases, 4 the project's margin for device against host rounding.
  * Row order: the permuted table's result is the sorted table's gathered by the stable
    permutation, bit for bit.
  * Spectra of family S: assert_spectrum of tests/test_gpu_parity.py against the oracle.
test_zz_error_to_bound_report prints the worst error-to-bound ratio per family.
"""
import time
from types import SimpleNamespace

import numpy as np
import pytest

from tests import line_scalar_cases as lc

pytestmark = pytest.mark.gpu

LBL_OUT_OF_RANGE = 4        # include/lbl_amd.h
RATIOS = {}                 # family -> [gamma, strength]: worst error over bound, prep = 0
SECONDS = {}


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import Engine
    e = Engine(0)
    yield e
    e.set_option("prep", 0)
    e.close()


@pytest.fixture(scope="module")
def references(oracle):
    """(case name, level, policy) -> (float64 mirror, oracle's derived): made once, read-only."""
    out = {}
    for case, level, policy in lc.walk():
        pair = (lc.mirror64(case, level, policy), lc.oracle_derived(oracle, case, level, policy))
        for array in pair:
            array.setflags(write=False)
        out[case.name, level, policy] = pair
    return out


def scalars(engine, molecule, case, level, policy="reference", prep=0, table=None):
    table = case.table if table is None else table
    engine.set_option("prep", prep)
    try:
        return engine.line_scalars(molecule, table.num_lines, *level, case.v0, case.vn, case.npv,
                                   cut_off=case.cut_off, range_policy=policy).copy()
    finally:
        engine.set_option("prep", 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", list(lc.cases()))
def test_columns(engine, references, name):
    case = lc.cases()[name]
    started = time.perf_counter()
    molecule = engine.load(case.table)
    try:
        for level in case.levels:
            for policy in case.policies:
                what = "%s, %s, %s" % (name, level, policy)
                mirror, oracle_rows = references[name, level, policy]
                host = scalars(engine, molecule, case, level, policy, prep=1)
                assert same_bits(host, oracle_rows), what + ": prep = 1 against the oracle"
                got = scalars(engine, molecule, case, level, policy, prep=0)
                assert np.array_equal(got[:, 4:7], mirror[:, 4:7]), what + ": window and status"
                assert np.array_equal(host[:, 4:7], mirror[:, 4:7]), what
                assert same_bits(got[:, 0], mirror[:, 0]), what + ": centre"
                assert same_bits(got[:, 1], mirror[:, 1]), what + ": alpha"
                assert np.all(got[:, 7] == 0.)
                unreached = mirror[:, 6] == -1.
                assert np.all(got[unreached, :6] == 0.), what + ": rows never reached"
                ratio = lc.bound_ratio(got, case, level, policy)
                worst = RATIOS.setdefault(case.family, [0., 0.])
                worst[0], worst[1] = max(worst[0], ratio[0]), max(worst[1], ratio[1])
                print("%s: gamma %.3f, strength %.3f of the bound" % ((what,) + ratio))
                assert ratio[0] <= 1., what + ": gamma"
                assert ratio[1] <= 1., what + ": strength"
    finally:
        engine.free(molecule)
    SECONDS[name] = time.perf_counter() - started


def test_refused_levels_leave_the_engine_usable(engine):
    from pylbl_amd.errors import EngineError
    case = lc.cases()["S"]
    molecule = engine.load(case.table)
    narrow_table = lc.s_table((300, 400))
    narrow = engine.load(narrow_table)
    try:
        for prep in (0, 1):
            before = scalars(engine, molecule, case, case.levels[3], prep=prep)
            for level in lc.S_REFUSED:
                with pytest.raises(EngineError, match="outside the partition-function table"):
                    scalars(engine, molecule, case, level, prep=prep)
                assert same_bits(scalars(engine, molecule, case, case.levels[3], prep=prep), before)
            with pytest.raises(EngineError, match="status %d: level 0" % LBL_OUT_OF_RANGE):
                scalars(engine, narrow, case, lc.S_NO_REFERENCE_LEVEL, prep=prep,
                        table=narrow_table)
            assert same_bits(scalars(engine, molecule, case, case.levels[3], prep=prep), before)
            # A refused level in a compute call of several: nothing of the call is returned.
            t, p, x = (np.array(c) for c in zip(case.levels[0], lc.S_REFUSED[1], case.levels[1]))
            with pytest.raises(EngineError, match="level 1"):
                engine.set_option("prep", prep)
                try:
                    engine.compute(molecule, t, p, x, case.v0, case.vn, case.npv)
                finally:
                    engine.set_option("prep", 0)
            assert same_bits(scalars(engine, molecule, case, case.levels[3], prep=prep), before)
    finally:
        engine.free(narrow)
        engine.free(molecule)


def test_bad_rows_outside_the_range_touch_no_other_row(engine):
    case = lc.cases()["B outside"]
    good = np.setdiff1d(np.arange(case.table.num_lines), lc.B_OUT_AT)
    good_table = lc.take(case.table, good)
    molecule, without = engine.load(case.table), engine.load(good_table)
    try:
        for prep in (0, 1):
            got = scalars(engine, molecule, case, lc.B_LEVEL, "skip", prep)
            assert np.all(got[list(lc.B_OUT_AT), 6] == -1.)
            assert np.all(np.delete(got[list(lc.B_OUT_AT)], 6, axis=1) == 0.)
            alone = scalars(engine, without, case, lc.B_LEVEL, "skip", prep, table=good_table)
            assert np.all(alone[:, 6] >= 0.)
            assert same_bits(got[good], alone)
            # The reference's policy: the first bad row is the first row out of range.
            got = scalars(engine, molecule, case, lc.B_LEVEL, "reference", prep)
            assert np.all(got[lc.B_OUT_AT[0]:, 6] == -1.) and np.all(got[lc.B_OUT_AT[0]:, :6] == 0.)
            assert same_bits(got[:lc.B_OUT_AT[0]], alone[:lc.B_OUT_AT[0]])
    finally:
        engine.free(without)
        engine.free(molecule)


@pytest.mark.parametrize("bad", lc.B_IDS)
def test_bad_row_inside_the_range_is_named_in_row_order(engine, bad):
    from pylbl_amd.errors import EngineError
    table = lc.b_inside(bad)
    case = lc._case("B inside", "B", table, lc.GRID, (lc.B_LEVEL,))
    assert not np.all(np.diff(table.nu) >= 0.)      # permuted: the sorted index is another
    assert int(np.argsort(table.nu, kind="stable").tolist().index(lc.B_IN_AT)) != lc.B_IN_AT
    good = lc.cases()["B outside"]
    molecule, other = engine.load(table), engine.load(good.table)
    try:
        before = scalars(engine, other, good, lc.B_LEVEL, "skip")
        message = "status %d: row %d: local_iso_id %d has no mass" % (LBL_OUT_OF_RANGE,
                                                                      lc.B_IN_AT, bad)
        for prep in (0, 1):
            for policy in ("reference", "skip"):
                with pytest.raises(EngineError, match=message):
                    scalars(engine, molecule, case, lc.B_LEVEL, policy, prep)
                with pytest.raises(EngineError, match=message):
                    engine.compute(molecule, *lc.B_LEVEL, case.v0, case.vn, case.npv,
                                   range_policy=policy)
        # A grid whose range rule leaves the row out evaluates the others.
        away = lc._case("B away", "B", table, (int(table.nu[lc.B_IN_AT]) + 3,
                                               int(table.nu[lc.B_IN_AT]) + 35, 10, 1),
                        (lc.B_LEVEL,))
        got = scalars(engine, molecule, away, lc.B_LEVEL, "skip")
        assert np.array_equal(got[:, 4:7], lc.mirror64(away, lc.B_LEVEL, "skip")[:, 4:7])
        assert got[lc.B_IN_AT, 6] == -1. and np.count_nonzero(got[:, 6] == 1.) > 0
        assert same_bits(scalars(engine, other, good, lc.B_LEVEL, "skip"), before)
    finally:
        engine.free(other)
        engine.free(molecule)


@pytest.mark.parametrize("name, policy", [("R0", "reference"), ("R0", "skip"), ("R", "skip")])
def test_rows_come_back_in_the_reference_order(engine, references, name, policy):
    case = lc.cases()[name]
    order = np.argsort(case.table.nu, kind="stable")
    assert not np.array_equal(order, np.arange(order.size))
    sorted_table = lc.take(case.table, order)
    molecule, ascending = engine.load(case.table), engine.load(sorted_table)
    try:
        for prep in (0, 1):
            got = scalars(engine, molecule, case, lc.R_LEVEL, policy, prep)
            straight = scalars(engine, ascending, case, lc.R_LEVEL, policy, prep,
                               table=sorted_table)
            assert same_bits(got[order], straight)
            assert np.array_equal(got[:, 4:7], references[name, lc.R_LEVEL, policy][0][:, 4:7])
            # Every row is its own: no two rows of a group of equal nu were exchanged.
            assert np.unique(got[got[:, 6] >= 0., 3]).size == np.count_nonzero(got[:, 6] >= 0.)
    finally:
        engine.free(ascending)
        engine.free(molecule)


def test_rows_after_an_outside_row_are_never_reached(engine, references):
    case = lc.cases()["R"]
    molecule = engine.load(case.table)
    try:
        for prep in (0, 1):
            got = scalars(engine, molecule, case, lc.R_LEVEL, "reference", prep)
            assert np.all(got[lc.R_OUTSIDE_AT:, 6] == -1.)
            assert np.all(got[:lc.R_OUTSIDE_AT, 6] >= 0.)
            assert np.all(got[lc.R_OUTSIDE_AT:, :6] == 0.)
            k, evals = engine.compute(molecule, *lc.R_LEVEL, case.v0, case.vn, case.npv,
                                      want_evals=True)
            assert evals == lc.evals_of(references["R", lc.R_LEVEL, "reference"][0])
    finally:
        engine.free(molecule)


@pytest.mark.parametrize("n_lines", lc.N_LINES)
def test_eval_count_is_the_sum_of_the_windows(engine, references, oracle, n_lines):
    from tests.test_gpu_parity import assert_spectrum
    case = lc.cases()["N %d" % n_lines]
    described = SimpleNamespace(remove_pedestal=False, n_per_v=case.npv, cut_off=case.cut_off)
    mirror = references[case.name, lc.N_LEVEL, "reference"][0]
    k_ref, extras = oracle.absorption_port(case.table, *lc.N_LEVEL, case.v0, case.vn, case.npv,
                                           cut_off=case.cut_off)
    assert extras["evals"] == lc.evals_of(mirror)
    molecule = engine.load(case.table)
    try:
        for prep in (0, 1):
            engine.set_option("prep", prep)
            k, evals = engine.compute(molecule, *lc.N_LEVEL, case.v0, case.vn, case.npv,
                                      cut_off=case.cut_off, want_evals=True)
            assert evals == lc.evals_of(mirror), (n_lines, prep)
            assert_spectrum(k[0], k_ref, described, "N %d, prep %d" % (n_lines, prep))
    finally:
        engine.set_option("prep", 0)
        engine.free(molecule)


def test_a_table_without_lines(engine):
    """The engine takes an empty table: no rows, no evaluations, a spectrum of zeros."""
    table = lc.empty_table()
    molecule = engine.load(table)
    try:
        v0, vn, npv, cut_off = lc.GRID
        for prep in (0, 1):
            engine.set_option("prep", prep)
            got = engine.line_scalars(molecule, 0, *lc.N_LEVEL, v0, vn, npv, cut_off=cut_off)
            assert got.shape == (0, 8)
            k, evals = engine.compute(molecule, *lc.N_LEVEL, v0, vn, npv, cut_off=cut_off,
                                      want_evals=True)
            assert evals == 0 and k.shape == (1, (vn - v0)*npv) and np.all(k == 0.)
    finally:
        engine.set_option("prep", 0)
        engine.free(molecule)


@pytest.fixture(scope="module")
def s_spectra(oracle):
    """remove_pedestal -> oracle spectra [5, n] of family S."""
    case = lc.cases()["S"]
    out = {}
    for remove_pedestal in (False, True):
        k = np.array([oracle.absorption_port(case.table, t, p, x, case.v0, case.vn, case.npv,
                                             cut_off=case.cut_off,
                                             remove_pedestal=remove_pedestal)[0]
                      for t, p, x in case.levels])
        k.setflags(write=False)
        out[remove_pedestal] = k
    return out


@pytest.mark.parametrize("remove_pedestal", [False, True])
@pytest.mark.parametrize("farfield", [False, True])
def test_spectra_of_the_slots(engine, s_spectra, farfield, remove_pedestal):
    """End to end on S: a q_ratio or a Doppler width from another slot moves these spectra by per
    cent.  Five levels in one call (past kInlineLevels) are the five single-level calls."""
    from tests.test_gpu_parity import assert_spectrum
    case = lc.cases()["S"]
    assert len(case.levels) == lc.INLINE_LEVELS + 1
    described = SimpleNamespace(remove_pedestal=remove_pedestal, n_per_v=case.npv,
                                cut_off=case.cut_off)
    t, p, x = (np.array(c) for c in zip(*case.levels))
    molecule = engine.load(case.table)
    try:
        together = engine.compute(molecule, t, p, x, case.v0, case.vn, case.npv,
                                  cut_off=case.cut_off, remove_pedestal=remove_pedestal,
                                  farfield=farfield).copy()
        for l, level in enumerate(case.levels):
            what = "S level %d, farfield %d, pedestal %d" % (l, farfield, remove_pedestal)
            assert_spectrum(together[l], s_spectra[remove_pedestal][l], described, what,
                            k_plain=s_spectra[False][l])
            alone = engine.compute(molecule, *level, case.v0, case.vn, case.npv,
                                   cut_off=case.cut_off, remove_pedestal=remove_pedestal,
                                   farfield=farfield)
            assert same_bits(alone[0], together[l]), what + ": alone against together"
    finally:
        engine.free(molecule)


def test_zz_error_to_bound_report():
    """What the device's gamma and strength used of their bound, per family (run after
    test_columns)."""
    print("worst error over bound (gamma, strength):",
          {k: "%.3f, %.3f" % tuple(v) for k, v in sorted(RATIOS.items())})
    print("slowest test_columns cases [s]:",
          sorted(((round(v, 3), k) for k, v in SECONDS.items()), reverse=True)[:3])
    assert sorted(RATIOS) in ([], sorted("SEWFRNB"))       # (empty: this test run on its own)
    assert all(0. <= r <= 1. for pair in RATIOS.values() for r in pair)

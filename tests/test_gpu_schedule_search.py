"""The table searches of the tile schedule (csrc/tile_schedule.h: search_bracket and the eight
searches of schedule_tile; csrc/engine.hip: the cell_first block of lbl_molecule_load) through the
spectra they lead to.  Inputs and a numpy mirror of the searches are
tests/schedule_search_cases.py; tests/test_schedule_search_cases_host.py checks them on the CPU
and shows which mutants of the bracket drop lines from tiles these cases run.

One base table and six variants of it that differ in one inert line far outside every window:
`fine` (none: 8 cells per cm-1), `switch` (7.875), `coarse` (3.375), `coarsest` (0.125), `none`
(no cell table, every search takes the whole table) and `below` (3.375 from a negative base).
Windows inside the table across runs of empty cells, across its first and its last line, and out
of its reach on either side; cut-offs 25 and 3; cell-aligned and unaligned tiles.

  * Every (variant, window) against the CPU oracle by assert_spectrum of tests/test_gpu_parity.py
    (1e-6 and its pedestal rules): pedestal on and off, far-field series on and off, line
    scalars made on the device (prologue_kernel) and on the host (schedule_kernel alone), two
    levels (level scalars as kernel arguments) and five (read from memory), range policy `skip`
    with the in-range rows for the oracle, and `reference` with the whole table where the inert
    line lies above.
  * Between the variants, bit for bit: the inert line moves no level scalar, no plan weight and
    no wing bound, and the accumulate kernel, the series and the pedestal pass address lines
    relative to the ranges of the schedule -- what is left is how the searches are bracketed.
    `none` is what the others are held to.  No pair needed an exception.
  * The base table with its rows permuted: the stable sort, then the cell table, bit for bit
    what the sorted table gives -- with the pedestal removed against the oracle on the permuted
    rows, since the pedestals follow the row order by the reference's own definition.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import schedule_search_cases as sc

pytestmark = pytest.mark.gpu

LEVEL_SETS = (sc.TWO_LEVELS, sc.FIVE_LEVELS)


@pytest.fixture(scope="module")
def setup():
    """One engine with every variant loaded: (engine, {variant: handle})."""
    from pylbl_amd.engine import Engine
    e = Engine(0)
    handles = {}
    try:
        for name, (table, _) in sc.variants().items():
            handles[name] = e.load(table)
        yield e, handles
    finally:
        for handle in handles.values():
            e.free(handle)
        e.close()


@pytest.fixture(scope="module")
def references(oracle):
    """(table key, case key, pedestal) -> [5 levels, n] of the oracle, made once each and never
    written to.  Table key: "in range" (the rows the skip policy accepts, the same for every
    variant) or the name of a variant (its whole table, for the reference policy)."""
    made = {}

    def reference(which, key, remove_pedestal):
        if (which, key, remove_pedestal) not in made:
            case = sc.CASES[key]
            base = sc.variants()["fine"][0]
            table = sc.in_range(base, case) if which == "in range" else sc.variants()[which][0]
            out = np.array([oracle.absorption_port(table, t, p, sc.X, case.v0, case.vn, case.npv,
                                                   cut_off=case.cut_off,
                                                   remove_pedestal=remove_pedestal)[0]
                            for t, p in sc.FIVE_LEVELS])
            out.setflags(write=False)
            made[which, key, remove_pedestal] = out
        return made[which, key, remove_pedestal]
    return reference


def compute(engine, handle, case, levels, remove_pedestal, range_policy):
    t = np.array([level[0] for level in levels])
    p = np.array([level[1] for level in levels])
    return engine.compute(handle, t, p, np.full(len(levels), sc.X), case.v0, case.vn, case.npv,
                          cut_off=case.cut_off, remove_pedestal=remove_pedestal,
                          range_policy=range_policy).copy()


def against_the_oracle(k, references, which, key, levels, remove_pedestal, label):
    from tests.test_gpu_parity import assert_spectrum
    case = sc.CASES[key]
    described = SimpleNamespace(remove_pedestal=remove_pedestal, n_per_v=case.npv,
                                cut_off=case.cut_off)
    k_ref = references(which, key, remove_pedestal)
    k_plain = references(which, key, False)
    for l, level in enumerate(levels):
        row = sc.FIVE_LEVELS.index(level)
        assert_spectrum(k[l], k_ref[row], described, "%s level %d" % (label, l),
                        k_plain=k_plain[row])


@pytest.mark.parametrize("key", list(sc.CASES))
def test_every_variant_computes_the_same_spectrum(setup, references, key):
    engine, handles = setup
    case = sc.CASES[key]
    calls = 0
    try:
        engine.set_option("points_per_lane", case.points)
        for prep in (0, 1):
            engine.set_option("prep", prep)
            for farfield in (0, 1):
                engine.set_option("farfield", farfield)
                for levels in LEVEL_SETS:
                    for remove_pedestal in (False, True):
                        what = "%s, prep %d, farfield %d, %d levels, pedestal %d" % (
                            key, prep, farfield, len(levels), remove_pedestal)
                        k = {name: compute(engine, handles[name], case, levels, remove_pedestal,
                                           "skip") for name in sc.VARIANTS}
                        calls += len(k)
                        for name in sc.VARIANTS:
                            against_the_oracle(k[name], references, "in range", key, levels,
                                               remove_pedestal, "%s, %s, skip" % (what, name))
                            assert np.array_equal(k[name], k["none"]), \
                                "%s: %s differs from none at %d points, by up to %.3g relative" % (
                                    what, name, np.count_nonzero(k[name] != k["none"]),
                                    np.max(np.abs(k[name] - k["none"]))/np.max(k["none"]))
                        if key in sc.OUT_OF_REACH:
                            assert not np.any(k["none"]), what
                        else:
                            assert np.all(k["none"].max(axis=1) > 0.), what
                        if prep == 1 or len(levels) > 2:
                            continue
                        # The reference policy: the rows up to the first one out of range, which
                        # the inert line is where it lies above the table.
                        for name in ("fine",) + sc.ABOVE:
                            got = compute(engine, handles[name], case, levels, remove_pedestal,
                                          "reference")
                            calls += 1
                            against_the_oracle(got, references, name, key, levels,
                                               remove_pedestal, "%s, %s, reference" % (what, name))
                            first_row_accepted = case.v0 - (case.cut_off + 1) <= sc.FIRST <= \
                                case.vn + case.cut_off + 1
                            # (the base table's rows ascend: from an accepted first row on, the
                            # policies accept the same rows)
                            assert np.array_equal(got, k["none"]) if first_row_accepted else \
                                not np.any(got), (what, name)
    finally:
        for option in ("points_per_lane", "prep", "farfield"):
            engine.set_option(option, 0)
    print("%s: %d calls" % (key, calls))


@pytest.mark.parametrize("key", ["a aligned 500", "a unaligned 512", "b cut 3", "c cut 25"])
def test_rows_in_another_order(setup, oracle, key):
    """The base table with its rows permuted (the nine duplicates and the dense cell in another
    row order), under the skip policy: after the stable sort the positions, and so the cell table
    and every search, are those of the sorted table, and lines on one position are alike in
    every column; the spectra are the sorted table's bit for bit.
    With the pedestal removed they are not, and must not be: every line's pedestal is taken from
    the spectrum of the rows before it (spectra.c:66-78; csrc/pedestal.h walks the runs in the
    reference's row order), so another row order is another result.  There the permuted rows go to
    the oracle, in their order, and the comparison is assert_spectrum's."""
    from tests.test_gpu_parity import assert_spectrum
    engine, handles = setup
    case = sc.CASES[key]
    base = sc.variants()["fine"][0]
    shuffled = base.subset(np.random.default_rng(7).permutation(base.num_lines))
    assert not np.all(np.diff(shuffled.nu) >= 0.)
    described = SimpleNamespace(remove_pedestal=True, n_per_v=case.npv, cut_off=case.cut_off)
    source = sc.in_range(shuffled, case)
    handle = engine.load(shuffled)
    try:
        engine.set_option("points_per_lane", case.points)
        for farfield in (0, 1):
            engine.set_option("farfield", farfield)
            for levels in LEVEL_SETS:
                got = compute(engine, handle, case, levels, False, "skip")
                expect = compute(engine, handles["fine"], case, levels, False, "skip")
                assert np.any(expect)
                assert np.array_equal(got, expect), (key, farfield, len(levels))
            got = compute(engine, handle, case, sc.TWO_LEVELS, True, "skip")
            for l, (t, p) in enumerate(sc.TWO_LEVELS):
                k_ref, k_plain = (oracle.absorption_port(
                    source, t, p, sc.X, case.v0, case.vn, case.npv, cut_off=case.cut_off,
                    remove_pedestal=pedestal)[0] for pedestal in (True, False))
                assert_spectrum(got[l], k_ref, described, "%s permuted, farfield %d, level %d" % (
                    key, farfield, l), k_plain=k_plain)
    finally:
        engine.free(handle)
        engine.set_option("points_per_lane", 0)
        engine.set_option("farfield", 0)

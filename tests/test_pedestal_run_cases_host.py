"""CPU checks behind tests/test_gpu_pedestal_many_runs.py: through the mirror of
tests/pedestal_run_cases.py every case and level has the run count, the fall-back predicates and
the margins from the cuts it is named for; the mirror's runs are the reference's (the recurrence
of csrc/pedestal.h's header comment replayed on them in float64 meets
oracle.absorption_port(..., remove_pedestal=True), kRunCut cuts included); the runs past the first
launch row are visible in the result a thousand times above the comparison's bar; and no case
needs the conditioning allowance of tests/test_gpu_parity.py::assert_spectrum."""
import numpy as np
import pytest

from tests import pedestal_run_cases as cases
from tests.test_gpu_parity import CONDITIONING_MARGIN, REL, oracle_conditioning

LEVELS = range(cases.LEVEL_P.size)


def test_constants_are_the_headers():
    found = cases.header_constants()
    assert found == {"GRID_X": {"run_sums_kernel": [65535], "run_links_kernel": [65535]},
                     "kRunCut": 1024, "kMaxStretch": 1024, "kMaxHistory": 16384, "chunk": 64}
    assert (cases.GRID_X, cases.RUN_CUT, cases.MAX_STRETCH, cases.MAX_HISTORY, cases.CHUNK) == \
        (65535, 1024, 1024, 16384, 64)
    chain = (cases.CSRC / "pedestal_chain.h").read_text()
    runs = (cases.CSRC / "pedestal_runs.h").read_text()
    # the decisions the mirror restates, as the kernels spell them
    for statement in ("const bool too_long = r - begin > kMaxHistory;",
                      "const int begin = wave_lower_bound(prefix, 0, r, m.first_slot);",
                      "const bool displaced = !bin_ok || (r > 0 && prefix[r - 1] > m.bin + 1);",
                      "bin_end[(long long)level*n_bins + mine.bin] - r > kMaxStretch)",
                      "const int base = chunk*64;"):
        assert statement in chain, statement
    for statement in ("if (r % kRunCut == 0) return 1;",
                      "for (int run = blockIdx.x; run < count; run += gridDim.x)",
                      "meta.bin = (int)floor(head.centre) - (g.v0 - g.cut_off - 1);"):
        assert statement in runs, statement
    assert "for (int r = blockIdx.x; r < count; r += gridDim.x)" in chain


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_is_what_it_is_named_for(name):
    case = cases.case(name)
    assert np.all(np.diff(case.table.nu) > 0.)
    for level in LEVELS:
        runs = cases.runs_of(name, level)
        where = f"{name} level {level}"
        assert runs.integer_margin >= cases.INTEGER_MARGIN, where
        assert not runs.displaced, where
        wanted = case.fall_back[level].split()
        assert runs.too_long == ("too_long" in wanted), where
        assert runs.stretch_cut == ("stretch_cut" in wanted), where
        assert cases.falls_back(runs) == bool(wanted), where
        assert case.bits[level] == "same" or not wanted, where      # the serial chain's bits
        history, stretch = int(runs.history.max()), int(runs.stretch.max())
        if name in cases.ON_THE_HISTORY_CUT and level == cases.TOP:
            assert np.count_nonzero(runs.history > cases.MAX_HISTORY) == \
                cases.ON_THE_HISTORY_CUT[name] <= cases.CHUNK, where
            assert np.all(np.flatnonzero(runs.history > cases.MAX_HISTORY) >=
                          runs.run_count - cases.ON_THE_HISTORY_CUT[name]), where     # the last runs
        else:
            assert history <= cases.HISTORY_BELOW or history >= cases.HISTORY_ABOVE, (where, history)
        assert stretch <= cases.STRETCH_BELOW or stretch >= cases.STRETCH_ABOVE, (where, stretch)
        assert cases.HISTORY_BELOW < cases.MAX_HISTORY < cases.HISTORY_ABOVE
        assert cases.STRETCH_BELOW < cases.MAX_STRETCH < cases.STRETCH_ABOVE
    counts = [cases.runs_of(name, level).run_count for level in LEVELS]
    top = counts[cases.TOP]
    assert top == max(counts) and len(set(counts)) == len(counts)     # one stride, three counts
    assert counts[0] < cases.GRID_X         # the low level: about a run per window
    if case.over == ">":
        assert cases.GRID_X + cases.CHUNK <= top <= 2*cases.GRID_X
    elif case.over == ">>":
        assert top > 2*cases.GRID_X
    elif case.over == "<":
        assert top < cases.GRID_X
    else:
        assert top == case.over
    assert case.trips == -(-top//cases.GRID_X)
    if case.over in (">", ">>"):
        assert -(-top//cases.CHUNK) > 1024      # chunks of run_solve_kernel per level


def test_three_trips_and_both_edges_are_among_the_cases():
    trips = {name: cases.case(name).trips for name in cases.NAMES}
    assert 3 in trips.values()
    assert cases.MANY_TRIPS == tuple(name for name in cases.NAMES if trips[name] > 1)
    assert cases.runs_of("B65535", cases.TOP).run_count == cases.GRID_X
    assert cases.runs_of("B65536", cases.TOP).run_count == cases.GRID_X + 1
    # settled on the long side: the history walks of B are thousands of runs (dozens of LDS tiles)
    assert cases.runs_of("B", cases.TOP).history.max() > 14000
    # too_long alone, the stretch cut alone
    assert cases.case("C1'").fall_back[cases.TOP] == "too_long"
    assert cases.case("C2").fall_back[cases.TOP] == "stretch_cut"


@pytest.mark.parametrize("name", ["D25", "D40"])
def test_run_cut_case(name):
    """One window of 3 100 rows that begins on row 300 (no multiple of 64) and is cut at rows
    1 024, 2 048 and 3 072; a window change on row 4 096; the last run is row 5 120, the cut's."""
    table = cases.case(name).table
    cut = cases.RUN_CUT
    assert table.num_lines % cut == 1 and table.num_lines >= 4*cut + 1
    for level in LEVELS:
        runs = cases.runs_of(name, level)
        same = np.zeros(table.num_lines, bool)
        same[1:] = (runs.first[1:] == runs.first[:-1]) & (runs.last[1:] == runs.last[:-1])
        begin = 300
        assert begin % 64 != 0 and runs.opens[begin] and not same[begin]
        assert same[begin + 1:begin + 3100].all()
        for row in (cut, 2*cut, 3*cut):
            assert begin < row < begin + 3100 and runs.opens[row] and same[row]
        assert np.count_nonzero(runs.opens[begin:begin + 3100]) == 4
        assert runs.opens[4*cut] and not same[4*cut]
        assert same[4*cut + 1:].all()
        assert runs.row_begin[-1] == 5*cut == table.num_lines - 1 and same[5*cut]
        # (wider than one pass of 64 slots at cut_off 40: two slot passes in run_sums_kernel)
        assert (runs.n_slots.max() > 64) == (name == "D40")


def _spectrum_error(k, k_ref, k_plain, grid):
    return float(np.max(np.abs(k - k_ref)/cases.plain_tolerance(k_ref, k_plain, grid, REL)))


@pytest.mark.parametrize("name", ["D25", "D40", "B cut"])
def test_mirror_runs_are_the_references(oracle, name):
    """The recurrence over the MIRROR's runs gives the reference's spectrum: the grouping, the
    slots and the bins are right, and a kRunCut cut changes nothing."""
    if name == "B cut":
        whole = cases.case("B")
        table, grid = whole.table.subset(np.arange(whole.table.num_lines) < 2000), whole.grid
        # (the grid reaches far beyond a cut table: still inside the range rule)
    else:
        table, grid = cases.case(name).table, cases.case(name).grid
    for level in LEVELS:
        runs = cases.mirror(table, cases.LEVEL_P[level], grid)
        k, k_plain = cases.replay(oracle, table, level, grid, runs)
        k_ref, _ = oracle.absorption_port(table, cases.LEVEL_T[level], cases.LEVEL_P[level],
                                          cases.LEVEL_X[level], grid.v0, grid.vn, grid.n_per_v,
                                          cut_off=grid.cut_off, remove_pedestal=True)
        worst = _spectrum_error(k, k_ref, k_plain, grid)
        assert worst <= 1., f"{name} level {level}: {worst:.3g} x the pedestal tolerance"


@pytest.mark.parametrize("name", cases.MANY_TRIPS)
def test_late_runs_are_visible(oracle, name):
    """On the points inside the windows of the runs from index 65 535 on the pedestals are at least
    1e-3 of the plain spectrum: a pre-pass that dropped them cannot meet the 1e-6 bar."""
    runs = cases.runs_of(name, cases.TOP)
    grid = cases.case(name).grid
    inside = np.zeros((grid.vn - grid.v0)*grid.n_per_v, bool)
    for head in runs.row_begin[cases.GRID_X:]:
        inside[runs.first[head]:runs.last[head] + 1] = True
    assert inside.any()
    k_ref = cases.reference(oracle, name, cases.TOP)
    k_plain = cases.reference(oracle, name, cases.TOP, remove_pedestal=False)
    assert np.max((k_plain - k_ref)[inside])/np.max(k_plain[inside]) >= 1.e-3


@pytest.mark.parametrize("name", cases.NAMES)
def test_no_case_needs_the_conditioning_allowance(oracle, name):
    """CONDITIONING_MARGIN x the reference's own movement under a one-ulp change of the line
    strengths stays below the plain tolerance at every point: the GPU tests pass no
    `conditioning=`."""
    case = cases.case(name)
    grid = case.grid
    for level in LEVELS:
        k_ref = cases.reference(oracle, name, level)
        k_plain = cases.reference(oracle, name, level, remove_pedestal=False)
        assert np.isfinite(k_ref).all() and np.isfinite(k_plain).all()
        moved = oracle_conditioning(oracle, case.table, cases.LEVEL_T[level], cases.LEVEL_P[level],
                                    cases.LEVEL_X[level], grid.v0, grid.vn, grid.n_per_v,
                                    grid.cut_off, k_ref)
        ratio = float(np.max(CONDITIONING_MARGIN*moved/cases.plain_tolerance(k_ref, k_plain, grid, REL)))
        assert ratio < 1., f"{name} level {level}: {ratio:.3g}"

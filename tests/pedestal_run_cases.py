"""Line tables that give the pedestal pre-pass (csrc/pedestal.h) more runs than one launch row
takes and stand on its fixed cuts, with a numpy mirror of the run bookkeeping of
csrc/pedestal_runs.h (opens_run, run_find_kernel, RunMeta) and csrc/pedestal_chain.h
(run_links_kernel's `displaced` and `too_long`, run_solve_kernel's stretch cut).

tests/test_pedestal_run_cases_host.py proves on the CPU that every case is what
tests/test_gpu_pedestal_many_runs.py takes it for, and holds the cuts restated here against the
headers' text, so a changed cut fails there and does not silently move the cases.

Every table is ascending in nu and holds K lines per integer wavenumber N, at N + eps with eps
spread over (0.0005, 0.0035), delta_air alternating between -0.009 and +0.001 from row to row: at
101 325 Pa successive rows fall alternately into the windows of N - 1 and N and every row opens a
run; at 10 Pa nothing alternates and a window is one run (plus the kRunCut cuts)."""
from collections import namedtuple
from pathlib import Path
import re

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pylbl_amd" / "csrc"
PA_TO_ATM = 9.86923e-6          # spectra.c:17, LevelScalars::p_atm


def constant(text, name):
    """An integer constant of a header: a literal, or `1 << n`."""
    value = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text).group(1)
    base, _, shift = value.partition("<<")
    return int(base.strip(), 0) << (int(shift.strip(), 0) if shift else 0)


def header_constants():
    """The cuts as the headers spell them; GRID_X is the row length of the run_sums_kernel and
    run_links_kernel launches (both must name the same one)."""
    pedestal = (CSRC / "pedestal.h").read_text()
    chain = (CSRC / "pedestal_chain.h").read_text()
    rows = {}
    for kernel in ("run_sums_kernel", "run_links_kernel"):
        rows[kernel] = [int(x) for x in re.findall(
            r"hipLaunchKernelGGL\(%s, dim3\(std::min\(max_runs, (\d+)\), count\)" % kernel, pedestal)]
    return {"GRID_X": rows, "kRunCut": constant(pedestal, "kRunCut"),
            "kMaxStretch": constant(chain, "kMaxStretch"),
            "kMaxHistory": constant(chain, "kMaxHistory"), "chunk": 64}


# The cuts the cases are built on; tests/test_pedestal_run_cases_host.py holds them against
# header_constants().
GRID_X, RUN_CUT, MAX_STRETCH, MAX_HISTORY, CHUNK = 65535, 1024, 1024, 16384, 64

# Margins the cases keep from the cuts (the host test asserts them).
HISTORY_BELOW, HISTORY_ABOVE = 15000, 18000
STRETCH_BELOW, STRETCH_ABOVE = 900, 1100
INTEGER_MARGIN = 1.e-6

Grid = namedtuple("Grid", "v0 vn n_per_v cut_off")
Runs = namedtuple("Runs", "centre first last opens run_count row_begin bin first_slot last_slot "
                          "n_slots prefix begin history stretch displaced too_long stretch_cut "
                          "integer_margin")


def mirror(table, pressure, grid):
    """The runs of one level as run_find_kernel finds them and what run_links_kernel and
    run_solve_kernel's first sweep decide from them."""
    v0, vn, npv, cut = grid
    n, n_cells = (vn - v0)*npv, vn - v0
    n_bins = n_cells + 2*cut + 3
    nu = np.asarray(table.nu, np.float64)
    # (the range rule, absorption.c:80-83: every row of these tables is accepted)
    assert np.all((nu <= vn + cut + 1) & (nu >= v0 - (cut + 1)))
    centre = nu + (pressure*PA_TO_ATM)*np.asarray(table.delta_air, np.float64)   # line_prep.h
    fl = np.floor(centre)
    first = ((fl - cut - v0)*npv).astype(np.int64)
    last = np.minimum(((fl + cut + 1 - v0)*npv).astype(np.int64), n - 1)
    empty = (first >= n)
    first = np.maximum(first, 0)
    empty |= last < first
    first = np.where(empty, 0x3fffffff, first)          # mark_empty
    last = np.where(empty, -0x3fffffff, last)
    r = np.arange(nu.size)
    changed = np.ones(nu.size, bool)
    changed[1:] = (first[1:] != first[:-1]) | (last[1:] != last[:-1])
    opens = ~empty & (changed | (r % RUN_CUT == 0))       # opens_run
    row_begin = np.flatnonzero(opens)
    count = row_begin.size
    bin_ = (fl[row_begin] - (v0 - cut - 1)).astype(np.int64)          # RunMeta::bin
    head_first, head_last = first[row_begin], last[row_begin]
    first_slot = head_first//npv
    last_int = head_last//npv
    extra = last_int*npv != head_last
    last_slot = np.where(extra, n_cells, last_int)
    n_slots = last_int - first_slot + 1 + extra
    prefix = np.maximum.accumulate(np.maximum(bin_, -1)) if count else bin_
    index = np.arange(count)
    bin_ok = (bin_ >= 0) & (bin_ < n_bins)
    displaced = ~bin_ok
    displaced[1:] |= prefix[:-1] > bin_[1:] + 1
    # wave_lower_bound(prefix, 0, r, first_slot): the prefix maxima do not decrease
    begin = np.minimum(np.searchsorted(prefix, first_slot, side="left"), index)
    history = index - begin
    # The first run of a bin against 1 + the last run of it (bin_end), run_solve_kernel sweep 0.
    stretch = np.zeros(count, np.int64)
    if count:
        firsts = np.full(n_bins, count, np.int64)
        ends = np.zeros(n_bins, np.int64)
        np.minimum.at(firsts, bin_[bin_ok], index[bin_ok])
        np.maximum.at(ends, bin_[bin_ok], index[bin_ok] + 1)
        is_first = bin_ok & (firsts[np.clip(bin_, 0, n_bins - 1)] == index)
        stretch = np.where(is_first, ends[np.clip(bin_, 0, n_bins - 1)] - index, 0)
    margin = float(np.min(np.abs(centre - np.round(centre))))
    return Runs(centre, first, last, opens, count, row_begin, bin_, first_slot, last_slot, n_slots,
                prefix, begin, history, stretch, bool(displaced.any()),
                bool((history > MAX_HISTORY).any()), bool((stretch > MAX_STRETCH).any()), margin)


def falls_back(runs):
    return runs.displaced or runs.too_long or runs.stretch_cut


# ---------------------------------------------------------------------------------------------
# Tables.
def near_integer_table(integers, per_integer, seed, blocks=(), gamma=0.14):
    """K = per_integer lines at every N of `integers` (ascending), alternating shifts.  blocks:
    (N, rows) pairs of extra lines with delta_air = 0 spread over N + (0.1, 0.9): one window at
    every pressure, placed in ascending order behind the lines of N."""
    from pylbl_amd import synthetic
    integers = np.asarray(integers, np.float64)
    eps = 0.0005 + 0.003*(np.arange(per_integer) + 0.5)/per_integer
    nu = (integers[:, None] + eps[None, :]).ravel()
    delta = np.where(np.arange(nu.size) % 2 == 0, -0.009, 0.001)
    for at, rows in blocks:
        extra = at + 0.1 + 0.8*(np.arange(rows) + 0.5)/rows
        where = np.searchsorted(nu, at + 0.1)
        nu = np.concatenate([nu[:where], extra, nu[where:]])
        delta = np.concatenate([delta[:where], np.zeros(rows), delta[where:]])
    assert np.all(np.diff(nu) > 0.)
    table = synthetic.line_table("CO2", float(nu[0]), float(nu[-1]) + 1., num_lines=nu.size,
                                 seed=seed, tips_range=(150, 400))
    table.nu = nu
    table.delta_air = delta
    # Strengths within half a decade and air-broadened widths of gamma .. gamma + 0.04 cm-1/atm
    # (0.14 at cut_off 25, 0.5 at cut_off 150 and 200, where the wings are taken 150 cm-1 out; the drawn
    # columns, rescaled): at 1 atm the pedestals -- the far wings of every line within cut_off --
    # are then 1e-3 and more of the peaks they lie under -- about (2 cut_off + 2) windows x
    # (gamma/cut_off)^2 whatever K is -- where eleven decades of strengths let a few lines hide the
    # rest (tests/test_pedestal_run_cases_host.py asserts the ratio).
    table.sw = 10.**(-21. + (np.log10(table.sw) + 30.)/22.)
    table.gamma_air = gamma + (table.gamma_air - 0.03)*(0.04/0.09)
    return table


# Every call takes three levels: 10 Pa (a window is a run), one in between (a third of the rows
# alternate: its histories and stretches stay clear of the cuts' margins in every case, and
# 16 073 Pa keeps every shifted centre 4e-6 from an integer) and 101 325 Pa (every row opens a run).
LEVEL_T = np.asarray([230., 255., 288.])
LEVEL_P = np.asarray([10., 16073., 101325.])
LEVEL_X = np.asarray([4.e-4, 4.e-4, 4.e-4])
TOP = 2         # the level with the most runs

Case = namedtuple("Case", "name table grid over trips fall_back bits")
# over: the side of GRID_X the 1-atm level's run count lies on (exact: the count itself);
# trips: the trips of the grid-stride loops there; fall_back: per level, which predicates hold
# ("" none: the level stays with the relaxation); bits: per level, what the four variants of
# tests/test_gpu_pedestal_many_runs.py must show (see there): "fixed" the relaxation's verified fixed
# point under `relax default` and `relax 7`, "late" under `relax 7` alone, "same" one spectrum.

_cache = {}


def _dense(integers, per_integer):
    return near_integer_table(np.arange(2300, 2300 + integers), per_integer, seed=integers)


# (the grid ends beyond the last window: hundreds of runs clipped at the last grid point each hold
# the last slot of all the others, a chain of dependences the sweeps do not settle)
DENSE_GRID = Grid(2290, 2580, 2, 25)


WIDE_GRID = Grid(2290, 3870, 1, 150)
# B and its cuts: the 16 073 Pa level settles; at 1 atm a bin's runs span nine chunks, more chunk
# boundaries than seven sweeps cover, and the serial chain takes the level behind the sweeps.
DENSE_BITS = ("same", "fixed", "same")


def _cut_to_runs(table, grid, wanted):
    """The first rows of the table that hold exactly `wanted` runs at the 1-atm level."""
    opens = mirror(table, LEVEL_P[TOP], grid).opens
    rows = int(np.searchsorted(np.cumsum(opens), wanted, side="right"))
    return table.subset(np.arange(table.num_lines) < rows)


def _d_table():
    # rows 0 .. 299: 15 integers x 20; 300 .. 3399: one window (2315), cut at 1024, 2048, 3072;
    # 3400 .. 4095: 24 integers x 29; 4096 .. 5120: one window (2340) that begins on a multiple
    # of kRunCut; row 5120 is the cut's, the last run, one row.
    head = near_integer_table(np.arange(2300, 2315), 20, seed=71, blocks=[(2315, 3100)])
    tail = near_integer_table(np.arange(2316, 2340), 29, seed=72, blocks=[(2340, 1025)])
    for name in ("nu", "sw", "gamma_air", "gamma_self", "n_air", "elower", "delta_air",
                 "local_iso_id"):
        setattr(head, name, np.concatenate([getattr(head, name), getattr(tail, name)]))
    assert np.all(np.diff(head.nu) > 0.) and head.num_lines == 5*RUN_CUT + 1
    return head


def case(name):
    if name in _cache:
        return _cache[name]
    none = ("", "", "")
    if name == "A":
        # wide, many windows: 22 000 integers x 4 lines, three runs to the integer at 1 atm
        made = Case(name, near_integer_table(np.arange(2, 22002), 4, seed=61),
                    Grid(1, 22004, 1, 25), ">", 2, none, ("same", "same", "fixed"))
    elif name == "B":
        # dense, few windows: history walks of ~14 600 runs, no predicate holds (the sweeps run in
        # full; at 1 atm they do not settle, and the chain takes the level behind them)
        made = Case(name, _dense(250, 276), DENSE_GRID, ">", 2, none, DENSE_BITS)
    elif name == "B65535":
        made = Case(name, _cut_to_runs(case("B").table, DENSE_GRID, GRID_X), DENSE_GRID,
                    GRID_X, 1, none, DENSE_BITS)
    elif name == "B65536":
        made = Case(name, _cut_to_runs(case("B").table, DENSE_GRID, GRID_X + 1), DENSE_GRID,
                    GRID_X + 1, 2, none, DENSE_BITS)
    elif name == "C1":
        # more than 2 x 65 535 runs: three trips; too_long (the stretch cut holds as well)
        made = Case(name, _dense(230, 600), DENSE_GRID, ">>", 3,
                    ("", "", "too_long stretch_cut"), ("same", "same", "same"))
    elif name == "C1'":
        made = Case(name, _dense(230, 400), DENSE_GRID, ">", 2, ("", "", "too_long"),
                    ("same", "late", "same"))
    elif name == "C2":
        made = Case(name, near_integer_table(np.arange(2300, 2340), 600, seed=62),
                    Grid(2298, 2342, 2, 3), "<", 1, ("", "", "stretch_cut"),
                    ("same", "same", "same"))
    elif name == "E":
        # dense AND settling: the history of B from many bins (cut_off 150: 302 bins hold a slot)
        # instead of many runs to the bin -- 47 runs to the integer, a bin's runs within two chunks,
        # so the chains of dependences that matter cross a boundary or two and the sweeps verify
        made = Case(name, near_integer_table(np.arange(2300, 3710), 48, seed=63, gamma=0.5),
                    WIDE_GRID, ">", 2, none, ("same", "fixed", "fixed"))
    elif name == "E65535":
        made = Case(name, _cut_to_runs(case("E").table, WIDE_GRID, GRID_X), WIDE_GRID,
                    GRID_X, 1, none, ("same", "fixed", "fixed"))
    elif name == "E65536":
        made = Case(name, _cut_to_runs(case("E").table, WIDE_GRID, GRID_X + 1), WIDE_GRID,
                    GRID_X + 1, 2, none, ("same", "fixed", "fixed"))
    elif name == "F":
        # too_long alone on a level that would settle: 402 bins x 47 runs of history, stretch ~95
        made = Case(name, near_integer_table(np.arange(2300, 2760), 48, seed=64, gamma=0.5),
                    Grid(2290, 2970, 1, 200), "<", 1, ("", "", "too_long"),
                    ("same", "fixed", "same"))
    elif name == "F40":
        # F cut to its first 16 385 + 40 runs at 1 atm: every run up to 16 385 looks back to run 0,
        # so exactly 40 runs are too_long, all of them in the last chunk or two.  Without the
        # hand-over such a level verifies a fixed point whose last runs lack gs and ge.
        made = Case(name, _cut_to_runs(case("F").table, case("F").grid, MAX_HISTORY + 1 + 40),
                    case("F").grid, "<", 1, ("", "", "too_long"), ("same", "fixed", "same"))
    elif name in ("D25", "D40"):
        made = Case(name, _d_table(), Grid(2255, 2385, 4, int(name[1:])), "<", 1, none,
                    ("same", "same", "fixed") if name == "D25" else ("same", "fixed", "fixed"))
    else:
        raise KeyError(name)
    _cache[name] = made
    return made


NAMES = ("A", "B", "B65535", "B65536", "C1", "C1'", "C2", "D25", "D40", "E", "E65535",
         "E65536", "F", "F40")
MANY_TRIPS = ("A", "B", "B65536", "C1", "C1'", "E", "E65536")      # more than one trip at 1 atm
# F40 stands ON the kMaxHistory cut: in place of the history margin the host test counts its
# too_long runs (the mirror is exact in integers, given the centres' distance from integers).
ON_THE_HISTORY_CUT = {"F40": 40}
_runs = {}


def runs_of(name, level):
    if (name, level) not in _runs:
        c = case(name)
        _runs[name, level] = mirror(c.table, LEVEL_P[level], c.grid)
    return _runs[name, level]


# ---------------------------------------------------------------------------------------------
# The comparison's tolerance, as tests/test_gpu_parity.py::assert_spectrum forms it.
def plain_tolerance(k_ref, k_plain, grid, rel):
    from tests import golden_io
    tol = golden_io.pedestal_tolerance(k_ref, grid.n_per_v, grid.cut_off, rel)
    tol = np.maximum(tol, rel*np.abs(k_plain))
    return np.maximum(tol, golden_io.pedestal_tolerance(k_plain, grid.n_per_v, grid.cut_off,
                                                        1.e-13)) + 1e-300


_references = {}


def reference(oracle, name, level, remove_pedestal=True):
    """oracle.absorption_port of a case's level, computed once and handed out read-only."""
    key = (name, level, remove_pedestal)
    if key not in _references:
        c = case(name)
        k, _ = oracle.absorption_port(c.table, LEVEL_T[level], LEVEL_P[level], LEVEL_X[level],
                                      c.grid.v0, c.grid.vn, c.grid.n_per_v,
                                      cut_off=c.grid.cut_off, remove_pedestal=remove_pedestal)
        k.setflags(write=False)
        _references[key] = k
    return _references[key]


def replay(oracle, table, level, grid, runs):
    """The factorisation of pedestal.h's header comment in float64 on the mirror's runs: every
    run's profile sums on its slots (oracle.voigt_port), P = min(a_s + VS, a_e + VE), every
    interior slot + sums - P; then the plain spectrum minus the runs' pedestals on their windows."""
    v0, vn, npv, cut = grid
    n, n_cells = (vn - v0)*npv, vn - v0
    k_plain, extras = oracle.absorption_port(table, LEVEL_T[level], LEVEL_P[level], LEVEL_X[level],
                                             v0, vn, npv, cut_off=cut, want_derived=True)
    derived = extras["derived"]
    assert np.array_equal(derived[:, 0], runs.centre)
    assert np.array_equal(derived[:, 4], runs.first) and np.array_equal(derived[:, 5], runs.last)
    a = np.zeros(n_cells + 1)
    windows = {}
    ends = np.append(runs.row_begin[1:], table.num_lines)
    for q in range(runs.run_count):
        slots = np.arange(runs.first_slot[q], runs.first_slot[q] + runs.n_slots[q])
        slots[-1] = runs.last_slot[q]
        points = np.where(slots < n_cells, slots*npv, n - 1)
        at = v0 + points*(1./npv)
        sums = np.zeros(slots.size)
        for row in range(runs.row_begin[q], ends[q]):
            assert runs.first[row] == runs.first[runs.row_begin[q]]
            assert runs.last[row] == runs.last[runs.row_begin[q]]
            oracle.voigt_port(at, 0, slots.size - 1, derived[row, 0], derived[row, 1],
                              derived[row, 2], derived[row, 3], k=sums)
        k_s, k_e = a[slots[0]] + sums[0], a[slots[-1]] + sums[-1]
        pedestal = k_s if slots.size == 1 or not k_s - k_e > 0. else k_e
        a[slots] += sums - pedestal
        a[slots[-1]] = max(k_e - k_s, 0.)
        a[slots[0]] = max(k_s - k_e, 0.) if slots.size > 1 else 0.
        head = runs.row_begin[q]
        window = (int(runs.first[head]), int(runs.last[head]))
        windows[window] = windows.get(window, 0.) + pedestal
    total = np.zeros(n)         # (window by window: exactly zero where no window reaches)
    for (first, last), pedestal in windows.items():
        total[first:last + 1] += pedestal
    return k_plain - total, k_plain

"""The case tables of tests/many_paths_cases.py, on the CPU: that the pattern of seven paths can
tell one launch chunk from the next, that it reaches both sides of the entries' branches, that its
inputs are ones the numpy mirrors stay inside, and why these have to be entry-level tests.

Every path entry goes through PathCall::launch (csrc/path_entry.inc), one launch per kPathGridY =
65535 paths of a run, and its band means through PathBands::means, one chunk of 65535 rows after
another.  Before tests/test_gpu_many_paths.py no test reached the later chunks of either loop:
Spectroscopy cuts a run at 65535 levels (paths._cut_runs), so a run of its calls touches at most
65535 paths and 65535 rows of means and is one launch and one chunk, whatever the atmosphere's
size; and the entry-level files all ran sweep_cases.PATHS = 3 paths."""
import re
from pathlib import Path

import numpy as np
import pytest

from pylbl_amd import paths
from tests import many_paths_cases as many
from tests import scatterer_cases as sc
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as rc
from tests import thermal_source_cases as tsc
from tests import two_stream_cases as ts

F64 = np.float64
CSRC = Path(__file__).resolve().parent.parent/"pylbl_amd"/"csrc"
LATER = many.GRID_Y % many.P        # the pattern path of path 65535

ALL_PATTERNS = {
    "sweep": many.sweep_pattern,
    "shortwave": lambda: many.shortwave_pattern(False),
    "shortwave spectral": lambda: many.shortwave_pattern(True),
    "longwave": lambda: many.longwave_pattern("isothermal"),
    "longwave linear": lambda: many.longwave_pattern("linear"),
    "longwave spectral": lambda: many.longwave_pattern("spectral"),
}


def test_the_constants_are_the_kernels():
    text = (CSRC/"path.h").read_text()
    found = re.search(r"kPathGridY\s*=\s*(\d+)", text)
    assert found and int(found.group(1)) == many.GRID_Y == paths._MAX_RUN_LEVELS
    assert many.GRID_Y == 3*5*17*257


def test_the_period_does_not_divide_a_launch():
    assert many.GRID_Y % many.P != 0 and LATER == 1
    # The period of the other entry-level files does: it cannot see a chunk's offset go missing.
    assert many.GRID_Y % cases.PATHS == 0
    # Nor does it divide two launches, or a launch less the two paths a run may skip.
    assert (2*many.GRID_Y) % many.P != 0 and (many.GRID_Y + 2) % many.P != 0
    assert many.N2 == many.GRID_Y + 7 and many.N3 == 2*many.GRID_Y + 3
    assert many.launches(many.N2) == 2 and many.launches(many.N3) == 3
    assert many.launches(many.N2 - 2) == 2
    # Per-level means: three chunks at N2, five at N3; per-path means: two chunks at N2.
    assert many.mean_chunks(many.LEVELS*many.N2) == 3
    assert many.mean_chunks(many.LEVELS*many.N3) == 5
    assert many.mean_chunks(many.N2) == 2 and many.mean_chunks(many.N2 - 2) == 2
    assert many.LEVELS == 2 and many.COLUMNS == 5
    assert cases.lane_widths(many.COLUMNS) == {1, 2}
    assert many.COLUMNS <= cases.PATH_THREADS*cases.PATH_WIDTH      # one workgroup in x
    assert cases.layout_is_vector("aligned", many.COLUMNS)
    assert not cases.layout_is_vector("odd", many.COLUMNS)
    assert tuple(many.BANDS) == (0, 2, 2, 5) and many.BANDS[-1] == many.COLUMNS


def test_tiles_repeat_the_pattern():
    values = np.arange(many.P*many.LEVELS*3).reshape(many.P*many.LEVELS, 3)
    tiled = many.tile_levels(values, many.N2)
    assert tiled.shape == (many.N2*many.LEVELS, 3)
    for p in (0, 1, 6, 7, many.GRID_Y - 1, many.GRID_Y, many.N2 - 1):
        rows = slice(p*many.LEVELS, (p + 1)*many.LEVELS)
        at = (p % many.P)*many.LEVELS
        assert np.array_equal(tiled[rows], values[at:at + many.LEVELS])
    assert np.array_equal(many.tile_levels(values, many.N2, 2), tiled[2*many.LEVELS:])
    per_path = many.tile_paths(values[:many.P], many.N2)
    assert np.array_equal(per_path[many.GRID_Y], values[LATER])
    assert not np.array_equal(per_path[many.GRID_Y], per_path[0])
    parts = [np.full((3, 2), i) for i in range(3)]
    assert many.part_paths(parts)[:, 0].tolist() == [0, 0, 0, 1, 1, 1, 2]
    parts = [np.full((3*many.LEVELS, 2), i) for i in range(3)]
    assert many.part_levels(parts)[:, 0].tolist() == [0]*6 + [1]*6 + [2]*2


@pytest.mark.parametrize("name", sorted(ALL_PATTERNS))
def test_the_pattern_is_distinct_table_by_table(name):
    pattern = ALL_PATTERNS[name]()
    per_path, per_level = pattern.per_path_tables(), pattern.per_level_tables()
    assert per_path and "beta" in per_level
    for table, values in per_path.items():
        assert values.shape[0] == many.P, table
        assert many.pairwise_distinct(values), (name, table)
        # What the first path of the second launch, and row 65535 of the run's tables, must not
        # be taken for: the pattern path of path 0 -- and path 2's run starts at path 2.
        assert not np.array_equal(values[LATER], values[0]), (name, table)
        assert not np.array_equal(values[(2 + many.GRID_Y) % many.P], values[2]), (name, table)
    for table, values in per_level.items():
        assert values.shape[0] == many.P*many.LEVELS, table
        assert many.levels_distinct(values), (name, table)
        # Per-level tables are read at the level's row in the run: row 2*65535 is pattern path
        # LATER's.
        level_rows = values.reshape(many.P, many.LEVELS, -1)
        assert not np.array_equal(level_rows[LATER], level_rows[0]), (name, table)
    if per_path.get("mu0") is not None:
        assert np.all((per_path["mu0"] > 0.) & (per_path["mu0"] <= 1.))


def test_the_sweeps_pattern_reaches_the_branches():
    pattern = many.sweep_pattern()
    # Paths with and without a boundary, eps = 1, inside (0, 1) and 0; the same at the surface.
    assert pattern.boundary_t[0] == 0. and np.all(pattern.boundary_t[1:] > 0.)
    assert np.all(pattern.jacobian_t > 0.)
    for eps in (pattern.boundary_e, pattern.surface_e, pattern.albedo):
        assert np.any(eps == 1.) and np.any(eps == 0.) and np.any((eps > 0.) & (eps < 1.))
    for rows in (pattern.e_rows, pattern.albedo_rows):
        assert np.any(np.all(rows == 1., axis=1)) and np.any(rows == 0.)
        assert np.any((rows > 0.) & (rows < 1.))
    assert np.all(pattern.d_rows > 0.)
    # One level without thickness, one without a view length, beta with zeros.
    assert np.count_nonzero(pattern.thickness == 0.) == 1
    assert np.count_nonzero(pattern.view_lengths == 0.) == 1
    assert np.any(pattern.beta == 0.) and np.all(pattern.beta >= 0.)
    # Three knots inside the grid, points on both sides of all of them.
    assert pattern.knots.size == many.KNOTS == 3 and np.all(np.diff(pattern.knots) > 0.)
    assert pattern.nu[0] < pattern.knots[0] and pattern.knots[-1] < pattern.nu[-1]
    assert np.all((pattern.knot_values >= 0.) & (pattern.knot_values <= 1.))
    # The two rows-in-flight classes of path_flux_kernel.
    assert cases.flux_ahead(1) != cases.flux_ahead(5)
    for angles in (1, 5):
        lengths, weight = pattern.flux_lengths(angles)
        assert lengths.shape == (many.P*many.LEVELS, angles) and weight.shape == (angles,)
        assert many.levels_distinct(lengths)
    # Edge temperatures are continuous inside every path.
    edges = pattern.edges.reshape(many.P, many.LEVELS, 2)
    assert np.array_equal(edges[:, :-1, 1], edges[:, 1:, 0])


def test_the_runs_put_paths_on_both_sides_of_a_launch():
    for n_paths in (many.N2, many.N3):
        levels = n_paths*many.LEVELS
        sets = many.run_sets(n_paths, True)
        assert sets["whole"] == [(0, levels)]
        (first, count), = sets["from path 2"]
        assert first == 2*many.LEVELS and first + count == levels
        assert many.first_path_of(sets["from path 2"]) == 2
        assert many.launches(n_paths - 2) >= 2
        before, middle, after = sets["inside paths"]
        assert before == (0, 1) and after == (levels - 1, 1)
        assert middle == (1, levels - 2)
        for from_last in (False, True):
            lanes = cases.path_lanes(middle[0], middle[1], many.LEVELS, from_last)
            assert len(lanes) == n_paths and many.launches(len(lanes)) >= 2
            # A partial path at either end (one starts, one finishes), whole paths between them,
            # across the launch edge.
            assert (lanes[0].n, lanes[-1].n) == (1, 1)
            assert (lanes[0].starts, lanes[0].finishes) == (False, True) if not from_last \
                else (lanes[0].starts, lanes[0].finishes) == (True, False)
            assert lanes[0].starts != lanes[-1].starts
            inner = lanes[many.GRID_Y - 1:many.GRID_Y + 1]
            assert all(x.n == many.LEVELS and x.starts and x.finishes for x in inner)
        cut = many.cut_at_the_launch_edge(n_paths)
        assert cut[0] == (0, many.GRID_Y*many.LEVELS) and sum(c for _, c in cut) == levels
    assert "inside paths" not in many.run_sets(many.N2, False)


def test_the_shortwave_patterns_reach_the_branches_and_stay_inside_the_mirror():
    for spectral in (False, True):
        pattern = many.shortwave_pattern(spectral)
        branches = pattern.branches()
        assert np.any(branches == ts.CONSERVATIVE_BRANCH) and np.any(branches == ts.GENERAL)
        assert np.any(pattern.albedo == 1.) and np.any(pattern.albedo == 0.)
        assert np.any((pattern.albedo > 0.) & (pattern.albedo < 1.))
        assert np.any(pattern.solar == 0.) and np.any(pattern.sigma == 0.)
        bound = sc.E_CPU_SHORTWAVE if spectral else ts.E_CPU
        for from_last in (False, True):
            for rows in (False, True):
                for worst, finite in pattern.worst_error(from_last, rows):
                    print("shortwave, spectral %s: worst error %.3g (E_cpu %.3g)"
                          % (spectral, worst, bound))
                    assert finite and worst <= bound
    spectral = many.shortwave_pattern(True)
    assert spectral.knots.size == many.KNOTS
    assert np.all(spectral.table[:, 2:] == 0.) and np.any(sc.scatters(spectral.optics))


@pytest.mark.parametrize("source", ["isothermal", "linear", "spectral"])
def test_the_longwave_patterns_reach_the_branches_and_stay_inside_the_mirror(source):
    pattern = many.longwave_pattern(source)
    branches = pattern.branches()
    for branch in (tc.CLEAR, tc.CONSERVATIVE_BRANCH, tc.GENERAL):
        assert np.any(branches == branch), branch
    if source == "spectral":
        scatters = sc.scatters(pattern.optics)
        assert np.any(scatters) and not np.all(scatters)
        assert np.all(pattern.table[:, 1:4] == 0.)
        bound = sc.E_CPU_LONGWAVE
    else:
        cloudy = pattern.table[:, 2] > 0.
        assert np.any(cloudy) and not np.all(cloudy)
        assert np.any(pattern.table[cloudy, 2] == pattern.table[cloudy, 1])     # omega_c = 1
        bound = tsc.E_CPU if source == "linear" else tc.E_CPU
    eps = pattern.emissivity
    assert np.any(eps == 1.) and np.any(eps == 0.) and np.any((eps > 0.) & (eps < 1.))
    sources = {"isothermal": (False,), "linear": (True,), "spectral": (False, True)}[source]
    for linear_source in sources:
        for from_last in (False, True):
            for rows in (False, True):
                for worst, finite in pattern.worst_error(from_last, rows, linear_source):
                    print("longwave %s: worst error %.3g (E_cpu %.3g)" % (source, worst, bound))
                    assert finite and worst <= bound
    if source != "isothermal":
        edges = pattern.edges.reshape(many.P, many.LEVELS, 2)
        assert np.array_equal(edges[:, :-1, 1], edges[:, 1:, 0])


def test_the_view_pattern_reaches_the_branches_and_stays_inside_the_mirror():
    pattern = many.longwave_pattern("isothermal")
    # mu and eps: thermal_radiance_cases.MU and thermal_cases.EMISSIVITY, and four more of each.
    assert tuple(pattern.view_mu[:3]) == rc.MU and tuple(pattern.emissivity[:3]) == tc.EMISSIVITY
    assert np.all((pattern.view_mu > 0.) & (pattern.view_mu <= 1.))
    for inputs in pattern.parts:
        li = inputs.layer_inputs(False)
        positive, series, _ = rc.decisions(li, inputs.view_mu[None, :, None])
        cloudy = li["branch"] != tc.CLEAR
        assert np.any(cloudy) and not np.all(cloudy)
    for from_last in (False, True):
        for worst, finite in pattern.view_worst_error(from_last):
            print("view: worst error %.3g (E_cpu %.3g)" % (worst, rc.E_CPU))
            assert finite and worst <= rc.E_CPU
        fluxes = pattern.flux_rows(from_last)
        assert fluxes["up"].shape == (many.P*many.LEVELS, many.COLUMNS)
        assert many.levels_distinct(fluxes["up"]) and many.levels_distinct(fluxes["down"])


# ---------------------------------------------------------------------------------------------
# Why entry-level tests: Spectroscopy never gives a run more than one launch.
@pytest.mark.parametrize("whole_paths", [False, True])
@pytest.mark.parametrize("per_path", [1, 2, 64])
def test_no_run_of_spectroscopy_touches_more_paths_than_one_launch(per_path, whole_paths):
    limit = 1 << 62
    for n_paths in (1, 1000, many.GRID_Y, many.GRID_Y + 1, 70000, many.N3):
        levels = n_paths*per_path
        run, runs = paths._cut_runs(levels, per_path, 8, limit, whole_paths)
        assert run <= many.GRID_Y
        assert runs[0][0] == 0 and runs[-1][1] == levels
        assert all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
        for begin, end in runs:
            assert 0 < end - begin <= many.GRID_Y           # rows of per-level means: one chunk
            touched = (end - 1)//per_path - begin//per_path + 1
            assert touched <= many.GRID_Y                    # PathCall::launch: one launch
            assert touched <= (many.GRID_Y + per_path - 2)//per_path + 1
            if whole_paths:
                assert begin % per_path == 0 and end % per_path == 0
    # The largest run there is: 65535 levels, of 32768 paths of two levels at the most.
    _, runs = paths._cut_runs(2*70000, 2, 8, limit, False)
    most = max((end - 1)//2 - begin//2 + 1 for begin, end in runs)
    assert most <= 32769 and many.launches(most) == 1 and len(runs) > 1

"""CPU checks behind tests/test_gpu_slot_shapes.py: through the mirrors of tests/slot_cases.py every
case reaches the route of csrc/xsec.h or csrc/continuum.h it is named for, for both
instantiations; the mirrors restate the headers' constants and decisions as the headers spell
them; and the oracles are finite on every case and exactly 0 outside the bands."""
from pathlib import Path
import re

import numpy as np
import pytest

from tests import slot_cases as cases

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pylbl_amd" / "csrc"
INSTANCES = list(cases.INSTANCES.values())


def constant(text, name):
    return re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text).group(1).strip()


def test_mirrors_restate_the_headers():
    """The constants, and the three decisions the mirrors restate, as the kernels spell them: a
    change of `<=` into `<` or of the staged range moves no value (both routes read the same
    frequencies) but moves the boundary these cases stand on."""
    xsec, continuum = (CSRC / "xsec.h").read_text(), (CSRC / "continuum.h").read_text()
    entry = (CSRC / "xsec_entry.inc").read_text() + (CSRC / "continuum_entry.inc").read_text()
    slot = (CSRC / "slot_entry.inc").read_text()
    assert int(constant(xsec, "kXsecStage")) == cases.XSEC_STAGE
    assert int(constant(xsec, "kMaxXsecBands")) == cases.XSEC_MAX_BANDS == max(cases.COUNTS)
    assert int(constant(xsec, "kModelThreads")) == cases.MODEL_THREADS
    assert float(constant(xsec, "kSpeedOfLight")) == cases.SPEED_OF_LIGHT
    for statement in ("const int base = max(w0 - 1, 0);", "const int length = w1 - base;",
                      "const bool in_lds = length <= kXsecStage;",
                      "const bool touches = x_hi >= f[0] && x_lo <= f[b.size - 1];",
                      "const long long block_first = (long long)blockIdx.x*(256*PT);"):
        assert statement in xsec, statement
    for statement in ("if (j_lo == last || run.hi < next_knot)",
                      "if (run.hi < b.lower || run.lo > x_last) return false;",
                      "if (run.lo >= b.lower && run.hi <= x_last)",
                      "run.usable = form.arithmetic != 0 && form.step > 0. && last < n;",
                      "const long long last = first + 64*G - 1;"):
        assert statement in continuum, statement
    assert "xsec_interp_kernel<4, 1>" in entry and "xsec_interp_kernel<2, 4>" in entry
    assert "if (count == 1) LBL_INTERP(4, 1); else LBL_INTERP(2, 4);" in entry
    # (per run of levels since the group call cuts them into runs of 65535 itself)
    assert "if (count == 1) LBL_GROUP_INTERP(4, 1); else LBL_GROUP_INTERP(4, 2);" in entry
    assert "std::min<long long>(n_levels, 65535)" in slot
    assert "const long long chunk = std::min<long long>(n_levels, 65535);" in entry
    assert [(i.points, i.run) for i in INSTANCES] == [(256*i.pt, 64*i.pt) for i in INSTANCES]


def test_mirror_on_known_answers():
    f = cases.hz(np.arange(100., 200., 1.))
    bands = [(f, np.zeros((4, f.size)))]
    grid = np.arange(90.5, 250., 0.05)
    four = cases.xsec_windows(bands, grid, cases.INSTANCES["4x1"])
    # the first workgroup: 90.5 ... 141.65; below the band, then between knots 41 and 42
    assert four[0][2:] == (True, 0, 42, 0, 42, True)
    # the second: 141.70 ... 192.85
    assert four[1][2:] == (True, 42, 93, 41, 52, True)
    assert four[3].touches is False and four[3].w0 == -1
    shuffled = cases.xsec_windows(bands, grid[::-1], cases.INSTANCES["2x4"])
    assert all(w[2:] == (True, 0, 100, 0, 100, True) for w in shuffled)
    coarse = cases.Coarse(-20., 10., 2003)
    runs = cases.continuum_runs(coarse, np.arange(-40., 0., 10./256), cases.INSTANCES["4x1"])
    assert [r.route for r in runs] == ["skip", "skip", "fast", "fast"]
    assert runs[2].classes == {"first is a knot", "one interval"}


# ---------------------------------------------------------------------------------------------
# Cross-sections.
MOLECULES = [(size, count) for size in cases.SIZES for count in cases.COUNTS]


@pytest.mark.parametrize("size,count", MOLECULES)
def test_molecules_and_their_grids(size, count):
    from oracle import xsec_oracle
    bands = cases.molecule(size, count)
    assert len(bands) == count and bands[0][0].size == size
    for frequency, coefficients in bands:
        assert np.all(np.diff(frequency) > 0.) and coefficients.shape == (4, frequency.size)
        gaps = np.diff(frequency)
        assert frequency.size < 4 or gaps.max() > 1.5*gaps.min()          # uneven
        # the conversion round trip: enough knots have a wavenumber that maps back exactly
        w, ok = cases.exact_knots(frequency)
        assert np.array_equal(cases.hz(w[ok]), frequency[ok])
        assert ok.sum() >= min(8, frequency.size), ok.sum()
    if count >= 2:      # overlap
        assert bands[0][0][0] < bands[1][0][0] < bands[0][0][-1]
    if count >= 3:      # a shared end frequency
        assert bands[2][0][0] == bands[1][0][-1]
    if count >= 15:     # apart; one band sums negative, one has no negative value
        assert bands[5][0][0] > max(b[0][-1] for b in bands[:5])
        for t, p in zip(*cases.levels(5)):
            fit = xsec_oracle.fit(t, p, bands[3][1])
            assert fit.sum() < 0. and (fit > 0.).any()
            assert xsec_oracle.fit(t, p, bands[4][1]).min() > 0.
            assert (xsec_oracle.fit(t, p, bands[0][1]) < 0.).any() or size < 63
    knots = cases.all_knots(bands)
    grid = cases.knots_grid(bands)
    x = cases.hz(grid)
    for frequency, _ in bands:
        w, ok = cases.exact_knots(frequency)
        assert np.isin(frequency[ok], x).all()
        assert np.isin(cases.hz(np.nextafter(w[ok], np.inf)), x).all()
    edges, plan = cases.edges_grid(bands)
    outside = cases.outside_every_band(bands, grid)
    assert outside.any() and (~outside).any()
    for instance in INSTANCES:
        assert grid.size > 2*instance.points
        windows = cases.xsec_windows(bands, grid, instance)
        assert any(w.touches and w.in_lds for w in windows)
        assert count == 1 or any(not w.touches for w in windows)
        # (on the edges grid a workgroup starts on a knot past a band's first: the staged range
        # begins with the extra element in front of the window)
        assert knots.size < 3 or any(w.touches and w.w0 >= 1 and w.base == w.w0 - 1
                                     for w in cases.xsec_windows(bands, edges, instance))
        # the edges grid: workgroup boundaries bit-equal to knots, and one ulp to either side
        x = cases.hz(edges)
        firsts, lasts = set(), set()
        for first, last in cases.boundary_points(edges, instance):
            for index, seen in ((first, firsts), (last, lasts)):
                for name, value in (("on", edges[index]),
                                    ("above", np.nextafter(edges[index], -np.inf)),
                                    ("below", np.nextafter(edges[index], np.inf))):
                    if value in knots:
                        assert name != "on" or any(x[index] in f for f, _ in bands)
                        seen.add(name)
        if len(plan) >= 12:
            assert {"on", "below", "above"} <= firsts & lasts, (instance.name, firsts, lasts)
        else:       # (a molecule of two or three frequencies has as many boundaries)
            assert "on" in firsts | lasts, (instance.name, firsts, lasts)
    for m, variant, knot in plan:
        pair = edges[512*m - 1], edges[512*m]
        assert knot in pair or np.nextafter(knot, -np.inf) in pair or np.nextafter(knot, np.inf) in pair
    # the oracle on these grids: finite, exactly 0 outside the bands
    for points in (grid, edges):
        expect = xsec_oracle.absorption_coefficient(bands, points, 285., 6.e4)
        assert np.isfinite(expect).all() and expect.max() > 0.
        assert np.all(expect[cases.outside_every_band(bands, points)] == 0.)


def test_window_sizes_are_exact():
    band = cases.window_band()
    assert band[0].size == 4097
    for instance in INSTANCES:
        for length in cases.WINDOWS:
            for from_start in (False, True):
                grid = cases.window_grid(band, length, instance, from_start)
                windows = cases.xsec_windows([band], grid, instance)
                first = windows[0]
                assert first.length == length, (instance.name, length, from_start, first)
                assert first.in_lds == (length <= 1024)
                assert (first.w0 == 0) == from_start and first.base == max(first.w0 - 1, 0)
                assert len(windows) == 2 and windows[1].touches     # a partial second workgroup
    staged = {cases.xsec_windows([band], cases.window_grid(band, n, i), i)[0].in_lds
              for n in (1024, 1025) for i in INSTANCES}
    assert staged == {True, False}


def test_tails_and_orders():
    from oracle import xsec_oracle
    bands = cases.molecule(129, 3)
    for n in cases.TAILS:
        grid = cases.tail_grid(bands, n)
        assert grid.size == n and cases.is_ascending(grid)
    # last-workgroup shapes: a full workgroup, one point more, one fewer, pair tails
    for instance in INSTANCES:
        rest = {n % instance.points for n in cases.TAILS}
        assert {0, 1, instance.points - 1} <= rest and {2, 3} <= rest
    grids, permutation = cases.order_grids(bands)
    assert np.array_equal(grids["shuffled"], grids["ascending"][permutation])
    assert not cases.is_ascending(grids["descending"]) and not cases.is_ascending(grids["shuffled"])
    repeated = grids["repeated neighbours"]
    assert cases.is_ascending(repeated) and (np.diff(repeated) == 0.).sum() > 1000
    assert (grids["zero and negative"] < 0.).any() and (grids["zero and negative"] == 0.).sum() == 2
    for name in ("below every band", "above every band"):
        assert cases.outside_every_band(bands, grids[name]).all()
        for instance in INSTANCES:
            assert not any(w.touches for w in cases.xsec_windows(bands, grids[name], instance))
    for name in ("descending", "shuffled"):     # the branch that takes whole bands as windows
        for instance in INSTANCES:
            windows = cases.xsec_windows(bands, grids[name], instance)
            assert all((w.w0, w.w1) == (0, bands[w.band][0].size) for w in windows)
    for name, grid in grids.items():
        expect = xsec_oracle.absorption_coefficient(bands, grid, 285., 6.e4)
        assert np.isfinite(expect).all(), name
        assert np.all(expect[cases.outside_every_band(bands, grid)] == 0.), name


def test_model_bands():
    from oracle import xsec_oracle
    bands = cases.model_bands()
    assert [b[0].size for b in bands[:5]] == list(cases.MODEL_SIZES)
    t, p = 285., 6.e4
    negative, lifted = xsec_oracle.fit(t, p, bands[5][1]), xsec_oracle.fit(t, p, bands[6][1])
    assert negative.sum() < 0. and (negative > 0.).any() and lifted.min() > 0.
    for frequency, coefficients in bands:
        model = xsec_oracle.full_model(t, p, coefficients)
        assert np.isfinite(model).all() and model.min() >= 0.


# ---------------------------------------------------------------------------------------------
# Continua.
@pytest.mark.parametrize("owner", cases.OWNERS)
def test_run_classes_are_reached(owner, continuum_oracle):
    from pylbl_amd import synthetic
    continuum = continuum_oracle.continuum(owner)
    knots = continuum.bands[cases.TARGET_BAND][0]
    coarse = cases.coarse_of(knots)
    assert np.array_equal(coarse.lower + np.arange(coarse.size)*coarse.resolution, knots)
    assert coarse.lower == int(coarse.lower) and coarse.resolution == int(coarse.resolution)
    atmos = synthetic.fixture_atmosphere()
    vmr = {name: values[-1] for name, values in atmos.vmr.items()}
    spectrum = continuum.band_spectra(atmos.t[-1], atmos.p[-1]*0.01, vmr)[cases.TARGET_BAND]
    zeros = cases.zero_knots(knots, spectrum)
    assert zeros.size >= 1
    for instance in INSTANCES:
        grids = cases.run_grids(coarse, instance)
        reached = {name: set() for name in cases.RUN_CLASSES}
        fast_with = set()
        ending_on_zero = False
        for name, grid in grids.items():
            is_arithmetic, start, step = cases.arithmetic(grid)
            assert is_arithmetic == (name != "linspace"), name
            runs = cases.continuum_runs(coarse, grid, instance)
            if name in ("descending", "linspace", "short"):
                assert {r.route for r in runs} == {"points"}, name
                assert name != "descending" or step < 0.
                assert name != "short" or grid.size < 64
                continue
            assert step > 0. and "partial" in runs[-1].classes, name
            for run in runs:
                for c in run.classes:
                    reached[c].add(name)
                if run.route == "fast":
                    fast_with |= run.classes
                if "last is a knot" in run.classes and not "partial" in run.classes:
                    end = grid[run.index*instance.run + instance.run - 1]
                    ending_on_zero = ending_on_zero or end in zeros
            expect = continuum.spectra(atmos.t[-1], atmos.p[-1], vmr, grid)
            assert np.isfinite(expect).all(), name
            below = grid < min(b[0][0] for b in continuum.bands)
            assert np.all(expect[below] == 0.)
        missing = [c for c in cases.RUN_CLASSES if not reached[c]]
        assert not missing, f"{owner} {instance.name}: no run is {missing}"
        assert fast_with >= {"one interval", "first is a knot"}
        assert not fast_with & {"last is a knot", "knot inside", "partial", "outside"}
        # a full run ends on the knot whose value is exactly 0 beside a non-zero one: the value
        # there is the table's, not the interval's line evaluated at its end
        assert ending_on_zero, (owner, instance.name, zeros)
        # where each class is reached, as DESIGN.md lists it
        assert "low ending on knots" in reached["straddles the first knot"]
        assert "high ending on knots" in reached["ends on the last knot"]
        assert "high knots inside" in reached["straddles the last knot"]
        assert "low between knots" in reached["one interval"]

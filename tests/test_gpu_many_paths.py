"""Every path entry fed more paths than one launch takes (Engine.path_* and surface_emissivity on
rows held in torch tensors): 65535 + 7 paths of two levels on five columns, for lbl_path_compute and
lbl_path_thermal_radiance 2*65535 + 3 as well.  PathCall::launch (csrc/path_entry.inc) puts at most
kPathGridY = 65535 paths of a run into a launch and PathBands::means as many rows into a chunk;
Spectroscopy never gives either loop a second trip (tests/test_many_paths_host.py), and the other
entry-level files run three paths.  Here the later launches run: the per-path tables read at
l.p - a.table_path, the per-chunk arithmetic of lbl_surface_emissivity, lbl_path_jacobian's fine
rows and the two-stream entries' up and down sweeps, the means' row offsets, and path_lane's
starts and finishes for runs that begin and end inside a path.

The problems are tests/many_paths_cases.py's: a pattern of seven distinct paths, tiled.  Seven does
not divide 65535, so the first path of a later launch is another pattern path than the first path
of the run, and a value read or written one chunk off is the neighbouring pattern path's.

What each test holds, on the aligned layout (the vector kernels) and the odd one (the scalar
kernels), for the whole block, for whole paths from path 2 on and, where the entry takes
LBL_PATH_CONTINUE, for the levels [1, 2N - 1) between the runs that start and finish them:
every row of every path within the entry's existing bound of the long-double mirror of its pattern
path -- the bounds are the constants of the entry's *_shapes test, imported, and no other; rows of
paths p and p + 7 with identical bits, across the launch edge; band means (bands 0 .. 2, an empty
one, 2 .. 5) within 1e-12 * magnitude as the entry's shapes test forms them, NaN exactly in the
empty band, on per-level rows and per-path rows past 65535; the padding, the rows of paths outside
the run and the inputs untouched; and the run cut at the launch edge into two calls with the bits
of the single call."""
import numpy as np
import pytest

from tests import jacobian_cases as jac
from tests import many_paths_cases as many
from tests import solar_cases as solar
from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import two_stream_cases as ts
from tests.test_gpu_scatterer_shapes import LONGWAVE_BOUND as SPECTRAL_LONGWAVE_BOUND
from tests.test_gpu_scatterer_shapes import SHORTWAVE_BOUND as SPECTRAL_SHORTWAVE_BOUND
from tests.test_gpu_solar_shapes import EXP_BOUND
from tests.test_gpu_solar_shapes import MEAN_BOUND as SOLAR_MEAN_BOUND
from tests.test_gpu_sweep_shapes import (BOUND, TRANS_BOUND, Grid, Rows, block, in_order, ordered,
                                         plain, read, same_bits)
from tests.test_gpu_thermal_radiance_shapes import BOUND as VIEW_BOUND
from tests.test_gpu_thermal_radiance_shapes import BRIGHTNESS_BOUND
from tests.test_gpu_thermal_shapes import FLUX_BOUND as THERMAL_BOUND
from tests.test_gpu_thermal_shapes import MEAN_BOUND
from tests.test_gpu_thermal_source_shapes import FLUX_BOUND as THERMAL_SOURCE_BOUND
from tests.test_gpu_two_stream_shapes import FLUX_BOUND as SHORTWAVE_BOUND

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
SENTINEL = cases.SENTINEL
P, L, C, GRID_Y, BANDS = many.P, many.LEVELS, many.COLUMNS, many.GRID_Y, many.BANDS
N_BANDS = BANDS.size - 1
WORST, LATER = {}, {}       # kernel -> worst error / bound: all rows, rows of the later launches


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    yield default_engine(0)
    for kernel in sorted(WORST):
        print("\nworst error / bound, %s: %.3g, in the later launches: %.3g"
              % (kernel, WORST[kernel], LATER[kernel]))


def run_cases(continues, sizes=(many.N2,)):
    """[(n_paths, run set)]: every run set at N2; a larger size takes the whole block alone."""
    found = [(many.N2, name) for name in many.run_sets(many.N2, continues)]
    return found + [(n, "whole") for n in sizes if n != many.N2]


def parametrised(continues, sizes=(many.N2,)):
    def wrap(test):
        test = pytest.mark.parametrize("n_paths,run_set", run_cases(continues, sizes))(test)
        return pytest.mark.parametrize("layout", many.LAYOUTS)(test)
    return wrap


# ---------------------------------------------------------------------------------------------
# Rows on the GPU.
def rows_in(values, n_paths, layout, per_level=False):
    """A pattern's rows [P or P*L, C] tiled to n_paths paths, NaN in the padding."""
    tiled = many.tile_levels(values, n_paths) if per_level else many.tile_paths(values, n_paths)
    return block(tiled, tiled.shape[0], C, layout, np.nan)


def row_in(values, layout):
    return block(np.asarray(values)[None, :], 1, C, layout, np.nan)


def rows_out(rows, layout):
    return block(None, rows, C, layout, SENTINEL)


def unwritten(what, tensor, values, n_paths, per_level=False):
    tiled = many.tile_levels(values, n_paths) if per_level else many.tile_paths(values, n_paths)
    assert same_bits(read(tensor)[:, :C], tiled), (what, "an input was written")


# ---------------------------------------------------------------------------------------------
# The checks.
class Scope(object):
    """The paths a run set covers: [first_path, n_paths)."""
    def __init__(self, n_paths, runs):
        self.n_paths, self.runs = n_paths, runs
        self.first_path = many.first_path_of(runs)
        self.paths = n_paths - self.first_path
        assert sum(count for _, count in runs) == self.paths*L
        assert many.launches(self.paths) >= 2

    def inside(self, got, rows_per_path, what, untouched=None):
        """The rows of the run's paths; those before them hold the sentinel (or `untouched`)."""
        cut = self.first_path*rows_per_path
        assert got.shape[0] == self.n_paths*rows_per_path, what
        if untouched is None:
            assert np.all(got[:cut] == SENTINEL), (what, "rows of paths outside the run")
        else:
            assert same_bits(got[:cut], untouched[:cut]), (what, "rows of paths outside the run")
        return got[cut:]

    def tiled(self, values, rows_per_path):
        return many.tile_paths(values, self.n_paths, self.first_path, rows_per_path)


def periodic(what, inside, rows_per_path):
    """Paths p and p + P of the run carry identical bits."""
    per_path = np.ascontiguousarray(inside, dtype=F64).view(np.uint64)
    per_path = per_path.reshape(inside.shape[0]//rows_per_path, -1)
    assert per_path.shape[0] > GRID_Y, what
    same = np.all(per_path[P:] == per_path[:-P], axis=1)
    if not np.all(same):
        path = int(np.flatnonzero(~same)[0]) + P
        assert False, (what, "path %d of the run (launch %d, path %d of it) differs from path %d"
                       % (path, path//GRID_Y, path % GRID_Y, path - P))


def within(kernel, what, got, reference, allowed, later_from):
    """|got - reference| <= allowed wherever the reference is a number, NaN exactly where it is
    NaN (empty bands), never inf; at least one number is compared.  Records the worst error /
    bound of all rows and of the rows from `later_from` on."""
    got = np.asarray(got, dtype=F64)
    reference = cases.flushed(np.asarray(reference, dtype=LD))
    allowed = np.broadcast_to(np.asarray(allowed, dtype=LD), reference.shape)
    assert got.shape == reference.shape and got.size > 0, what
    empty = np.isnan(reference)
    assert np.array_equal(np.isnan(got), empty), (what, "NaN not exactly in the empty bands")
    assert not np.any(np.isinf(got)), what
    assert np.count_nonzero(~empty) > 0, what
    error = np.where(empty, LD(0.), np.abs(got.astype(LD) - np.where(empty, LD(0.), reference)))
    scaled = (allowed > 0.) & ~empty
    ratio = np.zeros(reference.shape, dtype=F64)
    ratio[scaled] = (error[scaled]/allowed[scaled]).astype(F64)
    assert 0 < later_from < got.shape[0], what
    WORST[kernel] = max(WORST.get(kernel, 0.), float(ratio.max()))
    LATER[kernel] = max(LATER.get(kernel, 0.), float(ratio[later_from:].max()))
    bad = error > allowed
    if np.any(bad):
        row = int(np.flatnonzero(np.any(bad, axis=1))[0])
        assert False, (what, "row %d of the run" % row, float(ratio.max()),
                       float(np.max(error[~scaled], initial=0.)))


def check(kernel, what, scope, got, rules):
    """rules: {name: (rows per path, rule)} for every key of `got`; a rule is ("bits", pattern
    rows), ("close", pattern reference, pattern magnitude, bound) or ("allowed", pattern
    reference, pattern allowed), each with an optional dict(untouched=whole rows, mean=True)."""
    assert set(got) == set(rules), (what, sorted(set(got) ^ set(rules)))
    for name, (rows_per_path, rule) in rules.items():
        more = rule[-1] if isinstance(rule[-1], dict) else {}
        what_here = (what, name)
        inside = scope.inside(got[name], rows_per_path, what_here, more.get("untouched"))
        periodic(what_here, inside, rows_per_path)
        # Rows of a mean go GRID_Y to a chunk, paths of a sweep GRID_Y to a launch.
        later_from = GRID_Y if more.get("mean") else GRID_Y*rows_per_path
        if rule[0] == "bits":
            assert same_bits(inside, scope.tiled(rule[1], rows_per_path)), what_here
            continue
        reference = scope.tiled(rule[1], rows_per_path)
        if rule[0] == "close":
            allowed = rule[3]*scope.tiled(np.asarray(rule[2], dtype=LD), rows_per_path)
        else:
            allowed = scope.tiled(np.asarray(rule[2], dtype=LD), rows_per_path)
        within(kernel, what_here, inside, reference, allowed, later_from)


def mean_rule(reference, magnitude, bound=BOUND):
    """The means over BANDS of pattern rows and of their magnitudes, as a rule."""
    return ("close", cases.band_means(LD, reference, BANDS),
            cases.band_means(LD, magnitude, BANDS), bound, dict(mean=True))


def check_own_means(kernel, what, scope, rows, mean, rows_per_path, bound):
    """Band means of values >= 0 within bound*|mean| of the long-double means of the rows the call
    itself wrote, NaN exactly in the empty band; outside the run the sentinel; periodic."""
    what = (what, "mean")
    inside = scope.inside(mean, rows_per_path, what)
    periodic(what, inside, rows_per_path)
    expect = cases.band_means(LD, cases.flushed(scope.inside(rows, rows_per_path, what)), BANDS)
    assert np.all(np.isnan(expect[:, 1])) and not np.any(np.isnan(expect[:, [0, 2]]))
    within(kernel + " means", what, inside, expect, bound*np.abs(expect), GRID_Y)


def assert_same(what, got, base):
    assert set(got) == set(base), what
    for key in base:
        assert same_bits(got[key], base[key]), (what, key)


def both_ways(run, n_paths, run_set, continues):
    """(scope, run(runs) of the run set, and for the whole block the same cut at the launch edge
    into two calls, or None)."""
    runs = many.run_sets(n_paths, continues)[run_set]
    scope = Scope(n_paths, runs)
    got = run(runs)
    cut = run(many.cut_at_the_launch_edge(n_paths)) if run_set == "whole" else None
    return scope, got, cut


# ---------------------------------------------------------------------------------------------
# lbl_path_compute.
PATH_VARIANTS = (("per path", False), ("cumulative", False), ("cumulative", True), ("bands", False),
                 ("cumulative bands", False), ("cumulative bands", True))


def run_path(engine, n_paths, layout, runs, mode, from_last):
    pattern = many.sweep_pattern()
    cumulative, with_bands = mode.startswith("cumulative"), mode.endswith("bands")
    levels = n_paths*L
    beta = rows_in(pattern.beta, n_paths, layout, True)
    thickness = many.tile_levels(pattern.thickness, n_paths)
    carry = rows_out(n_paths, layout)
    rows = levels if cumulative else n_paths
    if with_bands:
        tau, trans = plain(rows, N_BANDS), plain(rows, N_BANDS)
    else:
        tau, trans = rows_out(rows, layout), rows_out(rows, layout)
    ordered(engine)
    for first, count in in_order(runs, from_last):
        part = slice(first, first + count)
        engine.path_compute(Rows(beta[part]), C, n_paths, L, first, thickness[part], Rows(carry),
                            optical_depth=Rows(tau[part] if cumulative else tau),
                            transmittance=Rows(trans[part] if cumulative else trans),
                            band_start=BANDS if with_bands else None, cumulative=cumulative,
                            from_last=from_last)
        engine.synchronize()
    if not with_bands:
        unwritten(mode, beta, pattern.beta, n_paths, True)
        return {"tau": read(tau, C), "trans": read(trans, C)}
    out = {"tau mean": read(tau), "trans mean": read(trans)}
    if cumulative:
        assert np.all(np.isnan(read(beta)[:, C:])), "the padding of beta was written"
        out["beta"] = read(beta)[:, :C]
    else:
        unwritten(mode, beta, pattern.beta, n_paths, True)
        out["carry"] = read(carry, C)
    return out


def path_rules(n_paths, mode, from_last):
    pattern, mirror = many.sweep_pattern(), many.path_mirror(from_last)
    cumulative = mode.startswith("cumulative")
    k = L if cumulative else 1
    pick = (lambda x: x) if cumulative else (lambda x: many.finals(x, from_last))
    loop, tau, mag, trans = (pick(mirror[name]) for name in ("loop", "tau", "mag", "trans"))
    if not mode.endswith("bands"):
        return {"tau": (k, ("bits", loop)), "trans": (k, ("close", trans, trans, TRANS_BOUND))}
    rules = {"tau mean": (k, mean_rule(tau, mag)), "trans mean": (k, mean_rule(trans, trans))}
    if cumulative:
        # In place: the rows of paths outside the run still hold beta.
        rules["beta"] = (k, ("bits", loop,
                             dict(untouched=many.tile_levels(pattern.beta, n_paths))))
    else:
        rules["carry"] = (k, ("bits", loop))
    return rules


@parametrised(True, (many.N2, many.N3))
def test_path_compute(engine, layout, n_paths, run_set):
    """Per path, cumulative from the first and from the last level, and both band modes: tau is
    the float64 loop bit for bit, exp(-tau) within 1e-15; 2N rows of per-level means are three
    chunks at N2 and five at N3."""
    for mode, from_last in PATH_VARIANTS:
        what = ("path", n_paths, layout, run_set, mode, from_last)
        scope, got, cut = both_ways(
            lambda runs: run_path(engine, n_paths, layout, runs, mode, from_last), n_paths,
            run_set, True)
        check("path", what, scope, got, path_rules(n_paths, mode, from_last))
        if cut is not None:
            assert_same((what, "cut at the launch edge"), cut, got)


# ---------------------------------------------------------------------------------------------
# lbl_path_radiance_source and lbl_path_radiance_surface.
def variant(**keywords):
    base = dict(from_last=False, cumulative=False, linear=False, rows=False, bands=False)
    assert set(keywords) <= set(base)
    base.update(keywords)
    return base


RADIANCE_VARIANTS = {
    "isothermal, per path": variant(),
    "isothermal, cumulative from the last level": variant(from_last=True, cumulative=True),
    "linear source, cumulative": variant(linear=True, cumulative=True),
    "linear source, per path from the last level": variant(linear=True, from_last=True),
    "emissivity rows and reflection, per path from the last level":
        variant(rows=True, from_last=True),
    "emissivity rows and reflection, linear source, cumulative":
        variant(rows=True, linear=True, cumulative=True),
    "per-path means": variant(bands=True),
    "per-level means from the last level, emissivity rows":
        variant(bands=True, cumulative=True, from_last=True, rows=True),
}


def run_radiance(engine, grid, n_paths, layout, runs, v):
    pattern = many.sweep_pattern()
    levels = n_paths*L
    from_last, cumulative = v["from_last"], v["cumulative"]
    beta = rows_in(pattern.beta, n_paths, layout, True)
    thickness = many.tile_levels(pattern.thickness, n_paths)
    temperature = many.tile_levels(pattern.temperature, n_paths)
    edges = many.tile_levels(pattern.edges, n_paths) if v["linear"] else None
    carry = rows_out(n_paths, layout)
    rows = levels if cumulative else n_paths
    if v["bands"]:
        rad, bt = plain(rows, N_BANDS), None
    else:
        rad, bt = rows_out(rows, layout), rows_out(rows, layout)
    e_rows = rows_in(pattern.e_rows, n_paths, layout) if v["rows"] else None
    d_rows = rows_in(pattern.d_rows, n_paths, layout) if v["rows"] else None
    # A reflecting surface needs a boundary behind every path; without the rows path 0 has none.
    boundary_t = pattern.jacobian_t if v["rows"] else pattern.boundary_t
    ordered(engine)
    for first, count in in_order(runs, from_last):
        part = slice(first, first + count)
        engine.path_radiance(
            Rows(beta[part]), C, grid, n_paths, L, first, thickness[part], temperature[part],
            Rows(carry), boundary_temperature=many.tile_paths(boundary_t, n_paths),
            boundary_emissivity=many.tile_paths(pattern.boundary_e, n_paths),
            radiance=Rows(rad[part] if cumulative else rad),
            brightness_temperature=None if bt is None else Rows(bt[part] if cumulative else bt),
            band_start=BANDS if v["bands"] else None, cumulative=cumulative, from_last=from_last,
            edge_temperature=None if edges is None else edges[part],
            emissivity_rows=None if e_rows is None else Rows(e_rows),
            reflection=None if d_rows is None else Rows(d_rows))
        engine.synchronize()
    if v["rows"]:
        unwritten("emissivity rows", e_rows, pattern.e_rows, n_paths)
        unwritten("reflection", d_rows, pattern.d_rows, n_paths)
    if not v["bands"]:
        unwritten("beta", beta, pattern.beta, n_paths, True)
        return {"rad": read(rad, C), "bt": read(bt, C)}
    out = {"rad mean": read(rad)}
    if cumulative:
        assert np.all(np.isnan(read(beta)[:, C:])), "the padding of beta was written"
        out["beta"] = read(beta)[:, :C]
    else:
        unwritten("beta", beta, pattern.beta, n_paths, True)
        out["carry"] = read(carry, C)
    return out


def radiance_rules(n_paths, v):
    pattern = many.sweep_pattern()
    rad, mag = many.radiance_mirror(v["from_last"], v["linear"], v["rows"])
    k = L if v["cumulative"] else 1
    if not v["cumulative"]:
        rad, mag = many.finals(rad, v["from_last"]), many.finals(mag, v["from_last"])
    if not v["bands"]:
        flushed = cases.flushed(rad)
        return {"rad": (k, ("close", rad, mag, BOUND)),
                "bt": (k, ("close", cases.brightness(LD, pattern.nu, flushed),
                           cases.brightness_magnitude(LD, pattern.nu, flushed, mag), BOUND))}
    rules = {"rad mean": (k, mean_rule(rad, mag))}
    if v["cumulative"]:
        rules["beta"] = (k, ("close", rad, mag, BOUND,
                             dict(untouched=many.tile_levels(pattern.beta, n_paths))))
    else:
        rules["carry"] = (k, ("close", rad, mag, BOUND))
    return rules


@parametrised(True)
def test_path_radiance(engine, layout, n_paths, run_set):
    """The isothermal and the linear-in-tau source, boundaries as scalars (path 0 has none) and
    as emissivity rows with reflection (the surface kernel, a boundary behind every path), both
    directions, per path and per level, and both kinds of means."""
    with Grid(engine, many.sweep_pattern().nu) as grid:
        for name, v in RADIANCE_VARIANTS.items():
            what = ("radiance", n_paths, layout, run_set, name)
            scope, got, cut = both_ways(
                lambda runs: run_radiance(engine, grid, n_paths, layout, runs, v), n_paths,
                run_set, True)
            check("radiance", what, scope, got, radiance_rules(n_paths, v))
            if cut is not None:
                assert_same((what, "cut at the launch edge"), cut, got)


# ---------------------------------------------------------------------------------------------
# lbl_surface_emissivity.
@pytest.mark.parametrize("layout", many.LAYOUTS)
def test_surface_emissivity(engine, layout):
    """path_begin = 2 and N2 - 2 paths of three knots: the second chunk takes its knot values at
    (first_path - path_begin)*n_knots and its rows at first_path*row_stride.  The float64 mirror
    bit for bit, within surface_cases.INTERPOLATION_BOUND of long double."""
    pattern = many.sweep_pattern()
    n_paths, begin = many.N2, 2
    values = many.tile_paths(pattern.knot_values, n_paths, begin)
    assert values.shape == (n_paths - begin, many.KNOTS)
    scope = Scope(n_paths, [(begin*L, (n_paths - begin)*L)])

    def fill(calls):
        rows = rows_out(n_paths, layout)
        ordered(engine)
        for first, count in calls:
            engine.surface_emissivity(grid, Rows(rows), pattern.knots,
                                      values[first - begin:first - begin + count],
                                      path_begin=first)
            engine.synchronize()
        return {"emissivity": read(rows, C)}

    with Grid(engine, pattern.nu) as grid:
        got = fill([(begin, n_paths - begin)])
        what = ("emissivity", layout)
        check("emissivity", what, scope, got,
              {"emissivity": (1, ("allowed", many.emissivity_mirror(LD),
                                  np.full((P, C), surface.INTERPOLATION_BOUND)))})
        check("emissivity", what, scope, got,
              {"emissivity": (1, ("bits", many.emissivity_mirror(F64)))})
        edge = begin + GRID_Y
        assert_same((what, "cut at the launch edge"),
                    fill([(begin, GRID_Y), (edge, n_paths - edge)]), got)


# ---------------------------------------------------------------------------------------------
# lbl_path_jacobian.
def run_jacobian(engine, grid, n_paths, layout, runs, from_last, with_bands):
    pattern = many.sweep_pattern()
    levels = n_paths*L
    beta = rows_in(pattern.beta, n_paths, layout, True)
    thickness = many.tile_levels(pattern.thickness, n_paths)
    temperature = many.tile_levels(pattern.temperature, n_paths)
    outputs = {}
    for q in jac.OUTPUTS:
        rows = levels if q in jac.PER_LEVEL else n_paths
        outputs[q] = plain(rows, N_BANDS) if with_bands else rows_out(rows, layout)
    # With bands: the fine rows of three per-level and three per-path quantities.
    work = rows_out(3*levels + 3*n_paths if with_bands else levels, layout)
    ordered(engine)
    for first, count in runs:
        part = slice(first, first + count)
        given = {q: Rows(outputs[q][part] if q in jac.PER_LEVEL else outputs[q])
                 for q in jac.OUTPUTS}
        engine.path_jacobian(
            Rows(beta[part]), C, grid, n_paths, L, first, thickness[part], temperature[part],
            Rows(work), boundary_temperature=many.tile_paths(pattern.jacobian_t, n_paths),
            boundary_emissivity=many.tile_paths(pattern.boundary_e, n_paths),
            band_start=BANDS if with_bands else None, from_last=from_last, **given)
        engine.synchronize()
    unwritten("beta", beta, pattern.beta, n_paths, True)
    read(work, C)       # its padding
    return {q: read(outputs[q], None if with_bands else C) for q in jac.OUTPUTS}


def jacobian_rules(from_last, with_bands):
    values, magnitudes = many.jacobian_mirror(from_last)
    rules = {}
    for q in jac.OUTPUTS:
        k = L if q in jac.PER_LEVEL else 1
        rules[q] = (k, mean_rule(values[q], magnitudes[q]) if with_bands
                    else ("close", values[q], magnitudes[q], BOUND))
    return rules


@parametrised(False)
def test_path_jacobian(engine, layout, n_paths, run_set):
    """All six fine outputs, and all six band outputs together (per-level and per-path
    quantities: the fine rows of a run's paths lie behind one another in the work block and are
    read back by the means in chunks), both directions."""
    with Grid(engine, many.sweep_pattern().nu) as grid:
        for from_last in (False, True):
            for with_bands in (False, True):
                what = ("jacobian", n_paths, layout, run_set, from_last, with_bands)
                scope, got, cut = both_ways(
                    lambda runs: run_jacobian(engine, grid, n_paths, layout, runs, from_last,
                                              with_bands), n_paths, run_set, False)
                check("jacobian", what, scope, got, jacobian_rules(from_last, with_bands))
                if cut is not None:
                    assert_same((what, "cut at the launch edge"), cut, got)


# ---------------------------------------------------------------------------------------------
# lbl_path_flux: the down sweep, then the up sweep over the same reflection rows.
def run_flux(engine, grid, n_paths, layout, runs, angles, surface_first, with_bands):
    pattern = many.sweep_pattern()
    levels = n_paths*L
    lengths, weight = pattern.flux_lengths(angles)
    lengths = many.tile_levels(lengths, n_paths)
    temperature = many.tile_levels(pattern.temperature, n_paths)
    beta = rows_in(pattern.beta, n_paths, layout, True)
    carry = rows_out(n_paths*angles, layout)
    reflection = rows_out(n_paths, layout)
    out = {}
    for sweep, up in (("down", False), ("up", True)):
        from_last = surface_first != up
        level = rows_out(levels, layout)
        mean = plain(levels, N_BANDS) if with_bands else None
        at_surface = plain(n_paths, N_BANDS) if with_bands and up else None
        ordered(engine)
        for first, count in in_order(runs, from_last):
            part = slice(first, first + count)
            engine.path_flux(
                Rows(beta[part]), C, grid, n_paths, L, first, lengths[part], weight,
                temperature[part], Rows(carry), Rows(reflection), Rows(level[part]),
                surface_temperature=many.tile_paths(pattern.surface_t, n_paths),
                surface_emissivity=many.tile_paths(pattern.surface_e, n_paths),
                flux=None if mean is None else Rows(mean[part]),
                surface_flux=None if at_surface is None else Rows(at_surface),
                band_start=BANDS if with_bands else None, up=up, from_last=from_last)
            engine.synchronize()
        out[sweep] = read(level, C)
        out["surface" if up else "reflection"] = read(reflection, C)
        if mean is not None:
            out[sweep + " mean"] = read(mean)
        if at_surface is not None:
            out["surface mean"] = read(at_surface)
    read(carry, C)      # its padding
    unwritten("beta", beta, pattern.beta, n_paths, True)
    return out


def flux_rules(angles, surface_first, with_bands):
    mirror = many.flux_mirror(angles, surface_first)
    rules = {name: (L if name in ("down", "up") else 1, ("close",) + mirror[name] + (BOUND,))
             for name in mirror}
    if with_bands:
        for name in ("down", "up", "surface"):
            rules[name + " mean"] = (rules[name][0], mean_rule(*mirror[name]))
    return rules


@parametrised(True)
def test_path_flux(engine, layout, n_paths, run_set):
    """K = 1 and K = 5, the two rows-in-flight classes of path_flux_kernel, with the surface
    behind the first level and behind the last: level fluxes, the reflection rows the down sweep
    leaves and the up sweep starts from, and the means of both and of the surface's flux."""
    with Grid(engine, many.sweep_pattern().nu) as grid:
        for angles, surface_first, with_bands in ((1, True, True), (1, False, False),
                                                  (5, False, True), (5, True, False)):
            what = ("flux", n_paths, layout, run_set, angles, surface_first, with_bands)
            scope, got, cut = both_ways(
                lambda runs: run_flux(engine, grid, n_paths, layout, runs, angles, surface_first,
                                      with_bands), n_paths, run_set, True)
            check("flux", what, scope, got, flux_rules(angles, surface_first, with_bands))
            if cut is not None:
                assert_same((what, "cut at the launch edge"), cut, got)


# ---------------------------------------------------------------------------------------------
# lbl_path_solar.
def run_solar(engine, n_paths, layout, runs, from_last, albedo_rows, with_bands):
    pattern = many.sweep_pattern()
    levels = n_paths*L
    beta = rows_in(pattern.beta, n_paths, layout, True)
    row = row_in(pattern.solar, layout)
    solar_lengths = many.tile_levels(pattern.solar_lengths, n_paths)
    view_lengths = many.tile_levels(pattern.view_lengths, n_paths)
    carry = rows_out(2*n_paths, layout)
    out_rows = {"interface_rows": rows_out(levels, layout)}
    for name in ("space_rows", "surface_rows", "reflected_rows"):
        out_rows[name] = rows_out(n_paths, layout)
    keywords, albedo = {}, None
    if albedo_rows:
        albedo = rows_in(pattern.albedo_rows, n_paths, layout)
        keywords["albedo_rows"] = Rows(albedo)
    else:
        keywords["albedo"] = many.tile_paths(pattern.albedo, n_paths)
    means = {}
    if with_bands:
        means = {name.replace("rows", "mean"): plain(rows.shape[0], N_BANDS)
                 for name, rows in out_rows.items()}
    ordered(engine)
    for first, count in in_order(runs, from_last):
        part = slice(first, first + count)
        per_level = {"interface_rows": Rows(out_rows["interface_rows"][part])}
        if with_bands:
            per_level["interface_mean"] = Rows(means["interface_mean"][part])
        engine.path_solar(
            Rows(beta[part]), C, n_paths, L, first, solar_lengths[part],
            many.tile_paths(pattern.mu0, n_paths), Rows(row), Rows(carry),
            view_lengths=view_lengths[part], band_start=BANDS if with_bands else None,
            from_last=from_last,
            **{k: Rows(v) for k, v in out_rows.items() if k != "interface_rows"},
            **{k: Rows(v) for k, v in means.items() if k != "interface_mean"},
            **per_level, **keywords)
        engine.synchronize()
    out = {"carry": read(carry, C)}
    out.update({name: read(rows, C) for name, rows in out_rows.items()})
    out.update({name: read(rows) for name, rows in means.items()})
    unwritten("beta", beta, pattern.beta, n_paths, True)
    assert same_bits(read(row)[0, :C], pattern.solar), "the solar row was written"
    if albedo is not None:
        unwritten("albedo rows", albedo, pattern.albedo_rows, n_paths)
    return out


def solar_allowed(reference):
    """test_gpu_solar_shapes.close's bound: 1.2e-15 relative, one subnormal step where the
    reference lies below the smallest normal double."""
    reference = np.abs(np.asarray(reference, dtype=LD))
    return np.where(reference < LD(solar.TINY), LD(solar.STEP), EXP_BOUND*reference)


def solar_rules(from_last, albedo_rows, with_bands):
    mirror = many.solar_mirror(from_last, True, albedo_rows)
    tau, tv = many.finals(mirror["tau"], from_last), many.finals(mirror["tv"], from_last)
    direct = mirror["direct"]
    at_surface = many.finals(direct, from_last)
    reference = {"interface": (L, direct), "space": (1, mirror["f0"].astype(LD)),
                 "surface": (1, at_surface), "reflected": (1, mirror["reflected"])}
    rules = {"carry": (2, ("bits", np.stack([tau, tv], axis=1).reshape(2*P, C))),
             "space_rows": (1, ("bits", mirror["f0"]))}
    for name in ("interface", "surface", "reflected"):
        k, values = reference[name]
        rules[name + "_rows"] = (k, ("allowed", values, solar_allowed(values)))
    if with_bands:
        for name, (k, values) in reference.items():
            flushed = cases.flushed(values)
            rules[name + "_mean"] = (k, mean_rule(flushed, np.abs(flushed), SOLAR_MEAN_BOUND))
    return rules


@parametrised(True)
def test_path_solar(engine, layout, n_paths, run_set):
    """With a viewer, the albedo as scalars and as a table, both orders: tau and tv in the carry
    rows are the float64 loop bit for bit, F0 = mu0*S is exact, the direct beam and the reflected
    radiance meet the long-double exponentials, the surface rows are the interface rows of each
    path's last level; the means of all four."""
    for from_last, albedo_rows, with_bands in ((False, False, True), (True, True, False),
                                               (True, False, True), (False, True, False)):
        what = ("solar", n_paths, layout, run_set, from_last, albedo_rows, with_bands)
        scope, got, cut = both_ways(
            lambda runs: run_solar(engine, n_paths, layout, runs, from_last, albedo_rows,
                                   with_bands), n_paths, run_set, True)
        check("solar", what, scope, got, solar_rules(from_last, albedo_rows, with_bands))
        last = np.arange(n_paths)*L + many.final_level(from_last)
        assert same_bits(got["surface_rows"][scope.first_path:],
                         got["interface_rows"][last][scope.first_path:]), (what, "surface")
        if cut is not None:
            assert_same((what, "cut at the launch edge"), cut, got)


# ---------------------------------------------------------------------------------------------
# The whole-path two-stream entries.
def flux_outputs(names, n_paths, layout, with_bands):
    rows = {name: rows_out(n_paths if name.startswith("top_") else n_paths*L, layout)
            for name in names}
    means = {} if not with_bands else {
        name: plain(n_paths if name.startswith("top_") else n_paths*L, N_BANDS) for name in names}
    return rows, means


def given(rows, means, part):
    """The keywords of a call on the levels `part`."""
    outputs = {}
    for name in rows:
        top = name.startswith("top_")
        outputs[name + "_rows"] = Rows(rows[name] if top else rows[name][part])
        if name in means:
            outputs[name + "_mean"] = Rows(means[name] if top else means[name][part])
    return outputs


def collected(rows, means, work, first_path):
    out = {name: read(tensor, C) for name, tensor in rows.items()}
    out.update({name + " mean": read(tensor) for name, tensor in means.items()})
    host = read(work, C)
    # Two work rows per level: those of the paths outside the run are left alone.
    assert np.all(host[:2*L*first_path] == SENTINEL), "work rows of paths outside the run"
    assert np.all(np.isfinite(host[2*L*first_path:])), "work"
    return out


def check_fluxes(kernel, what, scope, got, mirror, bound, with_bands):
    names = sorted(mirror)
    fine = {name: got[name] for name in names}
    check(kernel, what, scope, fine,
          {name: (1 if name.startswith("top_") else L, ("close",) + mirror[name] + (bound,))
           for name in names})
    for name in names:
        assert np.all(np.isfinite(scope.inside(got[name], 1 if name.startswith("top_") else L,
                                               (what, name)))), (what, name)
        if with_bands:
            check_own_means(kernel, (what, name), scope, got[name], got[name + " mean"],
                            1 if name.startswith("top_") else L, MEAN_BOUND)


def run_shortwave(engine, grid, n_paths, layout, runs, from_last, spectral, albedo_rows,
                  with_bands):
    pattern = many.shortwave_pattern(spectral)
    names = tuple(prefix + q for prefix in ("", "top_") for q in ts.QUANTITIES)
    beta = rows_in(pattern.beta, n_paths, layout, True)
    solar_row, sigma_row = row_in(pattern.solar, layout), row_in(pattern.sigma, layout)
    work = rows_out(2*n_paths*L, layout)
    rows, means = flux_outputs(names, n_paths, layout, with_bands)
    table = many.tile_levels(pattern.table, n_paths)
    optics = many.tile_levels(pattern.optics, n_paths) if spectral else None
    keywords, albedo = {}, None
    if albedo_rows:
        albedo = rows_in(pattern.albedo_rows, n_paths, layout)
        keywords["albedo_rows"] = Rows(albedo)
    else:
        keywords["albedo"] = many.tile_paths(pattern.albedo, n_paths)
    ordered(engine)
    for first, count in runs:
        part = slice(first, first + count)
        tail = (many.tile_paths(pattern.mu0, n_paths), Rows(solar_row),
                Rows(work[2*first:2*(first + count)]))
        more = dict(rayleigh_row=Rows(sigma_row), band_start=BANDS if with_bands else None,
                    from_last=from_last)
        if spectral:
            engine.path_two_stream_spectral(Rows(beta[part]), C, grid, n_paths, L, first,
                                            table[part], pattern.knots, optics[part], *tail,
                                            **more, **given(rows, means, part), **keywords)
        else:
            engine.path_two_stream(Rows(beta[part]), C, n_paths, L, first, table[part], *tail,
                                   **more, **given(rows, means, part), **keywords)
        engine.synchronize()
    unwritten("beta", beta, pattern.beta, n_paths, True)
    assert same_bits(read(solar_row)[0, :C], pattern.solar), "the solar row was written"
    assert same_bits(read(sigma_row)[0, :C], pattern.sigma), "the Rayleigh row was written"
    if albedo is not None:
        unwritten("albedo rows", albedo, pattern.albedo_rows, n_paths)
    return collected(rows, means, work, many.first_path_of(runs))


def shortwave_test(engine, layout, n_paths, run_set, spectral):
    pattern = many.shortwave_pattern(spectral)
    kernel = "two-stream spectral" if spectral else "two-stream"
    bound = SPECTRAL_SHORTWAVE_BOUND if spectral else SHORTWAVE_BOUND
    with Grid(engine, many.shortwave_pattern(True).nu) as grid:
        for from_last, albedo_rows, with_bands in ((True, False, True), (False, True, False)):
            what = (kernel, n_paths, layout, run_set, from_last, albedo_rows, with_bands)
            scope, got, cut = both_ways(
                lambda runs: run_shortwave(engine, grid, n_paths, layout, runs, from_last,
                                           spectral, albedo_rows, with_bands), n_paths, run_set,
                False)
            check_fluxes(kernel, what, scope, got, pattern.mirror(from_last, albedo_rows), bound,
                         with_bands)
            assert same_bits(got["top_direct"][scope.first_path:],
                             scope.tiled(pattern.f0(), 1)), (what, "F0")
            assert np.all(got["top_diffuse"][scope.first_path:] == 0.), (what, "diffuse at the top")
            if cut is not None:
                assert_same((what, "cut at the launch edge"), cut, got)


@parametrised(False)
def test_path_two_stream(engine, layout, n_paths, run_set):
    """All eight outputs within (4*E_cpu + 1e-13)*F0: every launch of the up sweep is queued before
    the first of the down sweep, over two work rows per level; scalar and spectral albedo."""
    shortwave_test(engine, layout, n_paths, run_set, False)


@parametrised(False)
def test_path_two_stream_spectral(engine, layout, n_paths, run_set):
    """The same with the scatterer of every level as a table of three knots."""
    shortwave_test(engine, layout, n_paths, run_set, True)


def run_longwave(engine, grid, n_paths, layout, runs, from_last, source, linear_source,
                 emissivity_rows, with_bands):
    pattern = many.longwave_pattern(source)
    beta = rows_in(pattern.beta, n_paths, layout, True)
    work = rows_out(2*n_paths*L, layout)
    rows, means = flux_outputs(tc.NAMES, n_paths, layout, with_bands)
    table = many.tile_levels(pattern.table, n_paths)
    edges = many.tile_levels(pattern.edges, n_paths) if linear_source else None
    optics = many.tile_levels(pattern.optics, n_paths) if source == "spectral" else None
    keywords, emissivity = {}, None
    if emissivity_rows:
        emissivity = rows_in(pattern.emissivity_rows, n_paths, layout)
        keywords["emissivity_rows"] = Rows(emissivity)
    else:
        keywords["emissivity"] = many.tile_paths(pattern.emissivity, n_paths)
    ordered(engine)
    for first, count in runs:
        part = slice(first, first + count)
        head = (Rows(beta[part]), C, grid, n_paths, L, first, table[part])
        tail = (many.tile_paths(pattern.surface_t, n_paths),
                Rows(work[2*first:2*(first + count)]))
        more = dict(diffusivity=pattern.diffusivity, band_start=BANDS if with_bands else None,
                    from_last=from_last)
        more.update(given(rows, means, part))
        more.update(keywords)
        if source == "spectral":
            engine.path_thermal_two_stream_spectral(
                *head, pattern.knots, optics[part], *tail,
                edge_temperature=None if edges is None else edges[part], **more)
        elif linear_source:
            engine.path_thermal_two_stream_source(*head, edges[part], *tail, **more)
        else:
            engine.path_thermal_two_stream(*head, *tail, **more)
        engine.synchronize()
    unwritten("beta", beta, pattern.beta, n_paths, True)
    if emissivity is not None:
        unwritten("emissivity rows", emissivity, pattern.emissivity_rows, n_paths)
    return collected(rows, means, work, many.first_path_of(runs))


def longwave_test(engine, layout, n_paths, run_set, source, kernel, bound, sources):
    pattern = many.longwave_pattern(source)
    with Grid(engine, pattern.nu) as grid:
        for linear_source in sources:
            for from_last, emissivity_rows, with_bands in ((True, False, True),
                                                           (False, True, False)):
                what = (kernel, n_paths, layout, run_set, linear_source, from_last,
                        emissivity_rows, with_bands)
                scope, got, cut = both_ways(
                    lambda runs: run_longwave(engine, grid, n_paths, layout, runs, from_last,
                                              source, linear_source, emissivity_rows,
                                              with_bands), n_paths, run_set, False)
                check_fluxes(kernel, what, scope, got,
                             pattern.mirror(from_last, emissivity_rows, linear_source), bound,
                             with_bands)
                assert np.all(got["top_down"][scope.first_path:] == 0.), (what, "from space")
                if cut is not None:
                    assert_same((what, "cut at the launch edge"), cut, got)


@parametrised(False)
def test_path_thermal_two_stream(engine, layout, n_paths, run_set):
    """Cloudy and clear levels, a conservative cloud, eps = 1, inside (0, 1) and 0, scalar and
    spectral emissivity: all four outputs within (4*E_cpu + 1e-13)*scale, and their means."""
    longwave_test(engine, layout, n_paths, run_set, "isothermal", "thermal", THERMAL_BOUND,
                  (False,))


@parametrised(False)
def test_path_thermal_two_stream_source(engine, layout, n_paths, run_set):
    """The same with the linear-in-tau source: the edge temperatures are per-level rows too."""
    longwave_test(engine, layout, n_paths, run_set, "linear", "thermal source",
                  THERMAL_SOURCE_BOUND, (True,))


@parametrised(False)
def test_path_thermal_two_stream_spectral(engine, layout, n_paths, run_set):
    """The same with the scatterer as a table of three knots, under either source."""
    longwave_test(engine, layout, n_paths, run_set, "spectral", "thermal spectral",
                  SPECTRAL_LONGWAVE_BOUND, (False, True))


# ---------------------------------------------------------------------------------------------
# lbl_path_thermal_radiance, on flux rows made by the numpy mirror.
def run_view(engine, grid, n_paths, layout, runs, from_last, with_bands):
    pattern = many.longwave_pattern("isothermal")
    fluxes = pattern.flux_rows(from_last)
    beta = rows_in(pattern.beta, n_paths, layout, True)
    up = rows_in(fluxes["up"], n_paths, layout, True)
    down = rows_in(fluxes["down"], n_paths, layout, True)
    table = many.tile_levels(pattern.table, n_paths)
    rows = {name: rows_out(n_paths, layout) for name in ("radiance", "brightness")}
    mean = plain(n_paths, N_BANDS) if with_bands else None
    ordered(engine)
    for first, count in runs:
        part = slice(first, first + count)
        outputs = {name + "_rows": Rows(tensor) for name, tensor in rows.items()}
        if mean is not None:
            outputs["radiance_mean"] = Rows(mean)
        engine.path_thermal_radiance(
            Rows(beta[part]), C, grid, n_paths, L, first, table[part],
            many.tile_paths(pattern.view_mu, n_paths),
            many.tile_paths(pattern.surface_t, n_paths), Rows(up[part]), Rows(down[part]),
            diffusivity=pattern.diffusivity,
            emissivity=many.tile_paths(pattern.emissivity, n_paths),
            band_start=BANDS if with_bands else None, from_last=from_last, **outputs)
        engine.synchronize()
    unwritten("beta", beta, pattern.beta, n_paths, True)
    unwritten("up_rows", up, fluxes["up"], n_paths, True)
    unwritten("down_rows", down, fluxes["down"], n_paths, True)
    out = {name: read(tensor, C) for name, tensor in rows.items()}
    if mean is not None:
        out["radiance mean"] = read(mean)
    return out


@parametrised(False, (many.N2, many.N3))
def test_path_thermal_radiance(engine, layout, n_paths, run_set):
    """Seven view cosines and emissivities (thermal_radiance_cases.MU, thermal_cases.EMISSIVITY and
    four more of each), a cloudy level that reads `down` of the next one: the radiance within
    (4*E_cpu + 1e-13)*scale, the brightness temperature the inversion of the radiance the call
    wrote, and the per-path means."""
    pattern = many.longwave_pattern("isothermal")
    with Grid(engine, pattern.nu) as grid:
        for from_last, with_bands in ((False, True), (True, False)):
            what = ("view", n_paths, layout, run_set, from_last, with_bands)
            scope, got, cut = both_ways(
                lambda runs: run_view(engine, grid, n_paths, layout, runs, from_last, with_bands),
                n_paths, run_set, False)
            mirror = pattern.view_mirror(from_last)
            check("thermal radiance", what, scope, {"radiance": got["radiance"]},
                  {"radiance": (1, ("close",) + mirror["radiance"] + (VIEW_BOUND,))})
            radiance = scope.inside(got["radiance"], 1, what)
            brightness = scope.inside(got["brightness"], 1, what)
            periodic((what, "brightness"), brightness, 1)
            assert np.all(np.isfinite(radiance)) and np.all(np.isfinite(brightness)), what
            inverted = cases.brightness(LD, pattern.nu[None, :], radiance)
            within("thermal radiance brightness", (what, "brightness"), brightness, inverted,
                   BRIGHTNESS_BOUND*inverted, GRID_Y)
            assert np.array_equal(brightness == 0., inverted == 0.), (what, "brightness")
            if with_bands:
                check_own_means("thermal radiance", what, scope, got["radiance"],
                                got["radiance mean"], 1, MEAN_BOUND)
            if cut is not None:
                assert_same((what, "cut at the launch edge"), cut, got)

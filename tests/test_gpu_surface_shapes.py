"""lbl_surface_emissivity and lbl_path_radiance_surface fed directly (Engine.surface_emissivity /
Engine.path_radiance with emissivity_rows and reflection on rows held in torch tensors): the
columns and layouts of tests/sweep_cases.py (odd strides, bases 8 bytes off, one-column tail lanes,
NaN padding), depths around kPathAhead, runs that cut paths, knot tables at their edges, grids that
are not ascending, and values chosen for the arithmetic.

Expected values come from the long-double mirror of tests/surface_cases.py alone.  Bounds: E is
within surface_cases.INTERPOLATION_BOUND (the roundings of the written formula) of long double;
radiances are within 1e-12 of the magnitude they are formed from -- the sweeps' recurrence over
absolute values started from |E|*B + |1 - E|*|D|.  Layouts, runs and the identities are compared
bit for bit."""
import numpy as np
import pytest

from pylbl_amd.errors import EngineError
from tests import linear_source_cases as linear
from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests import test_gpu_sweep_shapes as shapes

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
Rows, Grid = shapes.Rows, shapes.Grid
same_bits, read, ordered, block = shapes.same_bits, shapes.read, shapes.ordered, shapes.block
VECTOR, SCALAR = "aligned", "odd"


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    yield default_engine(0)
    for kernel, ratio in sorted(shapes.WORST.items()):
        print("\nworst error / bound, %s: %.3g" % (kernel, ratio))


def layouts_for(columns):
    return list(cases.LAYOUTS) if columns in cases.LAYOUT_COLUMNS else [VECTOR]


def table_for(nu, m, seed):
    """M knots inside and around the grid's range, PATHS tables: one flat, one random, one that
    alternates between 0 and 1."""
    rng = np.random.default_rng(seed)
    lo, hi = float(np.min(nu)), float(np.max(nu))
    span = max(hi - lo, 1.)
    knots = np.sort(rng.uniform(lo - 0.1*span, hi + 0.1*span, size=m))
    assert np.all(np.diff(knots) > 0.)
    values = rng.uniform(0., 1., size=(PATHS, m))
    values[0] = 0.625
    values[2, ::2], values[2, 1::2] = 0., 1.
    return knots, values


def fill(engine, grid, columns, layout, knots, values, path_begin=0):
    """The rows lbl_surface_emissivity leaves: [PATHS, columns], untouched rows are SENTINEL."""
    rows = block(None, PATHS, columns, layout, SENTINEL)
    ordered(engine)
    engine.surface_emissivity(grid, Rows(rows), knots, values, path_begin=path_begin)
    engine.synchronize()
    return read(rows, columns), rows


def check_fill(what, got, knots, values, nu):
    reference = surface.emissivity(LD, knots, values, nu)
    error = np.abs(got.astype(LD) - reference)
    ratio = float(error.max()/LD(surface.INTERPOLATION_BOUND))
    shapes.WORST["emissivity"] = max(shapes.WORST.get("emissivity", 0.), ratio)
    assert np.all(np.isfinite(got)) and ratio <= 1., (what, ratio)
    # Each operation rounded as written: the float64 mirror's bits.
    assert same_bits(got, surface.emissivity(F64, knots, values, nu)), what


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("columns", cases.COLUMNS)
def test_fill_columns_and_layouts(engine, columns):
    problem = cases.Problem(columns, 1, seed=900 + columns)
    assert problem.nu[0] == 0.
    knots, values = table_for(problem.nu, 3, 901 + columns)
    with Grid(engine, problem.nu) as grid:
        base, _ = fill(engine, grid, columns, VECTOR, knots, values)
        check_fill(columns, base, knots, values, problem.nu)
        assert np.all(base[0] == 0.625)
        for layout in layouts_for(columns):
            got, _ = fill(engine, grid, columns, layout, knots, values)
            assert same_bits(got, base), (columns, layout)
        # Some of the paths only: the other rows are left alone.
        part, _ = fill(engine, grid, columns, VECTOR, knots, values[1:], path_begin=1)
        assert np.all(part[0] == SENTINEL) and same_bits(part[1:], base[1:])
        one, _ = fill(engine, grid, columns, SCALAR, knots, values[1:2], path_begin=1)
        assert np.all(one[[0, 2]] == SENTINEL) and same_bits(one[1], base[1])


def knot_grids():
    """{name: (nu, knots)} on 515 columns (two blocks, a one-column tail lane)."""
    columns = 515
    nu = 600. + 0.25*np.arange(columns)
    rng = np.random.default_rng(77)
    out = {}
    for m in (2, 3, 1024):
        out["M = %d" % m] = (nu, np.sort(rng.uniform(590., 740., size=m)))
    # An interval narrower than a grid step (no point inside), between two wide ones.
    out["narrow interval"] = (nu, np.array([600., 650.30, 650.40, 700.]))
    out["wider than the grid"] = (nu, np.array([10., 5000.]))
    out["grid inside one end"] = (nu, np.array([10., 20.]))
    # Grid points exactly on knots at the edges of wavefronts (columns 127 | 128, 255 | 256):
    # the wavefront before ends on the knot, the one after starts in the next interval.
    on = np.array([nu[0], nu[127], nu[128], nu[256], nu[383], nu[514]])
    out["knots on wavefront edges"] = (nu, on)
    out["knot inside a wavefront"] = (nu, np.array([nu[5], nu[70] + 0.1, nu[200]]))
    out["descending"] = (nu[::-1].copy(), out["M = 3"][1])
    shuffled = nu.copy()
    rng.shuffle(shuffled)
    out["shuffled"] = (shuffled, out["M = 1024"][1])
    zero = nu.copy()
    zero[0] = 0.
    out["nu = 0"] = (zero, np.array([0., 650., 700.]))
    return out


@pytest.mark.parametrize("name", list(knot_grids()))
def test_fill_knots(engine, name):
    nu, knots = knot_grids()[name]
    rng = np.random.default_rng(len(name))
    values = rng.uniform(0., 1., size=(PATHS, knots.size))
    values[0] = 1.
    if name in ("descending", "shuffled"):
        assert not np.all(np.diff(nu) >= 0.)
    else:
        # Both the shared search and the per-lane one are reached (or, for the wide tables,
        # every wavefront shares).
        first = surface.interval(knots, nu[0::128])
        last = surface.interval(knots, nu[np.minimum(np.arange(127, 515 + 127, 128), 514)])
        if name in ("wider than the grid", "grid inside one end"):
            assert np.all(first == last)
        else:
            assert np.any(first != last)
        if name in ("knots on wavefront edges", "narrow interval"):
            assert np.any(first == last)
    with Grid(engine, nu) as grid:
        for layout in (VECTOR, SCALAR):
            got, _ = fill(engine, grid, nu.size, layout, knots, values)
            check_fill((name, layout), got, knots, values, nu)
            assert np.all(got[0] == 1.)
    if name == "knots on wavefront edges":
        assert np.array_equal(got[1, [0, 127, 128, 256, 383, 514]], values[1])


# ---------------------------------------------------------------------------------------------
# The sweeps.
def sweep(engine, grid, problem, layout, runs, from_last, e_rows=None, d_rows=None, edges=None,
          cumulative=True, plain=False, boundary_e=None):
    """lbl_path_radiance_surface (plain: Engine.path_radiance without the two rows) over `runs`
    in sweep order: {"rad": [levels or PATHS, columns], "carry@level": ...}."""
    n, columns, levels = problem.levels_per_path, problem.columns, problem.levels
    beta = block(problem.beta, levels, columns, layout, np.nan)
    carry = block(None, PATHS, columns, layout, SENTINEL)
    rad = block(None, levels if cumulative else PATHS, columns, layout, SENTINEL)
    more = {}
    if not plain:
        more = dict(emissivity_rows=None if e_rows is None else Rows(e_rows),
                    reflection=None if d_rows is None else Rows(d_rows))
    out = {}
    ordered(engine)
    for first, count in shapes.in_order(runs, from_last):
        part = slice(first, first + count)
        engine.path_radiance(
            Rows(beta[part]), columns, grid, PATHS, n, first, problem.thickness[part],
            problem.temperature[part], Rows(carry), boundary_temperature=problem.boundary_t,
            boundary_emissivity=problem.boundary_e if boundary_e is None else boundary_e,
            radiance=Rows(rad[part] if cumulative else rad), cumulative=cumulative,
            from_last=from_last, edge_temperature=None if edges is None else edges[part], **more)
        engine.synchronize()
        left = shapes.unfinished(first, count, n, from_last)
        if left is not None:
            out["carry@%d" % left[1]] = read(carry, columns)[left[0]]
    out["rad"] = read(rad, columns)
    assert np.all(read(beta)[:, :columns] == problem.beta)
    return out


def down_pass(engine, grid, problem, layout, runs, from_last, lengths, edges=None):
    """D as the header says it is formed: lbl_path_radiance_source against the direction, no
    boundary, the reflection rows as its per-path output.  Returns (values, the rows)."""
    n, columns, levels = problem.levels_per_path, problem.columns, problem.levels
    beta = block(problem.beta, levels, columns, layout, np.nan)
    carry = block(None, PATHS, columns, layout, SENTINEL)
    rows = block(None, PATHS, columns, layout, SENTINEL)
    ordered(engine)
    for first, count in shapes.in_order(runs, not from_last):
        part = slice(first, first + count)
        engine.path_radiance(
            Rows(beta[part]), columns, grid, PATHS, n, first, lengths[part],
            problem.temperature[part], Rows(carry), radiance=Rows(rows), from_last=not from_last,
            edge_temperature=None if edges is None else edges[part])
        engine.synchronize()
    return read(rows, columns), rows


def surface_problem(columns, n, seed, signed=False):
    problem = cases.Problem(columns, n, seed=seed, signed=signed)
    problem.boundary_t = np.array([260., 288., 215.])
    problem.edges = linear.edge_table(linear.interfaces_for(problem, seed + 1))
    problem.reflection = 1.66*problem.thickness
    problem.knots, problem.table = table_for(problem.nu, 5, seed + 2)
    return problem


def reference(problem, from_last, spectral=True, reflecting=True, linear_source=False):
    def form():
        e = surface.emissivity(LD, problem.knots, problem.table, problem.nu) if spectral \
            else problem.boundary_e
        return surface.two_pass(LD, problem, from_last, e,
                                problem.reflection if reflecting else None,
                                problem.edges if linear_source else None)
    return shapes.cached(problem, ("surface", from_last, spectral, reflecting, linear_source),
                         form)


def check_sweep(what, got, problem, from_last, cumulative=True, **kind):
    rad, mag = reference(problem, from_last, **kind)["up"]
    n = problem.levels_per_path
    rows = slice(None) if cumulative else surface.final_rows(n, from_last)
    shapes.close("surface radiance", what, got["rad"], rad[rows], mag[rows])
    for key in got:
        if "@" in key:
            level = int(key.split("@")[1])
            shapes.close("surface radiance", (what, key), got[key], rad[level], mag[level])


def surface_rows(engine, grid, problem, layout, runs, from_last, linear_source):
    _, e_rows = fill(engine, grid, problem.columns, layout, problem.knots, problem.table)
    d, d_rows = down_pass(engine, grid, problem, layout, runs, from_last, problem.reflection,
                          problem.edges if linear_source else None)
    return e_rows, d_rows, d


@pytest.mark.parametrize("columns", cases.COLUMNS)
def test_sweep_columns_and_layouts(engine, columns):
    """9 levels (a batch and a remainder), the four kSurface instantiations -- isothermal and
    linear, vector (aligned) and scalar (the other layouts) -- in both directions."""
    problem = surface_problem(columns, 9, 1000 + columns)
    whole = cases.run_sets(9)["whole"]
    with Grid(engine, problem.nu) as grid:
        for linear_source in (False, True):
            edges = problem.edges if linear_source else None
            for from_last in (False, True):
                what = (columns, linear_source, from_last)
                ref = reference(problem, from_last, linear_source=linear_source)
                base = None
                for layout in layouts_for(columns):
                    e_rows, d_rows, d = surface_rows(engine, grid, problem, layout, whole,
                                                     from_last, linear_source)
                    shapes.close("surface down", (what, layout), d, *ref["down"])
                    got = sweep(engine, grid, problem, layout, whole, from_last, e_rows, d_rows,
                                edges)
                    if base is None:
                        base = got
                        check_sweep(what, got, problem, from_last, linear_source=linear_source)
                    else:
                        assert same_bits(got["rad"], base["rad"]), (what, layout)
    print("worst error / bound so far:", shapes.WORST)


@pytest.mark.parametrize("n", [1, 8, 9, 17])
def test_depths_and_run_cuts(engine, n):
    """Depths around kPathAhead = 8, whole and in runs that cut paths -- the middle run of
    "uneven" holds the tail of path 0, all of path 1 and the head of path 2, "levels" is one level
    per call: a path takes its start value in the run it starts in and its carry row afterwards,
    so every run set gives the whole call's bits, per level and per path."""
    problem = surface_problem(515, n, 1100 + n, signed=n == 9)
    sets = cases.run_sets(n)
    names = ["uneven", "uneven mirrored", "levels"] if n > 1 else ["levels"]
    if n > 1:
        cut = [lane for first, count in sets["uneven"]
               for lane in cases.path_lanes(first, count, n, False)]
        assert any(not lane.starts for lane in cut) and any(not lane.finishes for lane in cut)
    with Grid(engine, problem.nu) as grid:
        for linear_source in (False, True):
            edges = problem.edges if linear_source else None
            for from_last in (False, True):
                for layout in (VECTOR, SCALAR):
                    what = (n, linear_source, from_last, layout)
                    e_rows, d_rows, _ = surface_rows(engine, grid, problem, layout,
                                                     sets["whole"], from_last, linear_source)
                    base = sweep(engine, grid, problem, layout, sets["whole"], from_last, e_rows,
                                 d_rows, edges)
                    check_sweep(what, base, problem, from_last, linear_source=linear_source)
                    final = sweep(engine, grid, problem, layout, sets["whole"], from_last,
                                  e_rows, d_rows, edges, cumulative=False)
                    rows = surface.final_rows(n, from_last)
                    assert same_bits(final["rad"], base["rad"][rows]), what
                    for name in names:
                        # The down pass in the same runs: its carry too crosses them.
                        _, d_cut = down_pass(engine, grid, problem, layout, sets[name], from_last,
                                             problem.reflection, edges)
                        assert same_bits(read(d_cut), read(d_rows)), (what, name)
                        got = sweep(engine, grid, problem, layout, sets[name], from_last, e_rows,
                                    d_cut, edges)
                        assert same_bits(got["rad"], base["rad"]), (what, name)
                        check_sweep((what, name), got, problem, from_last,
                                    linear_source=linear_source)
                        if n > 1 and name == "uneven":
                            assert any("@" in key for key in got)
    print("worst error / bound so far:", shapes.WORST)


def test_identities_bit_for_bit(engine):
    problem = surface_problem(515, 9, 1200)
    problem.boundary_e = np.array([0.625, 0.9, 0.])
    whole = cases.run_sets(9)["uneven"]
    with Grid(engine, problem.nu) as grid:
        for linear_source in (False, True):
            edges = problem.edges if linear_source else None
            for from_last in (False, True):
                for layout in (VECTOR, SCALAR):
                    what = (linear_source, from_last, layout)
                    plain = sweep(engine, grid, problem, layout, whole, from_last, edges=edges,
                                  plain=True)
                    # Both pointers NULL: lbl_path_radiance_source.
                    null = sweep(engine, grid, problem, layout, whole, from_last, edges=edges)
                    assert same_bits(null["rad"], plain["rad"]), what
                    # A flat table c without reflection: the scalar eps = c.
                    flat = np.repeat(problem.boundary_e[:, None], 4, axis=1)
                    _, e_rows = fill(engine, grid, problem.columns, layout,
                                     np.array([100., 700., 701., 9000.]), flat)
                    assert np.all(read(e_rows, problem.columns) == problem.boundary_e[:, None])
                    got = sweep(engine, grid, problem, layout, whole, from_last, e_rows,
                                edges=edges, boundary_e=np.zeros(PATHS))
                    assert same_bits(got["rad"], plain["rad"]), what
                    # Emissivity rows all 1 with reflection: the plain call with eps = 1.
                    _, ones = fill(engine, grid, problem.columns, layout, np.array([1., 2.]),
                                   np.ones((PATHS, 2)))
                    _, d_rows = down_pass(engine, grid, problem, layout, whole, from_last,
                                          problem.reflection, edges)
                    black = sweep(engine, grid, problem, layout, whole, from_last, edges=edges,
                                  plain=True, boundary_e=np.ones(PATHS))
                    got = sweep(engine, grid, problem, layout, whole, from_last, ones, d_rows,
                                edges)
                    assert same_bits(got["rad"], black["rad"]), what
                    # The scalar eps with reflection meets the mirror.
                    got = sweep(engine, grid, problem, layout, whole, from_last, None, d_rows,
                                edges)
                    check_sweep(what, got, problem, from_last, spectral=False,
                                linear_source=linear_source)
                    assert not same_bits(got["rad"], plain["rad"])


def test_values_chosen_for_the_arithmetic(engine):
    """sweep_cases.value_problem: columns with beta = 0 throughout (D = 0: the start is E*B
    alone), saturating first and last levels (D is B of the level next to the surface), beta of
    mixed sign, boundaries at 1 K and 5 K whose E*B underflows, nu = 0."""
    problem = cases.value_problem()
    problem.boundary_t = np.array([288., 1., 5.])
    problem.edges = linear.edge_table(linear.interfaces_for(problem, 1301))
    problem.reflection = problem.thickness.copy()
    problem.knots, problem.table = table_for(problem.nu, 7, 1302)
    problem.table[1] = 0.5
    whole = cases.run_sets(9)["whole"]
    group = problem.group
    with Grid(engine, problem.nu) as grid:
        for linear_source in (False, True):
            edges = problem.edges if linear_source else None
            for from_last in (False, True):
                for layout in (VECTOR, SCALAR):
                    what = ("values", linear_source, from_last, layout)
                    e_rows, d_rows, d = surface_rows(engine, grid, problem, layout, whole,
                                                     from_last, linear_source)
                    ref = reference(problem, from_last, linear_source=linear_source)
                    shapes.close("surface down", what, d, *ref["down"])
                    assert np.all(d[:, group == 0] == 0.) and np.all(d[:, 0] == 0.)
                    near = 0 if not from_last else 8        # the level next to the boundary
                    if not linear_source:
                        b = cases.planck(LD, problem.nu[None, :],
                                         problem.temperature[cases._flat(9, near)][:, None])
                        thick = group == 1
                        assert np.allclose(d[:, thick], b[:, thick].astype(F64), rtol=1e-13,
                                           atol=0.)
                    got = sweep(engine, grid, problem, layout, whole, from_last, e_rows, d_rows,
                                edges)
                    assert not np.any(np.isnan(got["rad"])) and not np.any(np.isinf(got["rad"]))
                    check_sweep(what, got, problem, from_last, linear_source=linear_source)
                    # Where E*B has underflowed and nothing comes down, the start is 0 exactly.
                    start = ref["start"][0]
                    assert np.any(cases.flushed(start[1:]) == 0.)
    print("worst error / bound so far:", shapes.WORST)


# ---------------------------------------------------------------------------------------------
def test_rejected_calls_launch_nothing_and_leave_the_engine_usable(engine):
    problem = surface_problem(515, 5, 1400)
    whole = [(0, problem.levels)]
    good_knots, good = problem.knots, problem.table
    with Grid(engine, problem.nu) as grid:
        base, rows = fill(engine, grid, 515, VECTOR, good_knots, good)

        def refused(knots, values, match, **more):
            before = read(rows)
            with pytest.raises(EngineError, match=match):
                engine.surface_emissivity(grid, Rows(rows), knots, values, **more)
            engine.synchronize()
            assert same_bits(read(rows), before)

        spoiled = good.copy()
        spoiled[1, 2] = 1.5
        refused(good_knots, spoiled, r"\[0, 1\]")
        spoiled[1, 2] = -1e-9
        refused(good_knots, spoiled, r"\[0, 1\]")
        spoiled[1, 2] = np.nan
        refused(good_knots, spoiled, r"\[0, 1\]")
        knots = good_knots.copy()
        knots[2] = knots[1]
        refused(knots, good, "strictly ascending")
        refused(good_knots[::-1].copy(), good, "strictly ascending")
        knots = good_knots.copy()
        knots[4] = np.inf
        refused(knots, good, "strictly ascending")
        knots[4] = np.nan
        refused(knots, good, "strictly ascending")
        refused(np.array([700.]), np.ones((PATHS, 1)), "2..1024")
        refused(np.arange(1025.), np.ones((PATHS, 1025)), "2..1024")
        refused(good_knots, good, "inside n_paths", path_begin=1)
        with pytest.raises(EngineError, match="unknown grid"):
            engine.surface_emissivity(grid + 1000, Rows(rows), good_knots, good)
        short = block(None, PATHS, 100, VECTOR, SENTINEL)
        with pytest.raises(EngineError, match="row_stride"):
            engine.surface_emissivity(grid, Rows(short), good_knots, good)

        # Reflection behind a path without a boundary.
        e_rows, d_rows, _ = surface_rows(engine, grid, problem, VECTOR, whole, False, False)
        ok = sweep(engine, grid, problem, VECTOR, whole, False, e_rows, d_rows)
        problem.boundary_t = np.array([260., 0., 215.])
        with pytest.raises(EngineError, match="lbl_path_radiance_surface.*boundary temperature"):
            sweep(engine, grid, problem, VECTOR, whole, False, e_rows, d_rows)
        # A run that does not hold that path is taken; spectral rows alone need no boundary.
        sweep(engine, grid, problem, VECTOR, [(0, 5)], False, e_rows, d_rows)
        sweep(engine, grid, problem, VECTOR, whole, False, e_rows, None)
        with pytest.raises(ValueError, match="reflection"):
            sweep(engine, grid, problem, VECTOR, whole, False, e_rows, d_rows[:2])
        problem.boundary_t = np.array([260., 288., 215.])
        again = sweep(engine, grid, problem, VECTOR, whole, False, e_rows, d_rows)
        assert same_bits(again["rad"], ok["rad"])
        after, _ = fill(engine, grid, 515, VECTOR, good_knots, good)
        assert same_bits(after, base)

"""lbl_path_radiance_source and lbl_path_flux_source fed directly (Engine.path_radiance /
path_flux with edge_temperature on rows held in torch tensors): 3 paths of 2*ahead + 3 levels on
515 columns (two blocks and a one-column tail lane), in the vector instantiations (even stride,
aligned bases) and the scalar ones (odd stride, base 8 bytes off), both directions, whole and in
runs that cut paths in the middle, every K of the flux kernel.

Bound: 1e-12 times the magnitude the result is formed from -- the sum over levels of
|I_in|*t + (|B_in| + |B_out|)*|a| -- against the long-double mirror of
tests/linear_source_cases.py, whose weight is a 24-term series below |x| = 0.5.  Runs, layouts
and the K = 1, w = 1 flux against the radiance are compared bit for bit."""
from collections import namedtuple

import numpy as np
import pytest

from pylbl_amd.errors import EngineError
from tests import linear_source_cases as linear
from tests import sweep_cases as cases
from tests import test_gpu_sweep_shapes as shapes

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
COLUMNS = 515
Rows, Grid = shapes.Rows, shapes.Grid
same_bits, read, plain, ordered = shapes.same_bits, shapes.read, shapes.plain, shapes.ordered

Layout = namedtuple("Layout", "name stride offset")
VECTOR = Layout("vector", lambda columns: columns + columns % 2, 0)
SCALAR = Layout("scalar", lambda columns: columns + 1 - columns % 2, 1)
LAYOUTS = (VECTOR, SCALAR)


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    yield default_engine(0)
    for kernel, ratio in sorted(shapes.WORST.items()):
        print("\nworst error / bound, %s: %.3g" % (kernel, ratio))


def block(values, rows, columns, layout, fill):
    """tests/test_gpu_sweep_shapes.py's block for a Layout of this file."""
    import torch
    stride = layout.stride(columns)
    host = np.full((rows, stride), fill, dtype=F64)
    if values is not None:
        host[:, :columns] = values
    flat = torch.full((rows*stride + 2,), fill, dtype=torch.float64, device="cuda:0")
    view = flat[layout.offset:layout.offset + rows*stride].view(rows, stride)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 16 == 8*(layout.offset % 2)
    assert cases.path_vector(stride, [layout.offset]) == (layout is VECTOR)
    return view


def test_shapes_reach_what_they_are_for():
    assert COLUMNS % cases.PATH_WIDTH == 1 and COLUMNS > cases.PATH_THREADS*cases.PATH_WIDTH
    assert cases.lane_widths(COLUMNS) == {1, 2}
    assert SCALAR.stride(COLUMNS) % 2 == 1 and SCALAR.offset == 1
    for angles in cases.ANGLES:
        n = cases.angle_levels(angles)
        assert n == (19 if angles <= 4 else 11)
        assert cases.depth_class(n, cases.flux_ahead(angles)) == "batches and remainder"
        cut = [lane for first, count in cases.run_sets(n)["uneven"]
               for lane in cases.path_lanes(first, count, n, False)]
        assert any(not lane.starts for lane in cut) and any(not lane.finishes for lane in cut)


# ---------------------------------------------------------------------------------------------
def problem_for(n, seed, signed=False):
    problem = cases.Problem(COLUMNS, n, seed=seed, signed=signed)
    problem.interfaces = linear.interfaces_for(problem, seed + 1)
    problem.edges = linear.edge_table(problem.interfaces)
    assert problem.nu[0] == 0.
    return problem


def run_radiance(engine, grid, problem, layout, runs, from_last, cumulative=True, boundary=True,
                 edges=True):
    n, columns, levels = problem.levels_per_path, problem.columns, problem.levels
    beta = block(problem.beta, levels, columns, layout, np.nan)
    carry = block(None, PATHS, columns, layout, SENTINEL)
    rows = levels if cumulative else PATHS
    rad = block(None, rows, columns, layout, SENTINEL)
    out = {}
    ordered(engine)
    for first, count in shapes.in_order(runs, from_last):
        part = slice(first, first + count)
        engine.path_radiance(
            Rows(beta[part]), columns, grid, PATHS, n, first, problem.thickness[part],
            problem.temperature[part], Rows(carry),
            boundary_temperature=problem.boundary_t if boundary else None,
            boundary_emissivity=problem.boundary_e if boundary else None,
            radiance=Rows(rad[part] if cumulative else rad), cumulative=cumulative,
            from_last=from_last, edge_temperature=problem.edges[part] if edges else None)
        engine.synchronize()
        left = shapes.unfinished(first, count, n, from_last)
        if left is not None:
            out["carry@%d" % left[1]] = read(carry, columns)[left[0]]
    out["rad"] = read(rad, columns)
    return out


def reference_radiance(problem, from_last, boundary=True):
    start = cases.boundary_start(LD, problem.nu, problem.boundary_t, problem.boundary_e) \
        if boundary else None
    return shapes.cached(problem, ("linear radiance", from_last, boundary),
                         lambda: linear.sweep_radiance(LD, problem.nu, problem.beta,
                                                       problem.thickness, problem.edges,
                                                       problem.levels_per_path, from_last, start))


def check_radiance(what, got, problem, from_last, cumulative=True, boundary=True):
    rad, mag = reference_radiance(problem, from_last, boundary)
    n = problem.levels_per_path
    rows = slice(None) if cumulative else cases._flat(n, 0 if from_last else n - 1)
    shapes.close("linear radiance", what, got["rad"], rad[rows], mag[rows])
    for key in got:
        if "@" in key:
            level = int(key.split("@")[1])
            shapes.close("linear radiance", (what, key), got[key], rad[level], mag[level])


def run_flux(engine, grid, problem, layout, runs, angles, surface):
    n, columns, levels = problem.levels_per_path, problem.columns, problem.levels
    lengths, weight = problem.lengths(angles)
    beta = block(problem.beta, levels, columns, layout, np.nan)
    carry = block(None, PATHS*angles, columns, layout, SENTINEL)
    reflection = block(None, PATHS, columns, layout, SENTINEL)
    out = {}
    for sweep, up in (("down", False), ("up", True)):
        from_last = (surface == "first") != up
        level = block(None, levels, columns, layout, SENTINEL)
        ordered(engine)
        for first, count in shapes.in_order(runs, from_last):
            part = slice(first, first + count)
            engine.path_flux(
                Rows(beta[part]), columns, grid, PATHS, n, first, lengths[part], weight,
                problem.temperature[part], Rows(carry), Rows(reflection), Rows(level[part]),
                surface_temperature=problem.surface_t, surface_emissivity=problem.surface_e,
                up=up, from_last=from_last, edge_temperature=problem.edges[part])
            engine.synchronize()
            left = shapes.unfinished(first, count, n, from_last)
            if left is not None:
                rows = slice(left[0]*angles, (left[0] + 1)*angles)
                out["%s carry@%d" % (sweep, left[1])] = read(carry, columns)[rows]
        out[sweep] = read(level, columns)
        out["surface" if up else "reflection"] = read(reflection, columns)
    assert np.all(read(beta)[:, :columns] == problem.beta)      # the block is only read
    return out


def check_flux(what, got, problem, angles, surface):
    n, nu = problem.levels_per_path, problem.nu
    lengths, weight = problem.lengths(angles)
    down_last = surface == "first"

    def sweep():
        down = linear.sweep_flux(LD, nu, problem.beta, lengths, weight, problem.edges, n,
                                 down_last)
        start, start_mag = cases.surface_start(LD, nu, problem.surface_t, problem.surface_e,
                                               down.total, down.total_mag)
        return down, start, start_mag, linear.sweep_flux(
            LD, nu, problem.beta, lengths, weight, problem.edges, n, not down_last, start,
            start_mag)
    down, start, start_mag, up = shapes.cached(problem, ("linear flux", angles, surface), sweep)
    w, pi = weight.astype(LD), LD(cases.FLUX_PI)
    at_surface = pi*cases.flux_sum(w, np.repeat(start[:, None, :], angles, axis=1))
    at_surface_mag = pi*cases.flux_sum(w, np.repeat(start_mag[:, None, :], angles, axis=1))
    shapes.close("linear flux", (what, "down"), got["down"], down.flux, down.flux_mag)
    shapes.close("linear flux", (what, "up"), got["up"], up.flux, up.flux_mag)
    shapes.close("linear flux", (what, "reflection"), got["reflection"], down.total,
                 down.total_mag)
    shapes.close("linear flux", (what, "surface"), got["surface"], at_surface, at_surface_mag)
    for key in got:
        if "@" in key:
            which = down if key.startswith("down") else up
            level = int(key.split("@")[1])
            shapes.close("linear flux", (what, key), got[key], which.rad[level],
                         which.rad_mag[level])


RUNS = ("uneven", "uneven mirrored", "deep", "ends mirrored")


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [False, True], ids=["positive", "mixed sign"])
def test_radiance_both_instantiations(engine, signed):
    """19 levels, both directions, with and without a boundary, per level and per path: the vector
    kernel meets the mirror; the scalar kernel and every run set give its bits, and the carry rows
    between runs meet the mirror.  beta of mixed sign: negative x, finite throughout."""
    n = 2*cases.PATH_AHEAD + 3
    problem = problem_for(n, 500 + signed, signed)
    sets = cases.run_sets(n, cases.PATH_AHEAD)
    with Grid(engine, problem.nu) as grid:
        for from_last in (False, True):
            for cumulative, boundary in ((True, True), (False, not from_last)):
                what = (signed, from_last, cumulative, boundary)
                base = run_radiance(engine, grid, problem, VECTOR, sets["whole"], from_last,
                                    cumulative, boundary)
                assert np.all(np.isfinite(base["rad"]))
                assert np.all(base["rad"][:, 0] == 0.)        # nu = 0: no source
                check_radiance(what, base, problem, from_last, cumulative, boundary)
                scalar = run_radiance(engine, grid, problem, SCALAR, sets["whole"], from_last,
                                      cumulative, boundary)
                assert same_bits(scalar["rad"], base["rad"]), what
                for layout in LAYOUTS:
                    for name in RUNS:
                        got = run_radiance(engine, grid, problem, layout, sets[name], from_last,
                                           cumulative, boundary)
                        assert same_bits(got["rad"], base["rad"]), (what, layout.name, name)
                        assert any("@" in key for key in got)
                        check_radiance((what, layout.name, name), got, problem, from_last,
                                       cumulative, boundary)
    print("worst error / bound so far:", shapes.WORST)


def test_nu_zero_column_has_no_source(engine):
    n = 2*cases.PATH_AHEAD + 3
    problem = problem_for(n, 520)
    with Grid(engine, problem.nu) as grid:
        got = run_radiance(engine, grid, problem, VECTOR, cases.run_sets(n)["whole"], False,
                           boundary=False)
    assert np.all(got["rad"][:, 0] == 0.) and np.any(got["rad"][:, 1:] > 0.)


@pytest.mark.parametrize("angles", cases.ANGLES)
def test_flux_every_angle_count(engine, angles):
    """K = 1..8 at two full batches and a remainder for that K, both surfaces (both directions of
    each sweep): the vector kernel meets the mirror, the scalar kernel and runs that cut paths
    give its bits.  K = 1 has w = 1: bit for bit the linear radiance."""
    n = cases.angle_levels(angles)
    problem = problem_for(n, 600 + angles, signed=angles == 3)
    sets = cases.run_sets(n, cases.flux_ahead(angles))
    with Grid(engine, problem.nu) as grid:
        for surface in ("first", "last"):
            base = run_flux(engine, grid, problem, VECTOR, sets["whole"], angles, surface)
            assert all(np.all(np.isfinite(v)) for v in base.values())
            check_flux((angles, surface), base, problem, angles, surface)
            for layout in LAYOUTS:
                for name in ("whole", "uneven", "deep mirrored"):
                    if layout is VECTOR and name == "whole":
                        continue
                    got = run_flux(engine, grid, problem, layout, sets[name], angles, surface)
                    for key in ("down", "up", "reflection", "surface"):
                        assert same_bits(got[key], base[key]), (angles, surface, layout.name,
                                                                name, key)
                    check_flux((angles, surface, layout.name, name),
                               {k: v for k, v in got.items() if "@" in k or k in base}, problem,
                               angles, surface)
        if angles == 1:
            lengths, weight = problem.lengths(1)
            assert weight[0] == 1.
            slant = problem_for(n, 600 + angles)
            slant.thickness = lengths[:, 0]
            for layout in LAYOUTS:
                for name in ("whole", "uneven"):
                    for surface in ("first", "last"):
                        from_last = surface == "first"      # the down sweep
                        flux = run_flux(engine, grid, problem, layout, sets[name], 1, surface)
                        rad = run_radiance(engine, grid, slant, layout, sets[name], from_last,
                                           boundary=False)
                        what = (layout.name, name, surface)
                        assert same_bits(flux["down"], cases.FLUX_PI*(1.*rad["rad"])), what
                        final = cases._flat(n, 0 if from_last else n - 1)
                        assert same_bits(flux["reflection"], rad["rad"][final]), what
                        for key in (k for k in rad if "@" in k):
                            assert same_bits(flux["down " + key][0], rad[key]), (what, key)
    print("worst error / bound so far:", shapes.WORST)


# ---------------------------------------------------------------------------------------------
# One-level paths on 515 columns: x is set per column.
def one_level_problem(x, thickness):
    """PATHS one-level paths whose row p has s*beta = x[p] (thickness[p] = 0: beta = 1)."""
    problem = cases.Problem(COLUMNS, 1, seed=700)
    problem.nu = np.linspace(400., 1200., COLUMNS)
    problem.thickness = np.asarray(thickness, dtype=F64)
    x = np.asarray(x, dtype=F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        problem.beta = np.where(problem.thickness[:, None] > 0.,
                                x/problem.thickness[:, None], 1.)
    problem.interfaces = np.tile([250., 300.], (PATHS, 1))
    problem.edges = linear.edge_table(problem.interfaces)
    return problem


@pytest.mark.parametrize("layout", LAYOUTS, ids=[x.name for x in LAYOUTS])
def test_zero_and_thin_layers(engine, layout):
    """One-level paths, no boundary, edges 250 K and 300 K.  Path 0: x log-spaced from 1e-12 to
    1e-3 with every fifth column beta = 0; path 1: s = 0; path 2: x = 1e-12 exactly and 1e-3.
    I_in = 0, so the result is the source term alone and the bound (|B_in| + |B_out|)*|a|*1e-12
    is relative to about twice the result: 1 - a/x formed directly is wrong by 1e-4 relative at
    x = 1e-12 and NaN at x = 0.  Then the same rows behind a boundary: x = 0 leaves I bit for bit
    what the isothermal kernel leaves at x = 0, which is I itself."""
    x = np.ones((PATHS, COLUMNS))
    x[0] = 10.**np.linspace(-12., -3., COLUMNS)
    x[0, ::5] = 0.
    x[2] = np.where(np.arange(COLUMNS) % 2 == 0, 1e-12, 1e-3)
    problem = one_level_problem(x, [1., 0., 4.])
    assert np.all(problem.thickness[:, None]*problem.beta == np.where([[1], [0], [1]], x, 0.))
    runs = [(0, PATHS)]
    with Grid(engine, problem.nu) as grid:
        for from_last in (False, True):
            got = run_radiance(engine, grid, problem, layout, runs, from_last, boundary=False)
            rad = got["rad"]
            assert np.all(np.isfinite(rad))
            zero = problem.thickness[:, None]*problem.beta == 0.
            assert np.count_nonzero(zero) > COLUMNS
            assert same_bits(rad[zero], np.zeros(np.count_nonzero(zero)))
            assert np.all(rad[~zero] > 0.)
            check_radiance(("thin", layout.name, from_last), got, problem, from_last,
                           boundary=False)
            # The thin limit x*(B_in + B_out)/2, to first order in x.
            b = cases.planck(LD, problem.nu, LD(250.)) + cases.planck(LD, problem.nu, LD(300.))
            thin = (x[0] > 0.) & (x[0] < 1e-9)
            assert np.allclose(rad[0][thin], (x[0]*b/2)[thin].astype(F64), rtol=1e-8, atol=0.)

            problem.boundary_t = np.array([280., 288., 215.])
            problem.boundary_e = np.array([1., 0.9, 0.5])
            behind = run_radiance(engine, grid, problem, layout, runs, from_last)
            isothermal = run_radiance(engine, grid, problem, layout, runs, from_last,
                                      edges=False)
            assert np.all(behind["rad"][zero] > 0.)
            assert same_bits(behind["rad"][zero], isothermal["rad"][zero])
            check_radiance(("thin behind a boundary", layout.name, from_last), behind, problem,
                           from_last)
            problem.__dict__.pop("_sweeps")
    print("worst error / bound so far:", shapes.WORST)


def test_saturating_layers(engine):
    """x = 50 and x = 700 (exp(-700) is 1e-304, a = 1): I tends to B_out - (B_out - B_in)/x
    whatever came in."""
    x = np.ones((PATHS, COLUMNS))
    x[0], x[1] = 50., 700.
    x[2] = np.where(np.arange(COLUMNS) % 2 == 0, 50., 700.)
    problem = one_level_problem(x, [1., 2., 0.5])
    problem.boundary_t = np.array([0., 288., 320.])
    with Grid(engine, problem.nu) as grid:
        for layout in LAYOUTS:
            for from_last in (False, True):
                got = run_radiance(engine, grid, problem, layout, [(0, PATHS)], from_last)
                check_radiance(("saturated", layout.name, from_last), got, problem, from_last)
                t_in, t_out = (300., 250.) if from_last else (250., 300.)
                b_in = cases.planck(LD, problem.nu, LD(t_in))
                b_out = cases.planck(LD, problem.nu, LD(t_out))
                limit = (b_out - (b_out - b_in)/LD(700.)).astype(F64)
                assert np.allclose(got["rad"][1], limit, rtol=1e-13, atol=0.)
                problem.__dict__.pop("_sweeps")


# ---------------------------------------------------------------------------------------------
def test_bad_edge_tables_are_refused_and_the_engine_stays_usable(engine):
    n = 5
    problem = cases.Problem(COLUMNS, n, seed=800)
    problem.interfaces = linear.interfaces_for(problem, 801)
    problem.edges = linear.edge_table(problem.interfaces)
    whole = [(0, problem.levels)]
    good = problem.edges

    def spoiled(row, side, value):
        edges = good.copy()
        edges[row, side] = value
        return edges
    bad = {"nan": spoiled(3, 0, np.nan), "inf": spoiled(14, 1, np.inf),
           "zero": spoiled(0, 0, 0.), "negative": spoiled(7, 1, -250.)}
    # Continuity is checked inside a path only: rows 4 and 5 belong to paths 0 and 1.
    gap_inside = spoiled(2, 1, good[2, 1] + 1.)
    assert good[4, 1] != good[5, 0]
    with Grid(engine, problem.nu) as grid:
        base = run_radiance(engine, grid, problem, VECTOR, whole, False)
        for name, edges in list(bad.items()) + [("discontinuous", gap_inside)]:
            problem.edges = edges
            expect = "continuous" if name == "discontinuous" else "finite and > 0"
            with pytest.raises(EngineError, match=expect):
                run_radiance(engine, grid, problem, VECTOR, whole, False)
            with pytest.raises(EngineError, match=expect):
                run_flux(engine, grid, problem, VECTOR, whole, 3, "last")
            with pytest.raises(EngineError, match="lbl_path_flux_source"):
                run_flux(engine, grid, problem, SCALAR, whole, 3, "first")
        # A run that ends where the table breaks does not see the break: the next run's own
        # table starts the level.
        problem.edges = gap_inside
        run_radiance(engine, grid, problem, VECTOR, [(0, 3), (3, problem.levels - 3)], False)
        with pytest.raises(EngineError, match="continuous"):
            run_radiance(engine, grid, problem, VECTOR, [(0, 4), (4, problem.levels - 4)], False)
        with pytest.raises(ValueError, match="edge_temperature"):
            problem.edges = good[:, :1]
            run_radiance(engine, grid, problem, VECTOR, whole, False)
        problem.edges = good
        again = run_radiance(engine, grid, problem, VECTOR, whole, False)
        assert same_bits(again["rad"], base["rad"])
        check_radiance("after the refusals", again, problem, False)

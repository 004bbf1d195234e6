"""lbl_path_jacobian fed directly (Engine.path_jacobian on rows held in torch tensors), in the
manner of tests/test_gpu_sweep_shapes.py: both instantiations (aligned even strides; odd strides
and bases 8 bytes off), one-column tail lanes, NaN padding, every depth of the two rows-in-flight
loops, both directions, several paths per launch, every subset of the quantities, band means, the
extreme values of sweep_cases.value_problem, and the calls the entry rejects.

Bounds against the long-double mirror of tests/jacobian_cases.py, none taken from the code under
test: the project's 1e-12 applied to the magnitude each result is formed from --
|dK_x| <= 1e-12*(|B_k| + |I_k|)*trail_k (B_k - I_k cancels in opaque layers), the same times |x_k|
for the log form, 1e-12 relative for the temperature and boundary Jacobians.  The radiance is
lbl_path_radiance's bit for bit; layouts, launches and subsets of one case give the same bits."""
from itertools import combinations

import numpy as np
import pytest

from tests import jacobian_cases as jac
from tests import sweep_cases as cases
from tests.test_gpu_sweep_shapes import (Grid, Rows, block, close, ordered, plain, read,
                                         same_bits, small_bands)

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
LBL_BAD_ARGUMENT = 2


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


def run_jacobian(engine, grid, problem, layout, from_last=False, quantities=jac.OUTPUTS,
                 launches=None, bands=None, in_place=None, boundary=True):
    """{quantity: rows on the host} of the calls `launches` [(first level, count)] (None: one)."""
    n, columns, levels = problem.levels_per_path, problem.columns, problem.levels
    beta = block(problem.beta, levels, columns, layout, np.nan)
    outputs = {}
    for q in jac.OUTPUTS:
        rows = levels if q in jac.PER_LEVEL else PATHS
        outputs[q] = plain(rows, bands.size - 1) if bands is not None else \
            block(None, rows, columns, layout, SENTINEL)
    work_rows = levels if bands is None else 3*levels + 3*PATHS
    work = outputs[in_place] if in_place else block(None, work_rows, columns, layout, SENTINEL)
    ordered(engine)
    for first, count in launches or [(0, levels)]:
        part = slice(first, first + count)
        given = {q: Rows(outputs[q][part] if q in jac.PER_LEVEL else outputs[q])
                 for q in quantities}
        engine.path_jacobian(
            Rows(beta[part]), columns, grid, PATHS, n, first, problem.thickness[part],
            problem.temperature[part], Rows(work[part] if in_place else work),
            boundary_temperature=problem.boundary_t if boundary else None,
            boundary_emissivity=problem.boundary_e if boundary else None,
            band_start=bands, from_last=from_last, **given)
        engine.synchronize()
    assert np.array_equal(read(beta)[:, :columns], problem.beta), "beta was written"
    got = {q: read(outputs[q], None if bands is not None else columns) for q in jac.OUTPUTS}
    for q in jac.OUTPUTS:
        if q not in quantities:
            assert np.all(got[q] == SENTINEL), ("an output that was not requested was written", q)
    return {q: got[q] for q in quantities}


def mirror(problem, from_last, boundary=True):
    store = problem.__dict__.setdefault("_jacobians", {})
    key = (from_last, boundary)
    if key not in store:
        store[key] = jac.jacobian(
            LD, problem.nu, problem.beta, problem.thickness, problem.temperature,
            problem.levels_per_path, from_last, problem.boundary_t if boundary else None,
            problem.boundary_e if boundary else None)
    return store[key]


def check(what, got, problem, from_last, boundary=True, bands=None):
    values, magnitudes = mirror(problem, from_last, boundary)
    for q, rows in got.items():
        reference, magnitude = values[q], magnitudes[q]
        if bands is not None:
            reference = cases.band_means(LD, reference, bands)
            magnitude = cases.band_means(LD, magnitude, bands)
        close("jacobian " + q, (what, q), rows, reference, magnitude)


def assert_same(got, base, what):
    assert set(got) <= set(base) and got, what
    for q in got:
        assert same_bits(got[q], base[q]), (what, q)


def with_boundaries(problem):
    """Every path behind a boundary, so that the boundary Jacobians can be asked for."""
    problem.boundary_t = np.array([301., 288., 215.])
    problem.boundary_e = np.array([1., 0.9, 0.])
    return problem


@pytest.mark.parametrize("from_last", [False, True])
@pytest.mark.parametrize("columns", cases.COLUMNS)
def test_columns_and_layouts(engine, columns, from_last):
    """19 levels per path (beyond twice the rows in flight of both loops) on 1 to 8193 columns:
    the aligned layout (the vector kernel) meets the reference; stride = columns, NaN padding, a
    base 8 bytes off and an odd stride (the scalar kernel, one-column tail lanes) give its bits,
    and the padding of every output stays untouched."""
    problem = with_boundaries(cases.Problem(columns, 19, seed=300 + columns))
    assert cases.layout_is_vector("aligned", columns)
    with Grid(engine, problem.nu) as grid:
        base = run_jacobian(engine, grid, problem, "aligned", from_last)
        check((columns, from_last), base, problem, from_last)
        layouts = [x for x in cases.LAYOUTS if x != "aligned"] \
            if columns in cases.LAYOUT_COLUMNS else []
        scalar = 0
        for layout in layouts:
            scalar += not cases.layout_is_vector(layout, columns)
            assert_same(run_jacobian(engine, grid, problem, layout, from_last), base,
                        (columns, layout))
        assert not layouts or scalar >= 2


DEPTHS = jac.DEPTHS     # tests/test_jacobian_host.py: they reach every loop of both depths


@pytest.mark.parametrize("from_last", [False, True])
@pytest.mark.parametrize("n", DEPTHS)
def test_depths_and_launches(engine, n, from_last):
    """Every depth of the two loops on 1031 columns (a one-column tail lane), vector and scalar;
    one path per call, two calls, and a call that starts at path 1 give the bits of the call
    with all three paths."""
    problem = with_boundaries(cases.Problem(1031, n, seed=400 + n))
    with Grid(engine, problem.nu) as grid:
        base = run_jacobian(engine, grid, problem, "aligned", from_last)
        check((n, from_last), base, problem, from_last)
        assert_same(run_jacobian(engine, grid, problem, "odd", from_last), base, (n, "odd"))
        for launches in ([(0, n), (n, n), (2*n, n)], [(n, 2*n), (0, n)], [(2*n, n), (0, 2*n)]):
            assert_same(run_jacobian(engine, grid, problem, "aligned", from_last,
                                     launches=launches), base, (n, launches))


@pytest.mark.parametrize("from_last", [False, True])
def test_radiance_is_path_radiance_bit_for_bit(engine, from_last):
    from tests.test_gpu_sweep_shapes import run_radiance
    for problem in (cases.Problem(1031, 19, seed=21), cases.value_problem()):
        runs = [(0, problem.levels)]
        with Grid(engine, problem.nu) as grid:
            for layout in ("aligned", "odd"):
                expect = run_radiance(engine, grid, problem, layout, runs, "per path", from_last)
                got = run_jacobian(engine, grid, problem, layout, from_last,
                                   quantities=("radiance", "temperature_jacobian"))
                assert same_bits(got["radiance"], expect["rad"]), (layout, from_last)


SUBSETS = [subset for size in range(1, len(jac.OUTPUTS) + 1)
           for subset in combinations(jac.OUTPUTS, size)]


@pytest.mark.parametrize("layout", ["aligned", "odd"])
def test_every_subset_of_quantities(engine, layout):
    """All 63 selections: what is requested has the bits of the call with everything, what is
    not requested is not written."""
    assert len(SUBSETS) == 63
    problem = with_boundaries(cases.Problem(131, 9, seed=9))
    with Grid(engine, problem.nu) as grid:
        base = run_jacobian(engine, grid, problem, layout, True)
        check("all", base, problem, True)
        for subset in SUBSETS:
            assert_same(run_jacobian(engine, grid, problem, layout, True, quantities=subset),
                        base, subset)


@pytest.mark.parametrize("in_place", ["optical_depth_jacobian", "log_optical_depth_jacobian"])
def test_work_block_in_place(engine, in_place):
    """dI/dx or dI/dln x written over the work block give the bits of separate blocks."""
    problem = with_boundaries(cases.Problem(513, 19, seed=31))
    with Grid(engine, problem.nu) as grid:
        for from_last in (False, True):
            base = run_jacobian(engine, grid, problem, "aligned", from_last)
            for layout in ("aligned", "odd"):
                assert_same(run_jacobian(engine, grid, problem, layout, from_last,
                                         in_place=in_place), base, (in_place, layout))


@pytest.mark.parametrize("from_last", [False, True])
def test_extreme_values(engine, from_last):
    """sweep_cases.value_problem: beta = 0, s = 0, saturating layers, beta of mixed sign, nu = 0,
    Planck arguments that overflow expm1, 1 K and 5 K boundaries -- the reference's values and
    its pattern of zeros, never NaN or inf."""
    problem = cases.value_problem()
    with Grid(engine, problem.nu) as grid:
        for boundary in (True, False):
            if boundary:
                # Path 0 has no boundary: the boundary Jacobians of paths 1 and 2 alone.
                first = run_jacobian(engine, grid, problem, "aligned", from_last,
                                     quantities=("radiance",) + jac.PER_LEVEL,
                                     launches=[(0, 9)])
                rest = run_jacobian(engine, grid, problem, "aligned", from_last,
                                    launches=[(9, 18)])
                got = {}
                for q in jac.OUTPUTS:
                    if q in jac.PER_LEVEL:
                        got[q] = np.concatenate([first[q][:9], rest[q][9:]])
                    elif q == "radiance":
                        got[q] = np.concatenate([first[q][:1], rest[q][1:]])
                    else:
                        assert np.all(rest[q][0] == SENTINEL)
                        got[q] = np.concatenate([np.zeros((1, problem.columns)), rest[q][1:]])
            else:
                got = run_jacobian(engine, grid, problem, "aligned", from_last,
                                   quantities=("radiance",) + jac.PER_LEVEL, boundary=False)
            check(("values", boundary), got, problem, from_last, boundary)
            values, _ = mirror(problem, from_last, boundary)
            for q in got:
                assert np.all(np.isfinite(got[q])), q
                assert cases.same_pattern(got[q], cases.flushed(values[q])), q
            zero = problem.group == 0
            assert np.all(got["temperature_jacobian"][:, zero] == 0.)
            assert np.all(got["log_optical_depth_jacobian"][:, zero] == 0.)
            assert np.all(got["temperature_jacobian"][12] == 0.)        # s = 0


@pytest.mark.parametrize("name,columns,bands", cases.BAND_SETS)
def test_band_means(engine, name, columns, bands):
    problem = with_boundaries(cases.Problem(columns, 9, seed=50 + columns))
    with Grid(engine, problem.nu) as grid:
        for from_last in (False, True):
            base = run_jacobian(engine, grid, problem, "aligned", from_last, bands=bands)
            check((name, from_last), base, problem, from_last, bands=bands)
            assert_same(run_jacobian(engine, grid, problem, "odd", from_last, bands=bands), base,
                        (name, "odd"))
            assert_same(run_jacobian(engine, grid, problem, "aligned", from_last, bands=bands,
                                     launches=[(9, 18), (0, 9)]), base, (name, "launches"))
            for subset in (("temperature_jacobian",), ("radiance", "log_optical_depth_jacobian"),
                           ("boundary_emissivity_jacobian",)):
                assert_same(run_jacobian(engine, grid, problem, "aligned", from_last,
                                         bands=bands, quantities=subset), base, (name, subset))


def test_small_bands(engine):
    problem = with_boundaries(cases.Problem(67, 5, seed=8))
    bands = small_bands(67)
    with Grid(engine, problem.nu) as grid:
        check("small bands", run_jacobian(engine, grid, problem, "aligned", bands=bands), problem,
              False, bands=bands)


# ---------------------------------------------------------------------------------------------
# Rejected calls.
def raw_call(engine, handle, problem, tensors, **changes):
    """lbl_path_jacobian itself with every argument valid but `changes`: (status, message)."""
    from pylbl_amd import engine as module
    n, columns, levels = problem.levels_per_path, problem.columns, problem.levels
    every = 0
    for _, flag in module.PATH_JACOBIAN_OUTPUTS:
        every |= flag
    a = dict(beta=tensors["beta"].data_ptr(), row_stride=tensors["beta"].shape[1],
             columns=columns, grid=handle, n_paths=PATHS, levels_per_path=n, level_begin=0,
             level_count=levels, path_length=problem.thickness, temperature=problem.temperature,
             boundary_temperature=problem.boundary_t, boundary_emissivity=problem.boundary_e,
             n_bands=0, band_start=None, work=tensors["work"].data_ptr(), flags=every)
    a.update({q: tensors[q].data_ptr() for q in jac.OUTPUTS})
    a.update(changes)
    host = {k: np.ascontiguousarray(a[k], dtype=F64) if a[k] is not None else None
            for k in ("path_length", "temperature", "boundary_temperature",
                      "boundary_emissivity")}
    pointer = lambda x: None if x is None else x.ctypes.data
    status = engine.lib.lbl_path_jacobian(
        engine.handle, a["beta"], a["row_stride"], a["columns"], a["grid"], a["n_paths"],
        a["levels_per_path"], a["level_begin"], a["level_count"], pointer(host["path_length"]),
        pointer(host["temperature"]), pointer(host["boundary_temperature"]),
        pointer(host["boundary_emissivity"]), a["n_bands"], pointer(a["band_start"]), a["work"],
        *(a[q] for q in jac.OUTPUTS), a["flags"])
    message = engine.lib.lbl_last_error(engine.handle).decode() if status else ""
    return status, message


def test_rejected_calls_launch_nothing(engine):
    from pylbl_amd import engine as module
    problem = with_boundaries(cases.Problem(67, 9, seed=3))
    levels = problem.levels
    tensors = {"beta": block(problem.beta, levels, 67, "aligned", np.nan),
               "work": block(None, levels, 67, "aligned", SENTINEL)}
    for q in jac.OUTPUTS:
        tensors[q] = block(None, levels if q in jac.PER_LEVEL else PATHS, 67, "aligned", SENTINEL)
    every = 0
    for _, flag in module.PATH_JACOBIAN_OUTPUTS:
        every |= flag
    no_boundary = problem.boundary_t.copy()
    no_boundary[1] = 0.
    rejected = {
        "level_begin inside a path": dict(level_begin=3, level_count=9),
        "level_count not whole paths": dict(level_count=13),
        "LBL_PATH_CONTINUE": dict(flags=every | module.PATH_CONTINUE),
        "LBL_PATH_CUMULATIVE": dict(flags=every | module.PATH_CUMULATIVE),
        "boundary Jacobian without a boundary": dict(boundary_temperature=no_boundary),
        "boundary Jacobian, no boundaries at all": dict(boundary_temperature=None),
        "requested output NULL": dict(temperature_jacobian=None),
        "requested radiance NULL": dict(radiance=None),
        "no quantity": dict(flags=module.PATH_FROM_LAST),
        "work NULL": dict(work=None),
        "beta NULL": dict(beta=None),
        "unknown grid": dict(grid=12345),
        "columns > stride": dict(columns=69),
        "run outside the levels": dict(level_begin=18, level_count=18),
        "negative length": dict(path_length=-problem.thickness),
        "zero temperature": dict(temperature=np.zeros(levels)),
        "negative boundary": dict(boundary_temperature=-problem.boundary_t),
        "emissivity above 1": dict(boundary_emissivity=problem.boundary_e + 1.),
        "bands without starts": dict(n_bands=2),
        "temperature Jacobian over work": dict(temperature_jacobian=tensors["work"].data_ptr()),
        "both depth Jacobians over work": dict(
            optical_depth_jacobian=tensors["work"].data_ptr(),
            log_optical_depth_jacobian=tensors["work"].data_ptr()),
    }
    with Grid(engine, problem.nu) as grid:
        ordered(engine)
        for what, changes in rejected.items():
            status, message = raw_call(engine, grid, problem, tensors, **changes)
            assert status == LBL_BAD_ARGUMENT, (what, status)
            assert message.startswith("lbl_path_jacobian: ") and len(message) > 25, (what, message)
        engine.synchronize()
        for name, tensor in tensors.items():
            if name != "beta":
                assert np.all(read(tensor) == SENTINEL), ("a rejected call wrote", name)
        # The engine stays usable, and the valid call passes the same route.
        status, message = raw_call(engine, grid, problem, tensors)
        assert status == 0, message
        engine.synchronize()
        got = {q: read(tensors[q], 67) for q in jac.OUTPUTS}
        check("after the rejected calls", got, problem, False)

"""Every refusal of the eight path entries, in the order their bodies check, with the message the
entry gives, and after them one good call per entry on the same engine.

The entries are called through the library (Engine.lib), because Engine's own checks refuse most
of these calls first.  Each bad call differs from a good one in what its check looks at, so every
earlier check passes and the first failing check decides the message.  The expected messages are
the entries' texts as they stood before the entries shared their helpers; they are not read from
the code under test.  All refusals happen before anything is queued.

Shapes: 2 paths of 3 levels (the first two of tests/sweep_cases.py's three, whose mirrors the
good calls are compared with): 8 columns in an aligned and in an unaligned block, 10 columns with
an odd stride -- the vector kernels and both reasons for the scalar ones."""
import numpy as np
import pytest

from tests import jacobian_cases as jac
from tests import solar_cases as solar
from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests.test_gpu_sweep_shapes import Grid, block, close, ordered, plain, read, same_bits

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
P, N = 2, 3                     # paths and levels per path of every call
LEVELS = P*N
SENTINEL = cases.SENTINEL
BAD_ARGUMENT = 2                # LBL_BAD_ARGUMENT
OPTICAL_DEPTH, TRANSMITTANCE, CUMULATIVE, FROM_LAST, CONTINUE = 0x100, 0x200, 0x400, 0x800, 0x1000
RADIANCE, BRIGHTNESS, FLUX_UP = 0x2000, 0x4000, 0x8000
JACOBIAN_DEPTH, JACOBIAN_LOG_DEPTH, JACOBIAN_TEMPERATURE = 0x10000, 0x20000, 0x40000
JACOBIAN_BOUNDARY_T, JACOBIAN_BOUNDARY_E = 0x80000, 0x100000


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


def test_the_flag_values_are_the_engine_module_s():
    from pylbl_amd import engine as module
    assert (OPTICAL_DEPTH, TRANSMITTANCE, CUMULATIVE, FROM_LAST, CONTINUE, RADIANCE, BRIGHTNESS,
            FLUX_UP) == (module.PATH_OPTICAL_DEPTH, module.PATH_TRANSMITTANCE,
                         module.PATH_CUMULATIVE, module.PATH_FROM_LAST, module.PATH_CONTINUE,
                         module.PATH_RADIANCE, module.PATH_BRIGHTNESS, module.PATH_FLUX_UP)
    flags = dict(module.PATH_JACOBIAN_OUTPUTS)
    assert flags == {"radiance": RADIANCE, "optical_depth_jacobian": JACOBIAN_DEPTH,
                     "log_optical_depth_jacobian": JACOBIAN_LOG_DEPTH,
                     "temperature_jacobian": JACOBIAN_TEMPERATURE,
                     "boundary_temperature_jacobian": JACOBIAN_BOUNDARY_T,
                     "boundary_emissivity_jacobian": JACOBIAN_BOUNDARY_E}


def address(value):
    if value is None:
        return None
    if isinstance(value, np.ndarray):
        assert value.flags["C_CONTIGUOUS"] and value.dtype in (np.float64, np.int64)
        return value.ctypes.data
    return value.data_ptr()         # a torch tensor


def call(engine, name, arguments):
    """(status, message) of the entry `name` given `arguments` in the header's order: numbers as
    they are, numpy arrays and torch tensors by address (held by `arguments` during the call)."""
    values = [v if isinstance(v, (int, float)) else address(v) for v in arguments.values()]
    status = getattr(engine.lib, name)(engine.handle, *values)
    return status, engine.lib.lbl_last_error(engine.handle).decode()


def refused(engine, name, good, cases_):
    """Every (changes, message) of `cases_` is refused with exactly `name: message`; returns the
    number of calls made."""
    for changes, message in cases_:
        assert set(changes) <= set(good), (name, set(changes) - set(good))
        status, text = call(engine, name, dict(good, **changes))
        assert status == BAD_ARGUMENT and text == "%s: %s" % (name, message), (message, text)
    return len(cases_)


class Scene(object):
    """The blocks of the calls on `columns` columns in `layout`, and a grid handle."""
    def __init__(self, engine, grid, columns, layout):
        self.problem = problem = cases.Problem(columns, N, seed=4000 + columns)
        self.columns, self.layout, self.grid = columns, layout, grid
        self.stride = cases.LAYOUTS[layout].stride(columns)
        self.beta = block(problem.beta[:LEVELS], LEVELS, columns, layout, np.nan)
        self.lengths = np.ascontiguousarray(problem.thickness[:LEVELS])
        self.temperature = np.ascontiguousarray(problem.temperature[:LEVELS])
        self.boundary_t = np.ascontiguousarray(problem.boundary_t[:P])
        self.boundary_e = np.ascontiguousarray(problem.boundary_e[:P])

    def rows(self, count):
        return block(None, count, self.columns, self.layout, SENTINEL)

    def run(self, **more):
        """The arguments every sweep has, in the header's order up to level_count."""
        return dict(beta=self.beta, row_stride=self.stride, columns=self.columns, **more,
                    n_paths=P, levels_per_path=N, level_begin=0, level_count=LEVELS)


BANDS = np.array([0, 3, 8], dtype=np.int64)
BAD_BANDS = np.array([0, 5, 3], dtype=np.int64)


# ---------------------------------------------------------------------------------------------
def path_compute_arguments(s):
    return dict(s.run(), path_length=s.lengths, n_bands=0, band_start=None, carry=s.rows(P),
                optical_depth=s.rows(P), transmittance=None, flags=OPTICAL_DEPTH)


def refuse_path_compute(engine, s):
    good = path_compute_arguments(s)
    return refused(engine, "lbl_path_compute", good, [
        (dict(carry=None), "beta, path_length and carry must not be NULL."),
        (dict(flags=0), "no quantity requested."),
        (dict(flags=OPTICAL_DEPTH | TRANSMITTANCE), "an output requested by the flags is NULL."),
        (dict(flags=OPTICAL_DEPTH | FROM_LAST), "LBL_PATH_FROM_LAST needs LBL_PATH_CUMULATIVE."),
        (dict(level_count=LEVELS + 1),
         "the run [level_begin, level_begin + level_count) is not inside the levels."),
        (dict(n_bands=2, band_start=BAD_BANDS), "band_start must not decrease."),
    ])


def good_path_compute(engine, s):
    arguments = path_compute_arguments(s)
    ordered(engine)
    assert call(engine, "lbl_path_compute", arguments)[0] == 0
    engine.synchronize()
    loop, _ = cases.sweep_tau(F64, s.problem.beta, s.problem.thickness, N)
    assert same_bits(read(arguments["optical_depth"], s.columns), loop[cases._flat(N, N - 1)[:P]])


# ---------------------------------------------------------------------------------------------
def radiance_arguments(s, surface_entry, e_rows=None):
    arguments = dict(
        s.run(grid=s.grid), path_length=s.lengths, temperature=s.temperature,
        edge_temperature=None, boundary_temperature=s.boundary_t,
        boundary_emissivity=s.boundary_e, n_bands=0, band_start=None, carry=s.rows(P),
        radiance=s.rows(P), brightness_temperature=None, flags=RADIANCE)
    if surface_entry:
        arguments.update(emissivity_rows=e_rows, reflection=None)
    return arguments


def refuse_radiance(engine, s, surface_entry):
    name = "lbl_path_radiance_surface" if surface_entry else "lbl_path_radiance_source"
    good = radiance_arguments(s, surface_entry)
    edges = np.full((LEVELS, 2), 250.)
    edges[0, 1] = 251.          # level 0's far side is not level 1's near side
    listed = [
        (dict(temperature=None), "beta, path_length, temperature and carry must not be NULL."),
        (dict(flags=0), "no quantity requested."),
        (dict(flags=RADIANCE | BRIGHTNESS), "an output requested by the flags is NULL."),
        (dict(flags=RADIANCE | BRIGHTNESS, brightness_temperature=s.rows(P), n_bands=2,
              band_start=BANDS), "brightness temperature has no band means."),
        (dict(grid=-5), "unknown grid handle."),
        (dict(flags=RADIANCE | CONTINUE),
         "the run starts a path: LBL_PATH_CONTINUE must not be set."),
        (dict(temperature=np.array([250., 0., 250., 250., 250., 250.])),
         "temperatures must be finite and > 0."),
        (dict(edge_temperature=edges),
         "edge temperatures must be continuous within a path: [r][1] == [r + 1][0]."),
        (dict(boundary_temperature=np.array([288., -1.])),
         "boundary temperatures must be finite and >= 0 (0: no boundary)."),
        (dict(boundary_emissivity=np.array([1., 1.5])),
         "boundary emissivities must lie in [0, 1]."),
        (dict(n_bands=-1), "n_bands < 0, or band_start is NULL."),
    ]
    if surface_entry:
        # (the problem's path 0 has no boundary: boundary temperature 0)
        listed.append((dict(reflection=s.rows(P)),
                       "a reflecting surface needs a boundary temperature > 0 for every path "
                       "of the run."))
    return refused(engine, name, good, listed)


def good_radiance(engine, s):
    """lbl_surface_emissivity, then lbl_path_radiance_surface behind its rows, and
    lbl_path_radiance_source with the scalar emissivities."""
    problem, nu = s.problem, s.problem.nu
    knots = np.array([nu[1], nu[4], nu[7]])
    values = np.array([[0.625, 0.625, 0.625], [0.2, 0.9, 0.4]])
    e_rows = s.rows(P)
    fill = dict(grid=s.grid, n_paths=P, path_begin=0, path_count=P, n_knots=3,
                knot_wavenumber=knots, knot_emissivity=values, rows=e_rows,
                row_stride=s.stride, flags=0)
    ordered(engine)
    assert call(engine, "lbl_surface_emissivity", fill)[0] == 0
    engine.synchronize()
    e = read(e_rows, s.columns)
    assert same_bits(e, surface.emissivity(F64, knots, values, nu))
    assert np.all(e[0] == 0.625)

    rows = cases._flat(N, N - 1)[:P]
    for surface_entry in (False, True):
        arguments = radiance_arguments(s, surface_entry, e_rows)
        name = "lbl_path_radiance_surface" if surface_entry else "lbl_path_radiance_source"
        ordered(engine)
        assert call(engine, name, arguments)[0] == 0
        engine.synchronize()
        emissivity = np.ones((cases.PATHS, s.columns))
        emissivity[:P] = e if surface_entry else problem.boundary_e[:P, None]
        start, start_mag = surface.surface_start(LD, nu, problem.boundary_t, emissivity, None,
                                                 None)
        rad, mag = surface.restart(LD, problem, problem.thickness, False, start, start_mag, None)
        close("radiance", name, read(arguments["radiance"], s.columns), rad[rows], mag[rows])


# ---------------------------------------------------------------------------------------------
def refuse_surface_emissivity(engine, s):
    knots = np.array([10., 20., 30.])
    values = np.full((P, 3), 0.5)
    good = dict(grid=s.grid, n_paths=P, path_begin=0, path_count=P, n_knots=3,
                knot_wavenumber=knots, knot_emissivity=values, rows=s.rows(P),
                row_stride=s.stride, flags=0)
    return refused(engine, "lbl_surface_emissivity", good, [
        (dict(rows=None), "knot_wavenumber, knot_emissivity and rows must not be NULL."),
        (dict(grid=-5), "unknown grid handle."),
        (dict(row_stride=s.columns - 1), "row_stride is less than the grid's points."),
        (dict(path_count=P + 1),
         "the paths [path_begin, path_begin + path_count) are not inside n_paths."),
        (dict(n_knots=1), "n_knots must lie in 2..1024."),
        (dict(knot_wavenumber=np.array([10., 10., 30.])),
         "knots must be finite and strictly ascending."),
        (dict(knot_emissivity=np.full((P, 3), 1.25)), "emissivities must lie in [0, 1]."),
    ])


# ---------------------------------------------------------------------------------------------
def flux_arguments(s, angles=2):
    lengths, weight = s.problem.lengths(angles)
    return dict(
        s.run(grid=s.grid), n_angles=angles, path_length=np.ascontiguousarray(lengths[:LEVELS]),
        weight=np.ascontiguousarray(weight), temperature=s.temperature, edge_temperature=None,
        surface_temperature=None, surface_emissivity=None, n_bands=0, band_start=None,
        carry=s.rows(P*angles), reflection=s.rows(P), level_flux=s.rows(LEVELS), flux=None,
        surface_flux=None, flags=0)


def refuse_flux(engine, s):
    good = flux_arguments(s)
    surface_t = np.ascontiguousarray(s.problem.surface_t[:P])
    surface_e = np.ascontiguousarray(s.problem.surface_e[:P])
    up = dict(flags=FLUX_UP | FROM_LAST, surface_temperature=surface_t,
              surface_emissivity=surface_e)
    edges = np.full((LEVELS, 2), 250.)
    edges[3, 0] = np.inf
    return refused(engine, "lbl_path_flux_source", good, [
        (dict(weight=None), "beta, path_length, weight, temperature, carry, reflection and "
                            "level_flux must not be NULL."),
        (dict(level_flux=s.beta), "level_flux must not be beta: the up sweep reads it."),
        (dict(flags=FLUX_UP | FROM_LAST),
         "the up sweep needs surface_temperature and surface_emissivity."),
        (dict(n_angles=9), "need 1 <= n_angles <= 8."),
        (dict(n_angles=0), "need 1 <= n_angles <= 8."),
        (dict(grid=-5), "unknown grid handle."),
        (dict(level_begin=-1),
         "the run [level_begin, level_begin + level_count) is not inside the levels."),
        (dict(weight=np.array([0.5, -0.5])), "weights must be finite and >= 0."),
        (dict(temperature=np.full(LEVELS, np.nan)), "temperatures must be finite and > 0."),
        (dict(edge_temperature=edges), "edge temperatures must be finite and > 0."),
        (dict(up, surface_temperature=np.array([288., 0.])),
         "surface temperatures must be finite and > 0."),
        (dict(up, surface_emissivity=np.array([-0.1, 1.])),
         "surface emissivities must lie in [0, 1]."),
        (dict(n_bands=2, band_start=np.array([0, 3, s.columns + 1], dtype=np.int64)),
         "band_start out of [0, columns]."),
        (dict(n_bands=2, band_start=BANDS),
         "band means need flux (and surface_flux on the up sweep)."),
    ])


def good_flux(engine, s):
    arguments = flux_arguments(s)
    ordered(engine)
    assert call(engine, "lbl_path_flux_source", arguments)[0] == 0
    engine.synchronize()
    problem = s.problem
    lengths, weight = problem.lengths(2)
    down = cases.sweep_flux(LD, problem.nu, problem.beta, lengths, weight, problem.temperature, N)
    close("flux", "down sweep", read(arguments["level_flux"], s.columns), down.flux[:LEVELS],
          down.flux_mag[:LEVELS])


# ---------------------------------------------------------------------------------------------
def jacobian_arguments(s):
    return dict(
        s.run(grid=s.grid), path_length=s.lengths, temperature=s.temperature,
        boundary_temperature=s.boundary_t, boundary_emissivity=s.boundary_e, n_bands=0,
        band_start=None, work=s.rows(LEVELS), radiance=s.rows(P),
        optical_depth_jacobian=s.rows(LEVELS), log_optical_depth_jacobian=None,
        temperature_jacobian=None, boundary_temperature_jacobian=None,
        boundary_emissivity_jacobian=None, flags=RADIANCE | JACOBIAN_DEPTH)


def refuse_jacobian(engine, s):
    good = jacobian_arguments(s)
    work = good["work"]
    return refused(engine, "lbl_path_jacobian", good, [
        (dict(work=None), "beta, path_length, temperature and work must not be NULL."),
        (dict(flags=0), "no quantity requested."),
        (dict(flags=RADIANCE | JACOBIAN_TEMPERATURE),
         "an output requested by the flags is NULL."),
        (dict(flags=RADIANCE | CUMULATIVE),
         "LBL_PATH_CONTINUE and LBL_PATH_CUMULATIVE must not be set: a call takes whole paths "
         "and returns every level."),
        (dict(level_count=LEVELS - 1),
         "the run must consist of whole paths: level_begin and level_count must be multiples of "
         "levels_per_path."),
        (dict(grid=-5), "unknown grid handle."),
        (dict(path_length=np.full(LEVELS, -1.)), "path lengths must be finite and >= 0."),
        (dict(temperature=np.zeros(LEVELS)), "temperatures must be finite and > 0."),
        (dict(boundary_temperature=np.array([np.inf, 288.])),
         "boundary temperatures must be finite and >= 0 (0: no boundary)."),
        (dict(boundary_emissivity=np.array([np.nan, 1.])),
         "boundary emissivities must lie in [0, 1]."),
        # (the problem's path 0 has no boundary)
        (dict(flags=RADIANCE | JACOBIAN_BOUNDARY_T, boundary_temperature_jacobian=s.rows(P)),
         "a boundary Jacobian is requested for a path without a boundary (boundary temperature "
         "0)."),
        (dict(n_bands=2, band_start=None), "n_bands < 0, or band_start is NULL."),
        (dict(flags=JACOBIAN_DEPTH | JACOBIAN_LOG_DEPTH, optical_depth_jacobian=work,
              log_optical_depth_jacobian=work), "only one of the outputs may be the work block."),
        (dict(radiance=work), "only dI/dx or dI/dln x may be written over the work block."),
    ])


def good_jacobian(engine, s):
    arguments = jacobian_arguments(s)
    ordered(engine)
    assert call(engine, "lbl_path_jacobian", arguments)[0] == 0
    engine.synchronize()
    problem = s.problem
    values, magnitudes = jac.jacobian(LD, problem.nu, problem.beta, problem.thickness,
                                      problem.temperature, N, False, problem.boundary_t,
                                      problem.boundary_e)
    for q, count in (("radiance", P), ("optical_depth_jacobian", LEVELS)):
        close("jacobian " + q, q, read(arguments[q], s.columns), values[q][:count],
              magnitudes[q][:count])


# ---------------------------------------------------------------------------------------------
def refuse_solar_spectrum(engine, s):
    row = s.rows(1)
    good = dict(grid=s.grid, columns=s.columns, n_knots=0, knot_wavenumber=None,
                knot_irradiance=None, temperature=5772., scale=6.8e-5, row=row, flags=0)
    values = np.linspace(1., 2., s.columns)
    table = dict(n_knots=3, knot_wavenumber=np.array([10., 20., 30.]),
                 knot_irradiance=np.array([1., 2., 3.]))
    return refused(engine, "lbl_solar_spectrum", good, [
        (dict(row=None), "row must not be NULL."),
        (dict(grid=-5), "unknown grid handle."),
        (dict(columns=s.columns + 1), "need 1 <= columns <= the grid's points."),
        (dict(scale=0.), "scale must be finite and > 0."),
        (dict(temperature=-1.), "the temperature must be finite and > 0."),
        (dict(n_knots=3), "knot_irradiance must not be NULL."),
        (dict(n_knots=s.columns - 1, knot_irradiance=values),
         "without knot_wavenumber n_knots must equal columns."),
        (dict(table, n_knots=1), "n_knots must lie in 2..4194304."),
        (dict(table, knot_wavenumber=np.array([10., np.nan, 30.])),
         "knots must be finite and strictly ascending."),
        (dict(table, knot_irradiance=np.array([1., -2., 3.])),
         "irradiances must be finite and >= 0."),
    ]), good


def good_solar_spectrum(engine, s, good):
    ordered(engine)
    assert call(engine, "lbl_solar_spectrum", good)[0] == 0
    engine.synchronize()
    got = read(good["row"], s.columns)[0].astype(LD)
    reference = solar.blackbody(LD, s.problem.nu, 6.8e-5, 5772.)
    assert np.all(np.abs(got - reference) <= LD(1e-12)*np.abs(reference)) and np.any(got > 0.)


# ---------------------------------------------------------------------------------------------
def solar_arguments(s):
    lengths, _ = solar.lengths_of(s.problem)
    sun = block(solar.solar_row(s.problem)[None, :], 1, s.columns, s.layout, np.nan)
    return dict(
        s.run(), solar_length=np.ascontiguousarray(lengths[:LEVELS]), view_length=None,
        solar_zenith_cosine=np.ascontiguousarray(solar.MU0[:P]), solar_row=sun, albedo_rows=None,
        albedo=None, n_bands=0, band_start=None, carry=s.rows(2*P),
        interface_rows=s.rows(LEVELS), space_rows=s.rows(P), surface_rows=None,
        reflected_rows=None, interface_mean=None, space_mean=None, surface_mean=None,
        reflected_mean=None, flags=0)


def refuse_solar(engine, s):
    good = solar_arguments(s)
    view = dict(view_length=s.lengths, albedo=np.array([0.3, 0.5]), reflected_rows=s.rows(P))
    return refused(engine, "lbl_path_solar", good, [
        (dict(solar_row=None),
         "beta, solar_length, solar_zenith_cosine, solar_row and carry must not be NULL."),
        (dict(view_length=s.lengths), "a view needs an albedo: albedo_rows or albedo, not both."),
        (dict(albedo=np.array([0.3, 0.5])), "an albedo is only used with view_length."),
        (dict(reflected_rows=s.rows(P)), "reflected_rows goes with view_length: both or neither."),
        (dict(interface_rows=None, space_rows=None), "no output requested."),
        (dict(interface_rows=s.beta), "interface_rows must not be beta."),
        (dict(n_paths=0), "need n_paths >= 1 and levels_per_path >= 1."),
        (dict(view, view_length=np.full(LEVELS, np.inf)), "view lengths must be finite and >= 0."),
        (dict(solar_zenith_cosine=np.array([1., 0.])), "solar zenith cosines must lie in (0, 1]."),
        (dict(view, albedo=np.array([0.3, 1.5])), "albedos must lie in [0, 1]."),
        (dict(n_bands=2, band_start=np.array([-1, 3, 8], dtype=np.int64)),
         "band_start out of [0, columns]."),
        (dict(n_bands=2, band_start=BANDS, surface_mean=plain(P, 2)),
         "a band mean needs the rows it is the mean of."),
        (dict(space_mean=plain(P, 2)), "band means need n_bands > 0."),
    ])


def good_solar(engine, s):
    arguments = solar_arguments(s)
    ordered(engine)
    assert call(engine, "lbl_path_solar", arguments)[0] == 0
    engine.synchronize()
    lengths, _ = solar.lengths_of(s.problem)
    loop = solar.mirror(F64, s.problem, solar.MU0, solar.solar_row(s.problem), lengths, False)
    last = solar.last_rows(N, False)[:P]
    carry = read(arguments["carry"], s.columns).reshape(P, 2, s.columns)
    assert same_bits(carry[:, 0], loop["tau"][last])
    assert same_bits(read(arguments["space_rows"], s.columns), loop["f0"][:P])


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("columns, layout", [(8, "aligned"), (8, "offset"), (10, "odd")])
def test_refusals_then_one_good_call_per_entry(engine, columns, layout):
    problem = cases.Problem(columns, N, seed=4000 + columns)
    assert cases.layout_is_vector(layout, columns) == (layout == "aligned")
    with Grid(engine, problem.nu) as grid:
        s = Scene(engine, grid, columns, layout)
        refusals = refuse_path_compute(engine, s)
        refusals += refuse_radiance(engine, s, False)
        refusals += refuse_radiance(engine, s, True)
        refusals += refuse_surface_emissivity(engine, s)
        refusals += refuse_flux(engine, s)
        refusals += refuse_jacobian(engine, s)
        spectrum_refusals, spectrum = refuse_solar_spectrum(engine, s)
        refusals += spectrum_refusals + refuse_solar(engine, s)
        assert refusals == 6 + 11 + 12 + 7 + 14 + 14 + 10 + 13
        # Nothing was queued and the engine is as usable as before.
        good_path_compute(engine, s)
        good_radiance(engine, s)
        good_flux(engine, s)
        good_jacobian(engine, s)
        good_solar_spectrum(engine, s, spectrum)
        good_solar(engine, s)

"""lbl_path_thermal_radiance_spectral and lbl_path_solar_radiance_spectral fed directly (Engine's
path_thermal_radiance_spectral and path_solar_radiance_spectral on rows held in torch tensors),
with flux rows made by the numpy mirror so that the view kernels are tested alone, on the case
tables of tests/scatterer_radiance_cases.py: 1, 3, 512, 513 and 1031 columns (a lane holds 2, a
block 512; the last lane partly filled), 1, 2 and 9 levels per path, both storage orders, M = 2, 3
and 1024 knots, grid points below, on, between and above the knots, descending grids, levels
without a scatterer, with one that only absorbs, with one in one level only, tau == 0 inside a
level that scatters, and in the shortwave calls with and without a Rayleigh row, columns inside the
guard k*mu0 = 1 and a conservative cloud.  tests/test_scatterer_radiance_host.py proves on the CPU
that the tables hold these and decide every branch far from its threshold.

Bounds, none taken from the code under test.  The reference is the long-double mirror of
tests/scatterer_radiance_cases.py, continued from the float64 layer inputs and fed the same float64
flux rows.  Every radiance is within (4*E_cpu + 1e-13)*scale of it, scale as
thermal_radiance_cases and solar_radiance_cases define it: E_cpu = 1.09e-11 (recorded as
E_CPU_THERMAL = 1.1e-11) and 8.3e-12 (E_CPU_SOLAR = 8.4e-12) are the worst |float64 mirror -
long-double mirror|/scale that tests/test_scatterer_radiance_host.py measures over the same tables,
capped at 1e-10; the factor 4 and the floor as in tests/test_gpu_thermal_radiance_shapes.py.  A flat
table gives the grey entry's bits, and without any scatterer the longwave entry gives
lbl_path_radiance's.  Nothing is NaN or inf.  Aligned and odd layouts (the vector and the scalar
kernels), and one run against one run per path, give identical bits; beta and the flux rows are
unwritten."""
import numpy as np
import pytest

from tests import scatterer_cases as sc
from tests import scatterer_radiance_cases as rc
from tests import solar_radiance_cases as src
from tests import sweep_cases as cases
from tests import thermal_radiance_cases as trc
from tests.test_gpu_solar_radiance_shapes import run as grey_solar_run
from tests.test_gpu_sweep_shapes import Grid, Rows, block, ordered, plain, read, same_bits
from tests.test_gpu_thermal_radiance_shapes import run as grey_thermal_run

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
PATHS, SENTINEL = cases.PATHS, cases.SENTINEL
THERMAL_BOUND = LD(4.*rc.E_CPU_THERMAL + rc.FLOOR)
SOLAR_BOUND = LD(4.*rc.E_CPU_SOLAR + rc.FLOOR)
THERMAL_CASES, SOLAR_CASES = rc.thermal_cases(), rc.solar_cases()
SOLAR_FLUXES = ("up", "direct", "diffuse")
BAD_ARGUMENT = 2            # LBL_BAD_ARGUMENT


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    return default_engine(0)


def whole(inputs):
    return [(0, inputs.levels)]


def per_path(inputs, reverse=False):
    n = inputs.levels_per_path
    runs = [(p*n, n) for p in range(PATHS)]
    return runs[::-1] if reverse else runs


def thermal(engine, inputs, mu, layout, runs, from_last, fluxes=None, knots=None, optics=None,
            bands=None):
    """Both outputs of lbl_path_thermal_radiance_spectral over `runs` of whole paths (first
    level, count)."""
    n, columns, levels = inputs.levels_per_path, inputs.columns, inputs.levels
    knots = inputs.knots if knots is None else knots
    optics = inputs.optics if optics is None else optics
    fluxes = rc.thermal_flux_rows(inputs, from_last) if fluxes is None else fluxes
    beta = block(inputs.beta, levels, columns, layout, np.nan)
    up = block(fluxes["up"], levels, columns, layout, np.nan)
    down = block(fluxes["down"], levels, columns, layout, np.nan)
    rows = {name: block(None, PATHS, columns, layout, SENTINEL)
            for name in ("radiance", "brightness")}
    mean = None if bands is None else plain(PATHS, bands.size - 1)
    keywords = {}
    if inputs.emissivity.ndim == 2:
        keywords["emissivity_rows"] = Rows(block(inputs.emissivity, PATHS, columns, layout, np.nan))
    else:
        keywords["emissivity"] = inputs.emissivity
    with Grid(engine, inputs.nu) as grid:
        ordered(engine)
        for first, count in runs:
            part = slice(first, first + count)
            outputs = {name + "_rows": Rows(rows[name]) for name in rows}
            if bands is not None:
                outputs["radiance_mean"] = Rows(mean)
            engine.path_thermal_radiance_spectral(
                Rows(beta[part]), columns, grid, PATHS, n, first, inputs.table[part], knots,
                optics[part], mu, inputs.surface_t, Rows(up[part]), Rows(down[part]),
                diffusivity=inputs.diffusivity, band_start=bands, from_last=from_last, **outputs,
                **keywords)
            engine.synchronize()
    out = {name: read(tensor, columns) for name, tensor in rows.items()}
    if mean is not None:
        out["radiance mean"] = read(mean)
    assert np.array_equal(read(beta)[:, :columns], inputs.beta), "beta was written"
    assert same_bits(read(up)[:, :columns], fluxes["up"]), "up_rows were written"
    assert same_bits(read(down)[:, :columns], fluxes["down"]), "down_rows were written"
    return out


def solar(engine, inputs, mu, phi, layout, runs, from_last, fluxes=None, knots=None, optics=None,
          rayleigh=None, bands=None):
    """The output of lbl_path_solar_radiance_spectral over `runs` of whole paths; rayleigh:
    whether the entry gets a Rayleigh row (None: as the problem says)."""
    n, columns, levels = inputs.levels_per_path, inputs.columns, inputs.levels
    knots = inputs.knots if knots is None else knots
    optics = inputs.optics if optics is None else optics
    rayleigh = getattr(inputs, "rayleigh", True) if rayleigh is None else rayleigh
    assert rayleigh or np.all(inputs.sigma == 0.)
    fluxes = rc.solar_flux_rows(inputs, from_last) if fluxes is None else fluxes
    cos_theta = src.scattering_cosine(mu, inputs.mu0, phi)
    beta = block(inputs.beta, levels, columns, layout, np.nan)
    rows = {q: block(fluxes[q], levels, columns, layout, np.nan) for q in SOLAR_FLUXES}
    sun = block(inputs.solar[None, :], 1, columns, layout, np.nan)
    sigma = block(inputs.sigma[None, :], 1, columns, layout, np.nan)
    radiance = block(None, PATHS, columns, layout, SENTINEL)
    mean = None if bands is None else plain(PATHS, bands.size - 1)
    keywords = {"rayleigh_row": Rows(sigma) if rayleigh else None}
    if inputs.albedo.ndim == 2:
        keywords["albedo_rows"] = Rows(block(inputs.albedo, PATHS, columns, layout, np.nan))
    else:
        keywords["albedo"] = inputs.albedo
    with Grid(engine, inputs.nu) as grid:
        ordered(engine)
        for first, count in runs:
            part = slice(first, first + count)
            outputs = {"radiance_rows": Rows(radiance)}
            if bands is not None:
                outputs["radiance_mean"] = Rows(mean)
            engine.path_solar_radiance_spectral(
                Rows(beta[part]), columns, grid, PATHS, n, first, inputs.table[part], knots,
                optics[part], inputs.mu0, mu, cos_theta, Rows(sun), Rows(rows["up"][part]),
                Rows(rows["direct"][part]), Rows(rows["diffuse"][part]), band_start=bands,
                from_last=from_last, **outputs, **keywords)
            engine.synchronize()
    host = radiance.cpu().numpy()
    assert np.all(host[:, columns:] == SENTINEL), "the padding of the output was written"
    out = {"radiance": np.ascontiguousarray(host[:, :columns])}
    if mean is not None:
        out["radiance mean"] = read(mean)
    assert np.array_equal(read(beta)[:, :columns], inputs.beta), "beta was written"
    for q in SOLAR_FLUXES:
        assert same_bits(read(rows[q])[:, :columns], fluxes[q]), q + "_rows were written"
    return out


def close(what, got, expect, scale, bound):
    """Every radiance within bound*scale of the long-double mirror, and finite."""
    value = got["radiance"]
    assert np.all(np.isfinite(value)), what
    error = np.abs(value.astype(LD) - expect)
    allowed = bound*scale
    lit = allowed > 0.
    worst = float(np.max(error[lit]/allowed[lit], initial=0.))
    print("%s: worst error / bound %.3g" % (what, worst))
    assert np.all(error <= allowed), (what, worst)


# ---------------------------------------------------------------------------------------------
# The case tables.
@pytest.mark.parametrize("index", range(len(THERMAL_CASES)))
def test_longwave_case_tables_match_the_mirror(engine, index):
    inputs, mu, from_last = THERMAL_CASES[index]
    what = (inputs.name, from_last)
    fluxes = rc.thermal_flux_rows(inputs, from_last)
    got = thermal(engine, inputs, mu, "aligned", whole(inputs), from_last, fluxes)
    expect = rc.thermal_mirror(LD, inputs, mu, from_last, fluxes)
    close(what, got, expect["radiance"], expect["scale"], THERMAL_BOUND)
    assert np.all(np.isfinite(got["brightness"])), what
    inverted = cases.brightness(LD, inputs.nu[None, :], got["radiance"])
    assert np.all(np.abs(got["brightness"].astype(LD) - inverted) <= LD(1e-13)*inverted), what
    # The scalar kernel on an odd stride, one run per path: the same bits.
    odd = thermal(engine, inputs, mu, "odd", per_path(inputs, from_last), from_last, fluxes)
    for name in got:
        assert same_bits(odd[name], got[name]), (what, name)


@pytest.mark.parametrize("index", range(len(SOLAR_CASES)))
def test_shortwave_case_tables_match_the_mirror(engine, index):
    inputs, mu, phi, from_last = SOLAR_CASES[index]
    what = (inputs.name, from_last)
    fluxes = rc.solar_flux_rows(inputs, from_last)
    got = solar(engine, inputs, mu, phi, "aligned", whole(inputs), from_last, fluxes)
    cos_theta = src.scattering_cosine(mu, inputs.mu0, phi)
    expect = rc.solar_mirror(LD, inputs, mu, cos_theta, from_last, fluxes)
    close(what, got, expect["radiance"], src.scale(inputs, expect), SOLAR_BOUND)
    odd = solar(engine, inputs, mu, phi, "odd", per_path(inputs, from_last), from_last, fluxes)
    assert same_bits(odd["radiance"], got["radiance"]), what
    if not inputs.rayleigh:
        # A Rayleigh row of zeros gives what no row gives: the level's own lines return what the
        # wave-uniform short cut returns.
        zeros = solar(engine, inputs, mu, phi, "aligned", whole(inputs), from_last, fluxes,
                      rayleigh=True)
        assert same_bits(zeros["radiance"], got["radiance"]), what


@pytest.mark.parametrize("name, columns, bands", cases.BAND_SETS[:1])
def test_band_means_are_the_grey_entries(engine, name, columns, bands):
    long = sc.longwave_inputs(columns, 3, 3, 70)
    got = thermal(engine, long, rc.MU, "aligned", whole(long), True, bands=bands)
    means = cases.band_means(LD, got["radiance"], bands)
    empty = np.isnan(means)
    assert np.array_equal(np.isnan(got["radiance mean"]), empty) and np.any(~empty)
    assert np.all(np.abs(got["radiance mean"][~empty].astype(LD) - means[~empty]) <=
                  LD(1e-12)*np.abs(means[~empty]))
    short = sc.shortwave_inputs(columns, 3, 3, 70)
    short.mu0 = np.array(src.MU0)
    got = solar(engine, short, rc.MU, rc.PHI, "aligned", whole(short), True, bands=bands)
    means = cases.band_means(LD, got["radiance"], bands)
    empty = np.isnan(means)
    assert np.array_equal(np.isnan(got["radiance mean"]), empty) and np.any(~empty)
    assert np.all(np.abs(got["radiance mean"][~empty].astype(LD) - means[~empty]) <=
                  LD(1e-12)*np.abs(means[~empty]))


# ---------------------------------------------------------------------------------------------
# Property 1: flat tables.
def level_optics(inputs):
    """[levels, 3]: a grey scatterer out of the table's first knot; every fourth level only
    absorbs, every fifth has none."""
    level = inputs.optics[:, 0, :].copy()
    level[::4, 1] = 0.
    level[::5, 0] = 0.
    return level


@pytest.mark.parametrize("m", [2, sc.MAX_KNOTS])
@pytest.mark.parametrize("from_last", [False, True])
def test_a_flat_table_gives_the_grey_entries_bits(engine, m, from_last):
    knots = np.sort(np.random.default_rng(m).uniform(-50., 3200., size=m))
    inputs = sc.longwave_inputs(513, 9, 3, 11, emissivity_rows=True)
    level = level_optics(inputs)
    grey = inputs.grey(level).isothermal()
    fluxes = trc.flux_rows(grey, from_last)
    expect = grey_thermal_run(engine, grey, rc.MU, "aligned", whole(inputs), from_last,
                              fluxes=fluxes)
    got = thermal(engine, inputs, rc.MU, "aligned", whole(inputs), from_last, fluxes, knots,
                  sc.flat_optics(level, m))
    for name in ("radiance", "brightness"):
        assert same_bits(got[name], expect[name]), (m, from_last, name)
    assert np.any(got["radiance"] > 0.)
    for rayleigh in (True, False):
        inputs = sc.shortwave_inputs(513, 9, 3, 11, albedo_rows=True)
        inputs.mu0 = np.array(src.MU0)
        if not rayleigh:
            rc.without_rayleigh(inputs)
        level = level_optics(inputs)
        grey = inputs.grey(level)
        fluxes = src.flux_rows(grey, from_last)
        expect = grey_solar_run(engine, grey, rc.MU, rc.PHI, "aligned", whole(inputs), from_last,
                                fluxes=fluxes)
        got = solar(engine, inputs, rc.MU, rc.PHI, "aligned", whole(inputs), from_last, fluxes,
                    knots, sc.flat_optics(level, m), rayleigh=rayleigh)
        assert same_bits(got["radiance"], expect["radiance"]), (m, from_last, rayleigh)
        assert np.any(got["radiance"] > 0.)


# ---------------------------------------------------------------------------------------------
# Property 2: without scatterers.
@pytest.mark.parametrize("from_last", [False, True])
def test_without_scatterers_the_longwave_entry_has_the_bits_of_path_radiance(engine, from_last):
    """No scatterer at any knot, eps = 1 and mu = 1: lbl_path_radiance's result from B(T_s)."""
    inputs = sc.longwave_inputs(513, 9, sc.MAX_KNOTS, 2)
    inputs.optics[:] = 0.
    inputs.emissivity = np.ones(PATHS)
    ones = np.ones(PATHS)
    got = thermal(engine, inputs, ones, "aligned", whole(inputs), from_last)
    beta = block(inputs.beta, inputs.levels, 513, "aligned", np.nan)
    carry = block(None, PATHS, 513, "aligned", SENTINEL)
    radiance = block(None, PATHS, 513, "aligned", SENTINEL)
    brightness = block(None, PATHS, 513, "aligned", SENTINEL)
    with Grid(engine, inputs.nu) as grid:
        ordered(engine)
        engine.path_radiance(Rows(beta), 513, grid, PATHS, 9, 0,
                             np.ascontiguousarray(inputs.table[:, 0]),
                             np.ascontiguousarray(inputs.table[:, 4]), Rows(carry),
                             boundary_temperature=inputs.surface_t, boundary_emissivity=ones,
                             radiance=Rows(radiance), brightness_temperature=Rows(brightness),
                             from_last=not from_last)
        engine.synchronize()
    assert same_bits(got["radiance"], read(radiance, 513))
    assert same_bits(got["brightness"], read(brightness, 513))
    assert np.any(got["radiance"] > 0.)


# ---------------------------------------------------------------------------------------------
# Refused calls.
def test_refused_knot_arguments_launch_nothing_and_leave_the_engine_usable(engine):
    long = sc.longwave_inputs(67, 3, 3, 1)
    short = sc.shortwave_inputs(67, 3, 3, 1)
    short.mu0 = np.array(src.MU0)
    columns, levels = 67, long.levels
    cos_theta = src.scattering_cosine(rc.MU, short.mu0, rc.PHI)
    fluxes = {"long": rc.thermal_flux_rows(long, False), "short": rc.solar_flux_rows(short, False)}

    def tensors(inputs, rows):
        made = {"beta": block(inputs.beta, levels, columns, "aligned", np.nan),
                "radiance": block(None, PATHS, columns, "aligned", SENTINEL)}
        for q, values in rows.items():
            made[q] = block(values, levels, columns, "aligned", np.nan)
        return made

    def changed(optics, index, value):
        out = optics.copy()
        out[index] = value
        return out

    def table_with(inputs, column):
        out = inputs.table.copy()
        out[2, column] = 0.5
        return out

    def bad_tables(inputs, word):
        m = inputs.knots.size
        return [dict(n_knots=1), dict(n_knots=sc.MAX_KNOTS + 1), dict(n_knots=0),
                dict(knots=None), dict(optics=None),
                dict(knots=inputs.knots[::-1].copy()),
                dict(knots=changed(inputs.knots, 1, inputs.knots[0])),
                dict(knots=changed(inputs.knots, 1, np.nan)),
                dict(knots=changed(inputs.knots, m - 1, np.inf)),
                dict(optics=changed(inputs.optics, (4, 1, 0), -1e-9)),
                dict(optics=changed(inputs.optics, (4, 1, 0), np.nan)),
                dict(optics=changed(inputs.optics, (4, 1, 0), np.inf)),
                dict(optics=changed(inputs.optics, (4, 1, 1), 1.0000001)),
                dict(optics=changed(inputs.optics, (4, 1, 1), -0.1)),
                dict(optics=changed(inputs.optics, (4, 1, 2), 1.)),
                dict(optics=changed(inputs.optics, (4, 1, 2), np.nan)),
                dict(table=table_with(inputs, word)), dict(table=table_with(inputs, word + 2)),
                dict(grid=12345), dict(short_grid=True)]

    def pointer(array):
        return None if array is None else array.ctypes.data

    def raw_long(made, grid, case):
        knots, optics = case.get("knots", long.knots), case.get("optics", long.optics)
        table = case.get("table", long.table)
        return engine.lib.lbl_path_thermal_radiance_spectral(
            engine.handle, made["beta"].data_ptr(), made["beta"].shape[1], columns,
            case.get("grid", grid), PATHS, 3, 0, levels, table.ctypes.data,
            case.get("n_knots", long.knots.size), pointer(knots), pointer(optics),
            float(long.diffusivity), rc.MU.ctypes.data, long.surface_t.ctypes.data, None,
            long.emissivity.ctypes.data, made["up"].data_ptr(), made["down"].data_ptr(), 0, None,
            made["radiance"].data_ptr(), None, None, 0)

    def raw_short(made, grid, case):
        knots, optics = case.get("knots", short.knots), case.get("optics", short.optics)
        table = case.get("table", short.table)
        return engine.lib.lbl_path_solar_radiance_spectral(
            engine.handle, made["beta"].data_ptr(), made["beta"].shape[1], columns, PATHS, 3, 0,
            levels, table.ctypes.data, case.get("grid", grid),
            case.get("n_knots", short.knots.size), pointer(knots), pointer(optics),
            short.mu0.ctypes.data, rc.MU.ctypes.data, cos_theta.ctypes.data,
            made["solar"].data_ptr(), None, None, short.albedo.ctypes.data, made["up"].data_ptr(),
            made["direct"].data_ptr(), made["diffuse"].data_ptr(), 0, None,
            made["radiance"].data_ptr(), None, 0)

    assert long.emissivity.ndim == 1 and short.albedo.ndim == 1
    for inputs, rows, raw, word, name in (
            (long, fluxes["long"], raw_long, 1, b"lbl_path_thermal_radiance_spectral"),
            (short, fluxes["short"], raw_short, 2, b"lbl_path_solar_radiance_spectral")):
        made = tensors(inputs, rows)
        if inputs is short:
            made["solar"] = block(short.solar[None, :], 1, columns, "aligned", np.nan)
        with Grid(engine, inputs.nu) as grid, Grid(engine, inputs.nu[:60]) as small:
            ordered(engine)
            for case in bad_tables(inputs, word):
                if case.pop("short_grid", False):
                    case["grid"] = small
                assert raw(made, grid, case) == BAD_ARGUMENT, case
                message = engine.lib.lbl_last_error(engine.handle)
                assert name in message and len(message) > len(name) + 10, case
            engine.synchronize()
            assert np.all(read(made["radiance"]) == SENTINEL)
            assert np.array_equal(read(made["beta"])[:, :columns], inputs.beta)
            for q, values in rows.items():
                assert same_bits(read(made[q])[:, :columns], values), q
            # The same call without the fault is taken: the engine is usable.
            assert raw(made, grid, {}) == 0
            engine.synchronize()
        value = read(made["radiance"], columns)
        assert np.all(np.isfinite(value)) and np.all(value != SENTINEL)

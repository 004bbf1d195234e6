"""CPU-only checks of Spectroscopy.compute_solar: the argument checks (all raised before anything
touches the GPU), the C header against the ctypes signatures of the two entries, the constants,
the numpy mirror of tests/solar_cases.py against analytic cases, that the case tables reach every
code path of csrc/solar.h they are meant to, and what one call queues on a stand-in engine."""
import inspect
import math
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy, paths
from pylbl_amd import engine as engine_module
from tests import abi_header, solar_cases as solar
from tests.abi_header import parameters_of
from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests.test_linear_source_host import make_spectroscopy

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd.h").read_text()
KERNELS = (ROOT / "pylbl_amd" / "csrc" / "solar.h").read_text()
F64, LD = np.float64, np.longdouble
ONES = np.ones((3, 5))
GRID_POINTS = 100            # make_spectroscopy's grid


# ---------------------------------------------------------------------------------------------
# The requests.
KNOTS = np.array([590., 600., 610.])
REFLECTED = dict(quantities="reflected_radiance", view_path_length=ONES, surface_albedo=0.3)
BAD = [
    (dict(layer_thickness=np.ones((3, 4))), "shape"),
    (dict(layer_thickness=-ONES), "finite and >= 0"),
    (dict(solar_zenith_cosine=0.), r"\(0, 1\]"),
    (dict(solar_zenith_cosine=1.0001), r"\(0, 1\]"),
    (dict(solar_zenith_cosine=np.nan), r"\(0, 1\]"),
    (dict(solar_zenith_cosine=[1., -0.5, 1.]), r"\(0, 1\]"),
    (dict(solar_zenith_cosine=np.ones(5)), "shape"),
    (dict(solar_path_length=np.ones((3, 4))), "shape"),
    (dict(solar_path_length=ONES*np.inf), "finite and >= 0"),
    (dict(solar_path_length=-ONES), "finite and >= 0"),
    (dict(distance_factor=0.), "distance_factor"),
    (dict(distance_factor=np.inf), "distance_factor"),
    (dict(distance_factor=[1., 1.]), "distance_factor"),
    (dict(solar_wavenumber=KNOTS), "needs solar_irradiance"),
    (dict(solar_irradiance=np.ones(GRID_POINTS - 1)), "one value per grid point"),
    (dict(solar_irradiance=-np.ones(GRID_POINTS)), "finite and >= 0"),
    (dict(solar_irradiance=np.full(GRID_POINTS, np.nan)), "finite and >= 0"),
    (dict(solar_irradiance=[1., 1., 1.], solar_wavenumber=[600., 600., 610.]),
     "strictly ascending"),
    (dict(solar_irradiance=[1., 1.], solar_wavenumber=[600., np.nan]), "strictly ascending"),
    (dict(solar_irradiance=[1.], solar_wavenumber=[600.]), "2..4194304"),
    (dict(solar_irradiance=[1., 1.], solar_wavenumber=KNOTS), "one value per knot"),
    (dict(solar_irradiance=[1., -1., 1.], solar_wavenumber=KNOTS), "finite and >= 0"),
    (dict(surface="top"), "surface must be"),
    (dict(quantities="reflected_radiance"), "needs view_path_length and surface_albedo"),
    (dict(quantities="reflected_radiance", view_path_length=ONES), "needs view_path_length"),
    (dict(quantities="reflected_radiance", surface_albedo=0.3), "needs view_path_length"),
    (dict(view_path_length=ONES), "only used by"),
    (dict(surface_albedo=0.3), "only used by"),
    (dict(albedo_wavenumber=KNOTS), "only used by"),
    (dict(REFLECTED, view_path_length=np.ones((3, 4))), "shape"),
    (dict(REFLECTED, view_path_length=-ONES), "finite and >= 0"),
    (dict(REFLECTED, surface_albedo=1.2), r"\[0, 1\]"),
    (dict(REFLECTED, surface_albedo=[0.1, np.nan, 0.3]), r"\[0, 1\]"),
    (dict(REFLECTED, surface_albedo=np.ones(4)), "shape"),
    (dict(REFLECTED, surface_albedo=[0.1, 0.2], albedo_wavenumber=KNOTS), "shape"),
    (dict(REFLECTED, surface_albedo=[0.1, 0.2, 1.3], albedo_wavenumber=KNOTS), r"\[0, 1\]"),
    (dict(REFLECTED, surface_albedo=np.ones(1025), albedo_wavenumber=np.arange(1025.)),
     "2..1024"),
    (dict(REFLECTED, surface_albedo=[0.1, 0.2, 0.3], albedo_wavenumber=[3., 2., 1.]),
     "albedo_wavenumber must be finite and strictly ascending"),
    (dict(quantities="net_flux"), "quantities must be"),
    (dict(quantities=()), "quantities must be"),
    (dict(range_policy="other"), "range_policy"),
    (dict(band_edges=[600.5, 600.2]), "strictly increasing"),
    (dict(band_edges=[600., 600.5], instrument="boxcar"), "not both"),
    (dict(instrument="boxcar"), "must be an Instrument"),
]


@pytest.mark.parametrize("keywords, match", BAD)
def test_bad_arguments_are_refused_before_the_gpu(monkeypatch, keywords, match):
    def touched(*arguments, **more):
        raise AssertionError("the GPU side was reached")
    monkeypatch.setattr(Spectroscopy, "_sweep_runs", touched)
    monkeypatch.setattr(engine_module, "default_engine", lambda device=0: surface.Untouchable())
    spec = make_spectroscopy((3, 5))
    call = dict(layer_thickness=ONES, solar_zenith_cosine=0.5)
    call.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_solar(**call)


def test_instrument_takes_only_the_quantities_per_path(monkeypatch):
    from pylbl_amd import Instrument
    monkeypatch.setattr(engine_module, "default_engine", lambda device=0: surface.Untouchable())
    spec = make_spectroscopy((3, 5))
    x = Instrument.boxcar([600.3, 600.6], 0.1)
    for quantities in ("direct_irradiance", "heating_rate",
                       ("surface_irradiance", "direct_irradiance")):
        with pytest.raises(ValueError, match="per path"):
            spec.compute_solar(ONES, 0.5, quantities=quantities, instrument=x)
    request = spec._solar_request(ONES, 0.5, None, None, 1., None, "first", None, None, None,
                                  "surface_irradiance", None, x, "reference")
    assert request.instrument is x and request.quantities == ("surface_irradiance",)


def test_heating_rates_need_a_physical_atmosphere(monkeypatch):
    monkeypatch.setattr(engine_module, "default_engine", lambda device=0: surface.Untouchable())
    spec = make_spectroscopy((3, 5))
    spec.atmosphere.pressure = spec.atmosphere.pressure.copy()
    spec.atmosphere.pressure[1, 2] = 0.
    with pytest.raises(ValueError, match="pressures"):
        spec.compute_solar(ONES, 0.5, quantities="heating_rate")
    spec.compute_solar  # the other quantities do not look at the pressure
    assert spec._solar_request(ONES, 0.5, None, None, 1., None, "first", None, None, None,
                               "direct_irradiance", None, None, "reference").scale == \
        paths.SOLAR_SOLID_ANGLE


def test_group_stays_not_implemented():
    spec = make_spectroscopy((3, 5))
    spec.group = object()
    with pytest.raises(NotImplementedError):
        spec.compute_solar(ONES, 0.5)


def test_requests_hold_what_the_sweep_needs():
    spec = make_spectroscopy((3, 5))
    thickness = np.arange(1., 16.).reshape(3, 5)
    mu0 = np.array([1., 0.5, 0.3])
    request = spec._solar_request(thickness, mu0, None, None, 1.03, None, "last", None, None,
                                  None, ("heating_rate", "direct_irradiance"), None, None,
                                  "reference")
    assert request.quantities == ("direct_irradiance", "heating_rate")
    # s/mu0 formed in fp64 on the host, as compute_flux forms s/mu_k.
    assert np.array_equal(request.solar_lengths, (thickness/mu0[:, None]).ravel())
    assert request.scale == paths.SOLAR_SOLID_ANGLE*1.03
    assert request.solar_values is None and request.view_lengths is None
    given = np.linspace(2., 3., 15).reshape(3, 5)
    table = np.array([[0.1, 0.2, 0.3]]*3)
    request = spec._solar_request(
        thickness, 0.25, [1., 2., 0.], KNOTS, 1., given, "first", table, KNOTS, 2.*thickness,
        ("reflected_radiance", "surface_irradiance"), None, None, "skip")
    assert np.array_equal(request.solar_lengths, given.ravel())
    assert np.array_equal(request.view_lengths, 2.*thickness.ravel())
    assert np.array_equal(request.mu0, np.full(3, 0.25))
    assert request.albedo.shape == (3, 3) and np.array_equal(request.albedo_knots, KNOTS)
    assert request.scale == 1. and np.array_equal(request.solar_knots, KNOTS)
    on_grid = spec._solar_request(thickness, 0.25, np.ones(GRID_POINTS), None, 2., None, "first",
                                  None, None, None, "direct_irradiance", None, None, "reference")
    assert on_grid.solar_knots is None and on_grid.solar_values.shape == (GRID_POINTS,)
    bound = inspect.signature(Spectroscopy.compute_solar).parameters
    assert list(bound)[1:] == [
        "layer_thickness", "solar_zenith_cosine", "solar_irradiance", "solar_wavenumber",
        "distance_factor", "solar_path_length", "surface", "surface_albedo", "albedo_wavenumber",
        "view_path_length", "quantities", "band_edges", "instrument", "remove_pedestal",
        "range_policy"]
    assert bound["quantities"].default == ("direct_irradiance",)
    assert bound["distance_factor"].default == 1. and bound["surface"].default == "first"


# ---------------------------------------------------------------------------------------------
# The C ABI and the constants.
def check_argtypes(name, parameters):
    """The shared comparison (tests/abi_header.py); these entries take plain addresses."""
    abi_header.check_argtypes(name, parameters, addresses=True)
    assert name in engine_module.EXPORTED_SYMBOLS


def test_header_declares_both_entries_and_ctypes_match():
    fill = parameters_of("lbl_solar_spectrum")
    assert fill == ["lbl_engine *engine", "int32_t grid", "int64_t columns", "int32_t n_knots",
                    "const double *knot_wavenumber", "const double *knot_irradiance",
                    "double temperature", "double scale", "double *row", "int32_t flags"]
    check_argtypes("lbl_solar_spectrum", fill)
    sweep = parameters_of("lbl_path_solar")
    assert sweep[:8] == parameters_of("lbl_path_compute")[:8]
    assert sweep[8:] == [
        "const double *solar_length", "const double *view_length",
        "const double *solar_zenith_cosine", "const double *solar_row",
        "const double *albedo_rows", "const double *albedo", "int32_t n_bands",
        "const int64_t *band_start", "double *carry", "double *interface_rows",
        "double *space_rows", "double *surface_rows", "double *reflected_rows",
        "double *interface_mean", "double *space_mean", "double *surface_mean",
        "double *reflected_mean", "int32_t flags"]
    check_argtypes("lbl_path_solar", sweep)
    # Appended: every declaration that was there is still there, before the new ones.
    assert HEADER.index("int lbl_wing_batches(") < HEADER.index("int lbl_solar_spectrum(") < \
        HEADER.index("int lbl_path_solar(")
    for method in ("solar_spectrum", "path_solar"):
        assert callable(getattr(engine_module.Engine, method))


def test_constants_agree_and_match_their_formula():
    def defined(name):
        return float(re.search(r"#define %s\s+(\S+)" % name, HEADER).group(1))
    assert defined("LBL_SOLAR_TEMPERATURE") == paths.SOLAR_TEMPERATURE == 5772.
    assert defined("LBL_SOLAR_SOLID_ANGLE") == paths.SOLAR_SOLID_ANGLE
    assert paths.SOLAR_SOLID_ANGLE == math.pi*(6.957e8/1.495978707e11)**2
    assert "SOLAR_SOLID_ANGLE = %r" % paths.SOLAR_SOLID_ANGLE in \
        (ROOT / "pylbl_amd" / "paths.py").read_text()
    assert paths.MAX_SOLAR_KNOTS == solar.MAX_KNOTS == 1 << 22
    assert "kSolarMaxKnots = 1 << 22" in KERNELS
    assert "kSurfaceMaxKnots = %d" % solar.LDS_KNOTS in \
        (ROOT / "pylbl_amd" / "csrc" / "surface.h").read_text()
    assert solar.BLOCK_COLUMNS == 512
    from pylbl_amd import spectroscopy
    assert spectroscopy.SOLAR_TEMPERATURE == 5772. and "heating_rate" in \
        spectroscopy.SOLAR_QUANTITIES


def test_header_docstring_and_kernel_state_the_same_formulas():
    def squeeze(text):
        return re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)", "\n", text))
    docstring = Spectroscopy.compute_solar.__doc__
    for text in (HEADER, KERNELS, docstring):
        assert "F0 = mu0*S" in squeeze(text)
        assert "tau = tau + a_l*beta_l" in squeeze(text)
        assert "tv = tv + v_l*beta_l" in squeeze(text)
        assert "F0*exp(-tau)" in squeeze(text)
        assert "((A*F0)/pi)*exp(-(tau + tv))" in squeeze(text)
        assert "Sun's order" in squeeze(text)
    assert "absorption of the reflected light is not included" in squeeze(docstring)
    # The written interpolation exists once: the fill kernel calls surface.h's functions.
    assert "surface_value(" in KERNELS and "surface_interval(" in KERNELS
    assert "e[j] + (nu - knot[j])" not in KERNELS
    assert "template <bool kVector, bool kView>" in KERNELS
    assert "path_levels<kPathAhead, kVector>" in KERNELS


# ---------------------------------------------------------------------------------------------
# The mirror.
def test_mirror_reproduces_analytic_cases():
    problem = cases.Problem(67, 5, seed=3)
    s = solar.solar_row(problem)
    solar_lengths, view_lengths = solar.lengths_of(problem)
    for kind in (F64, LD):
        for from_last in (False, True):
            # beta = 0: F = F0 at every interface.
            empty = cases.Problem(67, 5, seed=3)
            empty.beta = np.zeros_like(problem.beta)
            got = solar.mirror(kind, empty, solar.MU0, s, solar_lengths, from_last, view_lengths,
                               solar.ALBEDO)
            f0 = solar.incident(kind, solar.MU0, s)
            assert np.array_equal(got["direct"], f0[solar.path_of_level(5)])
            assert np.array_equal(got["reflected"], (solar.ALBEDO.astype(kind)[:, None]*f0) /
                                  kind(cases.FLUX_PI))
            # A = 0 gives no radiance at all.
            got = solar.mirror(kind, problem, solar.MU0, s, solar_lengths, from_last,
                               view_lengths, np.zeros(3))
            assert np.all(got["reflected"] == 0.)
            assert np.all(np.diff(got["tau"].reshape(3, 5, 67), axis=1)
                          * (-1 if from_last else 1) >= 0.)
    # One level: F0*exp(-a*beta).
    one = cases.Problem(67, 1, seed=4)
    a, _ = solar.lengths_of(one)
    got = solar.mirror(F64, one, solar.MU0, s, a, False)
    f0 = solar.MU0[:, None]*s
    assert np.array_equal(got["direct"], f0*np.exp(-(0. + a[:, None]*one.beta)))
    # The references of the GPU tests are formed from the float64 loop's values.
    loop = solar.mirror(F64, problem, solar.MU0, s, solar_lengths, True, view_lengths,
                        solar.ALBEDO)
    direct = solar.direct(LD, loop["f0"], loop["tau"], 5)
    assert np.allclose(direct.astype(F64), loop["direct"], rtol=1e-14, atol=0.)
    reflected = solar.reflected(LD, loop["f0"], solar.ALBEDO, loop["tau"], loop["tv"], 5, True)
    assert np.allclose(reflected.astype(F64), loop["reflected"], rtol=1e-14, atol=0.)
    assert np.array_equal(solar.last_rows(5, True), [0, 5, 10])
    assert np.array_equal(solar.last_rows(5, False), [4, 9, 14])


@pytest.mark.parametrize("m", [2, 17, 1024])
def test_table_mirror_is_the_emissivity_mirror(m):
    rng = np.random.default_rng(m)
    knots = np.sort(rng.uniform(600., 3000., size=m))
    values = solar.table_values(knots)
    nu = surface.knot_samples(knots)
    assert np.array_equal(solar.interval(knots, np.append(nu, np.nan)),
                          surface.interval(knots, np.append(nu, np.nan)))
    for kind in (F64, LD):
        ours = solar.table(kind, knots, values, nu)
        theirs = surface.emissivity(kind, knots, values[None, :], nu)[0]
        assert ours.dtype == kind and np.array_equal(ours, theirs)
    assert np.array_equal(solar.table(F64, knots, values, nu),
                          paths.interpolate_emissivity(knots, values, nu))
    error = np.abs(solar.table(F64, knots, values, nu).astype(LD) -
                   solar.table(LD, knots, values, nu))
    j = np.clip(solar.interval(knots, nu), 0, m - 2)
    assert np.all(error <= LD(6e-16)*np.maximum(values[j], values[j + 1]))
    assert np.all(solar.table(F64, knots, np.full(m, 0.7318), nu) == 0.7318)


# ---------------------------------------------------------------------------------------------
# The case tables reach the code they are meant to.
def test_case_tables_reach_every_path_of_the_kernels():
    # path_levels: every depth class, upward and downward, whole paths and pieces.
    classes = {cases.depth_class(n, cases.PATH_AHEAD) for n in solar.DEPTHS}
    for runs in cases.run_sets(solar.RUN_DEPTH, cases.PATH_AHEAD).values():
        for first, count in runs:
            for from_last in (False, True):
                for lane in cases.path_lanes(first, count, solar.RUN_DEPTH, from_last):
                    classes.add(cases.depth_class(lane.n, cases.PATH_AHEAD))
    assert classes == {"below", "one batch", "batch and remainder", "batches",
                       "batches and remainder"}
    pairs = {(lane.starts, lane.finishes)
             for runs in cases.run_sets(solar.RUN_DEPTH, cases.PATH_AHEAD).values()
             for first, count in runs
             for lane in cases.path_lanes(first, count, solar.RUN_DEPTH, True)}
    assert pairs == {(True, True), (True, False), (False, True), (False, False)}
    # The vector and the scalar form, full and one-column lanes.
    vector = {cases.layout_is_vector(name, columns)
              for name in cases.LAYOUTS for columns in cases.LAYOUT_COLUMNS}
    assert vector == {True, False}
    assert {w for columns in cases.COLUMNS for w in cases.lane_widths(columns)} == {1, 2}
    assert any(columns > solar.BLOCK_COLUMNS for columns in cases.COLUMNS)
    # Both interval routes of the fill kernel, and what each case is there for.
    routes = {name: solar.fill_routes(knots, nu) for name, (knots, nu) in
              solar.fill_cases().items()}
    assert all(len(r) == 3 for name, r in routes.items() if name != "grid points on knots")
    for name in ("2 knots", "1024 knots", "1025 knots", "grid below the knots",
                 "grid above the knots", "grid points on knots"):
        assert set(routes[name]) == {"staged"}, name
    assert set(routes["131072 knots"]) == {"searched"}
    assert routes["slice beyond LDS"] == ["searched", "staged", "staged"]
    assert set(routes["descending grid"]) == set(routes["shuffled grid"]) == {"searched"}
    knots, nu = solar.fill_cases()["grid points on knots"]
    assert np.count_nonzero(np.isin(nu, knots)) >= 300
    value = solar.value_problem()
    assert set(value.mu0) >= {1., 1e-3} and set(value.albedo) >= {0., 1.}
    assert np.any(value.solar == 0.) and np.all((value.solar >= 0.) & (value.solar <= 1.))
    assert np.any(value.beta < 0.) and np.all(value.beta[:, value.group == 0] == 0.)
    assert set(solar.MU0) >= {1., 1e-3} and len(set(solar.MU0)) == cases.PATHS


# ---------------------------------------------------------------------------------------------
# The queue.
def argument(line, name):
    return re.search(r"\b%s=([^,)]+)" % name, line).group(1)


def queue_of(spec, engine, limit_rows, **keywords):
    spec.device_output_limit = (8 << 30) if limit_rows is None else limit_rows*surface.ROW_BYTES
    engine.begin()
    result = spec.compute_solar(**keywords)
    return list(engine.log), result


@pytest.mark.parametrize("surface_end", ["first", "last"])
def test_one_call_computes_beta_once_however_the_levels_are_cut(tmp_path, monkeypatch, surface_end):
    from pylbl_amd import spectroscopy
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    thickness = np.linspace(50., 300., 6).reshape(surface.SHAPE)
    with solar.recorded(tmp_path) as (spec, engine):
        for limit, runs in ((None, 1), (4, 3), (2, 6)):
            log, result = queue_of(
                spec, engine, limit, layer_thickness=thickness, solar_zenith_cosine=[0.5, 0.8],
                surface=surface_end, surface_albedo=[[0.2, 0.4], [0.1, 0.3]],
                albedo_wavenumber=[10., 70.], view_path_length=2.*thickness,
                quantities=paths.SOLAR_QUANTITIES)
            # Two lines gases: two compute calls per run, each level in exactly one run.
            assert sum(line.startswith("compute(") for line in log) == 2*runs
            sweeps = [line for line in log if line.startswith("path_solar(")]
            assert len(sweeps) == runs
            begins = [int(argument(line, "level_begin")) for line in sweeps]
            from_last = surface_end == "first"
            assert begins == sorted(begins, reverse=from_last) and len(set(begins)) == runs
            assert {argument(line, "from_last") for line in sweeps} == {str(from_last)}
            # The S row and the albedo rows are filled once, before the first sweep.
            names = [line.split("(")[0] for line in log
                     if line.startswith(("solar_spectrum", "surface_emissivity", "path_solar"))]
            assert names == ["solar_spectrum", "surface_emissivity"] + ["path_solar"]*runs
            fill = next(line for line in log if line.startswith("solar_spectrum"))
            assert argument(fill, "row") == argument(sweeps[0], "solar_row")
            assert argument(fill, "scale") == repr(paths.SOLAR_SOLID_ANGLE)
            assert argument(fill, "irradiance") == "None"
            rows = next(line for line in log if line.startswith("surface_emissivity"))
            assert {argument(line, "albedo_rows") for line in sweeps} == {argument(rows, "rows")}
            assert {argument(line, "albedo") for line in sweeps} == {"None"}
            assert len({argument(line, "carry") for line in sweeps}) == 1
            assert all(argument(line, "interface_rows") != argument(line, "beta")
                       for line in sweeps)
            assert result["direct_irradiance"].shape == (2, 4, 160)
            assert result["surface_irradiance"].shape == (2, 160)
            assert result["reflected_radiance"].shape == (2, 160)
            assert result["heating_rate"].shape == (2, 3, 160)
        # Bands: the sweeps write blocks of the call, the outputs receive their means.
        log, result = queue_of(spec, engine, None, layer_thickness=thickness,
                               solar_zenith_cosine=0.5, surface=surface_end,
                               band_edges=[20., 30., 60.],
                               quantities=("direct_irradiance", "surface_irradiance"))
        sweep, = [line for line in log if line.startswith("path_solar(")]
        assert argument(sweep, "band_start") != "None" and "view_lengths=None" in sweep
        assert argument(sweep, "interface_mean") != argument(sweep, "interface_rows")
        assert "reflected_rows" not in sweep and "albedo_rows=None" in sweep
        assert result["direct_irradiance"].shape == (2, 4, 2)
        assert np.array_equal(result["band_points"], [40, 120])


def test_existing_calls_do_not_reach_the_new_entries(tmp_path):
    """compute_radiance and compute_flux queue nothing of the solar entries."""
    with solar.recorded(tmp_path) as (spec, engine):
        engine.begin()
        spec.compute_radiance(np.ones(surface.SHAPE), boundary_temperature=288.)
        assert not any(line.startswith(("solar_spectrum", "path_solar")) for line in engine.log)

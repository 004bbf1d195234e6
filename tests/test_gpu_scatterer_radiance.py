"""Spectroscopy.compute_thermal_radiance_spectral and compute_solar_radiance_spectral on the GPU,
on the synthetic database of the other product tests (2400 grid points, 3 paths of 4 levels): a
spectral cloud against the long-double mirror of its definition
(tests/scatterer_radiance_cases.py) fed compute_absorption("total") and the fluxes of
compute_thermal_flux_spectral and compute_solar_flux_spectral of the same Spectroscopy; flat
tables against the grey calls on the grid, in bands and through an instrument; a table that holds
nothing against compute_radiance and one that only absorbs against compute_solar's reflected
radiance; a table that is not flat against the grey call at its mean; band means and channels of
the fine result; and a call cut into runs of one path against all paths in one run.

Bounds, none taken from the code under test.  Every radiance is within (4*E_cpu + 1e-13)*scale of
the long-double mirror, with E_cpu = scatterer_radiance_cases.E_CPU_THERMAL and E_CPU_SOLAR and
scale as tests/test_gpu_scatterer_radiance_shapes.py has them and for its reasons.  A table that is
flat in wavenumber gives every quantity of the grey call bit for bit, and so does a cut into runs.
Channel radiances are held to tests/test_gpu_instrument.py's bound and band means to
1e-12*magnitude of the long-double means of the fine result."""
import numpy as np
import pytest

from pylbl_amd import paths, two_stream
from pylbl_amd.instrument import Instrument
from tests import scatterer_cases as sc
from tests import scatterer_radiance_cases as rc
from tests import solar_radiance_cases as src
from tests import sweep_cases as cases
from tests.test_gpu_flux import thickness_for, total_of
from tests.test_gpu_instrument import check as check_channels
from tests.test_gpu_solar_radiance import spectroscopy
from tests.test_gpu_thermal_flux_linear import interfaces_of

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
SHAPE = (3, 4)
LEVELS = SHAPE[1]
MU0 = np.array([1., 0.35, 0.08])
MU = np.array([1., 0.6, 0.05])
PHI = np.array([0., 90., 180.])
ALBEDO = np.array([1., 0.3, 0.])
SURFACE_T = np.array([300., 288., 270.])
EMISSIVITY = np.array([1., 0.3, 0.])
THERMAL_BOUND = LD(4.*rc.E_CPU_THERMAL + rc.FLOOR)
SOLAR_BOUND = LD(4.*rc.E_CPU_SOLAR + rc.FLOOR)
METHODS = ("compute_thermal_radiance", "compute_solar_radiance")
TAU, OMEGA, G = ("scatterer_optical_depth", "scatterer_single_scattering_albedo",
                 "scatterer_asymmetry")
# Knots on a grid point, between grid points and beyond both ends of the grid (600 .. 624 cm-1).
KNOTS = np.array([580., 603.345, 610., 615.005, 622., 650.])
EDGES = np.concatenate([[550., 600.5, 600.5005], np.arange(601.3, 624.1, 1.), [640.]])


def grey_cloud():
    """A grey scatterer in levels 1, 2 and 3 of every path: conservative in path 1, one that only
    absorbs in level 3; level 0 holds none."""
    tau_c = np.zeros(SHAPE)
    tau_c[:, 1], tau_c[:, 2], tau_c[:, 3] = [0.5, 8., 40.], [2., 0.05, 3.], [0.3, 0.3, 0.3]
    omega_c = np.full(SHAPE, 0.9)
    omega_c[1] = 1.
    omega_c[:, 3] = 0.
    g_c = np.full(SHAPE, 0.85)
    g_c[2] = 0.3
    return {TAU: tau_c, OMEGA: omega_c, G: g_c}


def flat(cloud, m):
    return {name: np.ascontiguousarray(np.repeat(value[..., None], m, axis=-1))
            for name, value in cloud.items()}


def spectral_cloud():
    """The grey cloud's levels with optics that vary over KNOTS: omega_c falling from 1 to 0.5,
    tau_c falling to exactly 0 at a knot, a level that scatters at two knots only; level 3 only
    absorbs and level 0 holds nothing."""
    rng = np.random.default_rng(4)
    m = KNOTS.size
    cloud = flat(grey_cloud(), m)
    cloud[TAU] = cloud[TAU]*rng.uniform(0.3, 1.5, size=SHAPE + (m,))
    cloud[TAU][:, 2, 2] = 0.
    cloud[OMEGA][:, 1] = np.linspace(1., 0.5, m)
    cloud[OMEGA][:, 2] = [0., 0., 1., 0.7, 0., 0.]
    cloud[G] = cloud[G]*rng.uniform(0.5, 1., size=SHAPE + (m,))
    return cloud


@pytest.fixture(scope="module")
def fine():
    """(spec, beta [3, 4, N], thickness, sigma on the grid, S on the grid)."""
    spec = spectroscopy()
    beta = total_of(spec)
    assert np.all(beta >= 0.) and spec.grid.size == 2400
    thickness = thickness_for(beta)
    column = spec.atmosphere.pressure/(paths.K_B*spec.atmosphere.temperature)*thickness
    sigma = np.random.default_rng(9).uniform(0., 0.3, size=spec.grid.size)/column.max()
    sigma[::11] = 0.
    solar = np.asarray(spec.compute_solar_flux(
        thickness, 1., rayleigh=False, quantities="direct_irradiance",
        remove_pedestal=False)["direct_irradiance"])[0, -1]
    return spec, beta, thickness, sigma, solar


def call(spec, method, fine, **keywords):
    _, _, thickness, sigma, _ = fine
    if method == "compute_solar_radiance":
        arguments = dict(layer_thickness=thickness, solar_zenith_cosine=MU0,
                         view_zenith_cosine=MU, relative_azimuth=PHI, surface_albedo=ALBEDO,
                         rayleigh_cross_section=sigma)
    else:
        arguments = dict(layer_thickness=thickness, surface_temperature=SURFACE_T,
                         view_zenith_cosine=MU, surface_emissivity=EMISSIVITY)
    arguments.update(remove_pedestal=False, **keywords)
    name = rc.SPECTRAL_METHOD[method] if "scatterer_wavenumber" in keywords else method
    return getattr(spec, name)(**arguments)


def rows_below(fluxes, names, first):
    """The flux rows at the interface below each level: interface l with the surface behind level
    0, interface l + 1 with it behind the last level."""
    below = slice(0, LEVELS) if first else slice(1, LEVELS + 1)
    return {name: np.ascontiguousarray(np.asarray(fluxes[q])[:, below].reshape(3*LEVELS, -1))
            for q, name in names}


def close(what, got, expect, scale, bound):
    value = np.asarray(got["radiance"])
    assert value.shape == expect.shape and np.all(np.isfinite(value)), what
    error = np.abs(value.astype(LD) - expect)
    allowed = bound*scale
    print("%s: worst error / bound %.3g" % (what, float(np.max(error/allowed))))
    assert np.all(allowed > 0.) and np.all(error <= allowed), what


# ---------------------------------------------------------------------------------------------
# Against the mirror.
@pytest.mark.parametrize("surface", ["first", "last"])
def test_a_spectral_cloud_in_the_longwave_matches_the_mirror(fine, surface):
    spec, beta, thickness, _, _ = fine
    cloud = spectral_cloud()
    out = call(spec, "compute_thermal_radiance", fine, surface=surface,
               scatterer_wavenumber=KNOTS, quantities=("radiance", "brightness_temperature"),
               **cloud)
    assert set(out) == {"radiance", "brightness_temperature", "wavenumber", "scatterer"}
    assert out["scatterer"] == "spectral"
    fluxes = spec.compute_thermal_flux_spectral(
        thickness, SURFACE_T, KNOTS, cloud[TAU], cloud[OMEGA], cloud[G],
        surface_emissivity=EMISSIVITY, surface=surface, remove_pedestal=False)
    request = two_stream._thermal_radiance_request(
        spec, thickness, SURFACE_T, MU, EMISSIVITY, None, surface, 1.66, cloud[TAU], cloud[OMEGA],
        cloud[G], ("radiance",), None, None, "reference", scatterer_wavenumber=KNOTS)
    interfaces = interfaces_of(spec)            # (not read: the source is the level temperatures')
    inputs = sc.Longwave("call", spec.grid, beta.reshape(3*LEVELS, -1), request.level_table,
                         interfaces, request.surface_temperature, request.surface_emissivity,
                         request.scatterer_knots, request.scatterer_optics, request.diffusivity)
    first = surface == "first"
    rows = rows_below(fluxes, (("upward_flux", "up"), ("downward_flux", "down")), first)
    expect = rc.thermal_mirror(LD, inputs, MU, first, rows)
    close(surface, out, expect["radiance"], expect["scale"], THERMAL_BOUND)
    inverted = cases.brightness(LD, spec.grid[None, :], np.asarray(out["radiance"]))
    got = np.asarray(out["brightness_temperature"])
    assert np.all(got > 0.) and np.all(np.abs(got.astype(LD) - inverted) <= LD(1e-13)*inverted)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_a_spectral_cloud_in_sunlight_matches_the_mirror(fine, surface):
    spec, beta, thickness, sigma, solar = fine
    cloud = spectral_cloud()
    out = call(spec, "compute_solar_radiance", fine, surface=surface, scatterer_wavenumber=KNOTS,
               **cloud)
    assert set(out) == {"radiance", "wavenumber", "scatterer"} and out["scatterer"] == "spectral"
    names = (("upward_flux", "up"), ("direct_irradiance", "direct"),
             ("diffuse_downward_flux", "diffuse"))
    fluxes = spec.compute_solar_flux_spectral(
        thickness, MU0, KNOTS, cloud[TAU], cloud[OMEGA], cloud[G], surface=surface,
        surface_albedo=ALBEDO, rayleigh_cross_section=sigma, quantities=[q for q, _ in names],
        remove_pedestal=False)
    request = spec._solar_flux_request(
        thickness, MU0, None, None, 1., surface, ALBEDO, None, True, sigma, cloud[TAU],
        cloud[OMEGA], cloud[G], ("upward_flux",), None, "reference", scatterer_wavenumber=KNOTS)
    inputs = sc.Shortwave("call", spec.grid, beta.reshape(3*LEVELS, -1), request.level_table, MU0,
                          solar, sigma, ALBEDO, request.scatterer_knots, request.scatterer_optics)
    first = surface == "first"
    space = LEVELS if first else 0
    assert np.array_equal(np.asarray(fluxes["direct_irradiance"])[:, space], inputs.f0())
    rows = rows_below(fluxes, names, first)
    expect = rc.solar_mirror(LD, inputs, MU, src.scattering_cosine(MU, MU0, PHI), first, rows)
    close(surface, out, expect["radiance"], src.scale(inputs, expect), SOLAR_BOUND)
    # Over a black surface what is seen was scattered: path 2.
    assert np.all(np.asarray(out["radiance"])[2] > 0.)


# ---------------------------------------------------------------------------------------------
# Flat tables.
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("surface", ["first", "last"])
def test_flat_tables_give_the_grey_call_bit_for_bit(fine, method, surface):
    spec = fine[0]
    cloud = grey_cloud()
    centers = np.arange(601., 623., 2.5)
    both = ("radiance", "brightness_temperature")
    for how in (dict(), dict(band_edges=EDGES),
                dict(instrument=Instrument.gaussian(centers, 0.5, half_width=0.55))):
        if method == "compute_thermal_radiance" and "band_edges" not in how:
            how["quantities"] = both
        grey = call(spec, method, fine, surface=surface, **how, **cloud)
        for m in (2, 5):
            knots = np.linspace(590., 630., m) if m == 5 else np.array([612.005, 612.015])
            got = call(spec, method, fine, surface=surface, scatterer_wavenumber=knots, **how,
                       **flat(cloud, m))
            for q in how.get("quantities", ("radiance",)):
                assert np.array_equal(np.asarray(got[q]), np.asarray(grey[q]), equal_nan=True), \
                    (sorted(how), m, q)
        assert np.any(np.asarray(grey["radiance"]) > 0.)


# ---------------------------------------------------------------------------------------------
# Without scatterers.
@pytest.mark.parametrize("surface", ["first", "last"])
def test_without_scatterers_the_longwave_call_is_compute_radiance_bit_for_bit(fine, surface):
    """A table that holds nothing at any knot, eps = 1 and mu = 1."""
    spec, _, thickness, _, _ = fine
    both = ("radiance", "brightness_temperature")
    nothing = {name: np.zeros(SHAPE + (KNOTS.size,)) for name in (TAU, OMEGA, G)}
    out = spec.compute_thermal_radiance_spectral(
        thickness, SURFACE_T, KNOTS, nothing[TAU], nothing[OMEGA], nothing[G], surface=surface,
        quantities=both, remove_pedestal=False)
    direction = "toward_last" if surface == "first" else "toward_first"
    plain = spec.compute_radiance(thickness, boundary_temperature=SURFACE_T, direction=direction,
                                  quantities=both, remove_pedestal=False)
    for q in both:
        assert np.array_equal(np.asarray(out[q]), np.asarray(plain[q])), q
    assert np.all(np.asarray(out["radiance"]) > 0.)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_a_table_that_only_absorbs_attenuates_compute_solars_reflected_radiance(fine, surface):
    """No Rayleigh row and omega_c = 0 at every knot: compute_solar's "reflected_radiance" under
    view_path_length = thickness/mu, times exp(-tau_c(nu)/mu0)*exp(-tau_c(nu)/mu) of every level,
    each call within 4*8 roundings per level of A*F0/pi (tests/test_gpu_solar_radiance.py's
    bound for the grey call, and for its reasons) and the factor's own few."""
    spec, _, thickness, _, _ = fine
    m = KNOTS.size
    tau_c = np.zeros(SHAPE + (m,))
    tau_c[:, 1] = np.linspace(0.2, 1.5, m)
    zeros = np.zeros(SHAPE + (m,))
    out = np.asarray(spec.compute_solar_radiance_spectral(
        thickness, MU0, KNOTS, tau_c, zeros, zeros, view_zenith_cosine=MU, relative_azimuth=PHI,
        surface=surface, surface_albedo=ALBEDO, rayleigh=False,
        remove_pedestal=False)["radiance"])
    plain = spec.compute_solar(
        thickness, MU0, surface=surface, surface_albedo=ALBEDO,
        view_path_length=thickness/MU[:, None],
        quantities=("direct_irradiance", "reflected_radiance"), remove_pedestal=False)
    space = LEVELS if surface == "first" else 0
    f0 = np.asarray(plain["direct_irradiance"])[:, space]
    on_grid = sc.interpolate(KNOTS, np.stack([tau_c[0, 1], zeros[0, 1], zeros[0, 1]], axis=1),
                             spec.grid)[:, 0].astype(LD)
    factor = np.exp(-(on_grid[None, :]/MU0[:, None].astype(LD))) * \
        np.exp(-(on_grid[None, :]/MU[:, None].astype(LD)))
    expect = np.asarray(plain["reflected_radiance"]).astype(LD)*factor
    size = ALBEDO[:, None].astype(LD)*f0.astype(LD)/LD(cases.FLUX_PI)
    allowed = LD(2.*4.*src.NO_SCATTERING_ROUNDINGS*LEVELS + 8.)*LD(2.**-53)*size
    assert np.all(np.isfinite(out)) and np.all(np.abs(out.astype(LD) - expect) <= allowed)
    assert np.all(out[:2] > 0.) and np.all(out[2] == 0.)


# ---------------------------------------------------------------------------------------------
# A table that is not flat.
@pytest.mark.parametrize("method", METHODS)
def test_a_cloud_that_is_not_grey_differs_from_the_grey_call_at_its_mean(fine, method):
    """omega_c falls from 1 to 0.5 across the grid and tau_c grows as nu^1.3: against the grey
    call with the table's mean the spectrum differs by per cent of its scale, where the tolerance
    of the other tests is 1e-10."""
    spec = fine[0]
    m = 16
    knots = np.linspace(600., 624., m)
    tau_c = np.zeros(SHAPE + (m,))
    tau_c[:, 1] = 2.*(knots/612.)**1.3
    omega_c = np.broadcast_to(np.linspace(1., 0.5, m), SHAPE + (m,)).copy()
    g_c = np.full(SHAPE + (m,), 0.8)
    cloud = {TAU: tau_c, OMEGA: omega_c, G: g_c}
    mean = {name: value.mean(axis=-1) for name, value in cloud.items()}
    got = np.asarray(call(spec, method, fine, scatterer_wavenumber=knots, **cloud)["radiance"])
    grey = np.asarray(call(spec, method, fine, **mean)["radiance"])
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(grey))
    difference = np.max(np.abs(got - grey), axis=1)/np.max(np.abs(grey), axis=1)
    print("%s: spectral against grey at the mean, of the largest radiance: %s" % (
        method, difference))
    # A million times the tolerance of the other tests.
    assert np.all(difference > 1e-4)


# ---------------------------------------------------------------------------------------------
# Bands, channels and runs.
@pytest.mark.parametrize("method", METHODS)
def test_bands_channels_and_runs_of_one_path(fine, method):
    spec = fine[0]
    cloud = spectral_cloud()
    whole = np.asarray(call(spec, method, fine, scatterer_wavenumber=KNOTS, **cloud)["radiance"])
    got = call(spec, method, fine, scatterer_wavenumber=KNOTS, band_edges=EDGES, **cloud)
    starts = np.searchsorted(spec.grid, EDGES, side="left")
    expect = cases.band_means(LD, whole, starts)
    mean = np.asarray(got["radiance"])
    empty = np.isnan(expect)
    assert np.array_equal(np.isnan(mean), empty) and np.any(empty) and np.any(~empty)
    assert np.all(np.abs(mean[~empty].astype(LD) - expect[~empty]) <=
                  LD(1e-12)*np.abs(expect[~empty]))
    centers = np.arange(601., 623., 2.5)
    instrument = Instrument.gaussian(centers, 0.5, half_width=0.55)
    channels = call(spec, method, fine, scatterer_wavenumber=KNOTS, instrument=instrument, **cloud)
    assert np.asarray(channels["radiance"]).shape == (3, len(centers))
    check_channels(channels["radiance"], instrument, spec.grid, whole)
    # A limit that holds one path and not two (beta, the work rows and the flux rows per level:
    # 5 blocks in the longwave, 6 in the shortwave, and the knot table's few bytes): the knot rows
    # of each run are its own, and the bits are the one-run call's.
    other = spectroscopy()
    blocks = 5 if method == "compute_thermal_radiance" else 6
    other.device_output_limit = int(1.5*blocks*LEVELS*spec.grid.size*8)
    for how, expect in ((dict(), whole), (dict(band_edges=EDGES), mean),
                        (dict(surface="last"), None)):
        cut = np.asarray(call(other, method, fine, scatterer_wavenumber=KNOTS, **how,
                              **cloud)["radiance"])
        if expect is None:
            expect = np.asarray(call(spec, method, fine, scatterer_wavenumber=KNOTS, **how,
                                     **cloud)["radiance"])
        assert np.array_equal(cut, expect, equal_nan=True), sorted(how)

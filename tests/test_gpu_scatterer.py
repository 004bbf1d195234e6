"""Spectroscopy.compute_solar_flux_spectral and compute_thermal_flux_spectral (both sources) on
the GPU, on the synthetic database of the other product tests
(atmosphere shape (3, 7)): a spectral cloud against the long-double mirror of its definition
(tests/scatterer_cases.py) over compute_absorption("total") of the same Spectroscopy, flat tables
against the grey calls, runs of one path against all paths in one run, a conservative spectral
cloud over a white surface, and equal temperatures under the linear source.

Bounds, none taken from the code under test.  Every flux is within (4*E_cpu + 1e-13)*scale of the
long-double mirror: scale = F0 = mu0*S and E_cpu = scatterer_cases.E_CPU_SHORTWAVE for the
shortwave call, scale = pi*max B(nu, T) over the path's temperatures and E_cpu =
scatterer_cases.E_CPU_LONGWAVE for the longwave ones, as tests/test_gpu_scatterer_shapes.py has
them and for its reasons.  A table that is flat in wavenumber gives every quantity of the grey call
bit for bit, and so does a cut into runs of one path; with one temperature throughout a path the
linear source gives the level-temperature source's bits."""
import numpy as np
import pytest

from pylbl_amd import paths, synthetic, two_stream
from tests import scatterer_cases as sc
from tests import thermal_cases as tc
from tests import two_stream_cases as ts
from tests.test_gpu_flux import spectroscopy, thickness_for, total_of
from tests.test_gpu_thermal_flux_linear import interfaces_of

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
SHAPE = (3, 7)
MU0 = np.array([1., 0.35, 0.08])
ALBEDO = np.array([1., 0.3, 0.])
SURFACE_T = np.array([300., 288., 270.])
EMISSIVITY = np.array([1., 0.3, 0.])
SHORTWAVE_BOUND = LD(4.*sc.E_CPU_SHORTWAVE + sc.FLUX_FLOOR)
LONGWAVE_BOUND = LD(4.*sc.E_CPU_LONGWAVE + sc.FLUX_FLOOR)
SOLAR = paths.SOLAR_FLUX_QUANTITIES
THERMAL = paths.THERMAL_FLUX_QUANTITIES
METHODS = ("compute_solar_flux", "compute_thermal_flux", "compute_thermal_flux_linear")
TAU, OMEGA, G = ("scatterer_optical_depth", "scatterer_single_scattering_albedo",
                 "scatterer_asymmetry")
# Knots on a grid point, between grid points and beyond both ends of the grid (600 .. 700 cm-1).
KNOTS = np.array([580., 612.345, 640., 655.005, 690., 730.])
EDGES = np.concatenate([[550., 600.5, 600.5005], np.arange(601.3, 700.1, 1.), [720.]])


def grey_cloud():
    """A grey scatterer in levels 2, 3 and 5 of every path: conservative in path 1, one that only
    absorbs in level 5."""
    tau_c = np.zeros(SHAPE)
    tau_c[:, 2], tau_c[:, 3], tau_c[:, 5] = [0.5, 8., 40.], [2., 0.05, 3.], [0.3, 0.3, 0.3]
    omega_c = np.full(SHAPE, 0.9)
    omega_c[1] = 1.
    omega_c[:, 5] = 0.
    g_c = np.full(SHAPE, 0.85)
    g_c[2] = 0.3
    return {TAU: tau_c, OMEGA: omega_c, G: g_c}


def flat(cloud, m):
    return {name: np.ascontiguousarray(np.repeat(value[..., None], m, axis=-1))
            for name, value in cloud.items()}


def spectral_cloud():
    """The grey cloud's levels with optics that vary over KNOTS: liquid-like omega_c falling from
    1 to 0.5, tau_c falling to exactly 0 at a knot, a level that scatters at two knots only; level
    5 only absorbs, the others hold nothing."""
    rng = np.random.default_rng(4)
    m = KNOTS.size
    cloud = flat(grey_cloud(), m)
    cloud[TAU] = cloud[TAU]*rng.uniform(0.3, 1.5, size=SHAPE + (m,))
    cloud[TAU][:, 3, 2] = 0.
    cloud[OMEGA][:, 2] = np.linspace(1., 0.5, m)
    cloud[OMEGA][:, 3] = [0., 0., 1., 0.7, 0., 0.]
    cloud[G] = cloud[G]*rng.uniform(0.5, 1., size=SHAPE + (m,))
    return cloud


@pytest.fixture(scope="module")
def fine():
    """(spec, beta [3, 7, N], thickness, sigma on the grid, interface temperatures)."""
    spec = spectroscopy(SHAPE)
    beta = total_of(spec)
    assert np.all(beta >= 0.)
    thickness = thickness_for(beta)
    column = spec.atmosphere.pressure/(paths.K_B*spec.atmosphere.temperature)*thickness
    sigma = np.random.default_rng(9).uniform(0., 0.3, size=spec.grid.size)/column.max()
    sigma[::11] = 0.
    return spec, beta, thickness, sigma, interfaces_of(spec)


def call(spec, method, fine, **keywords):
    _, _, thickness, sigma, interfaces = fine
    if method == "compute_solar_flux":
        arguments = dict(layer_thickness=thickness, solar_zenith_cosine=MU0,
                         surface_albedo=ALBEDO, rayleigh_cross_section=sigma)
    else:
        arguments = dict(layer_thickness=thickness, surface_temperature=SURFACE_T,
                         surface_emissivity=EMISSIVITY)
    if method == "compute_thermal_flux_linear":
        arguments["interface_temperature"] = interfaces
    arguments.update(remove_pedestal=False, **keywords)
    name = sc.SPECTRAL_METHOD[method] if "scatterer_wavenumber" in keywords else method
    return getattr(spec, name)(**arguments)


def quantities_of(method):
    return SOLAR if method == "compute_solar_flux" else THERMAL


def on_interfaces(got, names, levels, first):
    """{quantity: [3, 8, N]} on the result's interface dim from a mirror's flat rows."""
    out = {}
    for q, name in names.items():
        below = got[name].reshape(3, levels, -1)
        top = got["top_" + name][:, None, :]
        out[q] = np.concatenate([below, top] if first else [top, below], axis=1)
    return out


def close(what, out, reference, scale, bound):
    for q, expect in reference.items():
        got = np.asarray(out[q])
        assert got.shape == expect.shape and np.all(np.isfinite(got)), (what, q)
        error = np.abs(got.astype(LD) - expect)
        allowed = bound*scale
        lit = np.broadcast_to(allowed > 0., error.shape)
        print("%s, %s: worst error / bound %.3g" % (
            what, q, float(np.max((error/np.where(allowed > 0., allowed, 1.))[lit]))))
        assert np.all(error <= allowed), (what, q)


# ---------------------------------------------------------------------------------------------
# Against the mirror.
@pytest.mark.parametrize("surface", ["first", "last"])
def test_a_spectral_cloud_in_sunlight_matches_the_mirror(fine, surface):
    spec, beta, thickness, sigma, _ = fine
    cloud = spectral_cloud()
    out = call(spec, "compute_solar_flux", fine, surface=surface, scatterer_wavenumber=KNOTS,
               quantities=paths.SOLAR_FLUX_INTERFACE_QUANTITIES, **cloud)
    mark = out.attrs["scatterer"] if hasattr(out, "attrs") else out["scatterer"]
    assert mark == "spectral"
    request = spec._solar_flux_request(
        thickness, MU0, None, None, 1., surface, ALBEDO, None, True, sigma, cloud[TAU],
        cloud[OMEGA], cloud[G], paths.SOLAR_FLUX_INTERFACE_QUANTITIES, None, "reference",
        scatterer_wavenumber=KNOTS)
    space = 7 if surface == "first" else 0
    f0 = np.asarray(out["direct_irradiance"])[:, space]
    assert np.all(f0 > 0.)
    inputs = sc.Shortwave("call", spec.grid, beta.reshape(21, -1), request.level_table, MU0,
                          f0[0]/MU0[0], sigma, ALBEDO, request.scatterer_knots,
                          request.scatterer_optics)
    first = surface == "first"
    layers = ts.layer(LD, inputs.layer_inputs(first))
    got = ts.adding(LD, layers, ALBEDO[:, None], f0)
    names = dict(zip(paths.SOLAR_FLUX_INTERFACE_QUANTITIES, ts.QUANTITIES))
    reference = {}
    for q, name in names.items():
        rows = np.moveaxis(got[name], 0, 1)                     # [3, 8, N], interface 0 first
        reference[q] = rows[:, ::-1] if first else rows
    close(surface, out, reference, f0[:, None, :].astype(LD), SHORTWAVE_BOUND)
    # The cloud is not grey: the grey call with the first knot's optics differs.
    grey = call(spec, "compute_solar_flux", fine, surface=surface,
                quantities=("upward_flux",), **{name: v[..., 0] for name, v in cloud.items()})
    assert np.max(np.abs(np.asarray(grey["upward_flux"]) - np.asarray(out["upward_flux"])) /
                  f0[:, None, :]) > 1e-3


@pytest.mark.parametrize("method", METHODS[1:])
@pytest.mark.parametrize("surface", ["first", "last"])
def test_a_spectral_cloud_in_the_longwave_matches_the_mirror(fine, surface, method):
    spec, beta, thickness, _, interfaces = fine
    cloud = spectral_cloud()
    linear = method == "compute_thermal_flux_linear"
    out = call(spec, method, fine, surface=surface, scatterer_wavenumber=KNOTS,
               quantities=("upward_flux", "downward_flux"), **cloud)
    arguments = (EMISSIVITY, None, surface, 1.66, cloud[TAU], cloud[OMEGA], cloud[G],
                 ("upward_flux", "downward_flux"), None, "reference")
    request = two_stream._thermal_flux_linear_request(
        spec, thickness, SURFACE_T, interfaces, *arguments, scatterer_wavenumber=KNOTS)
    inputs = sc.Longwave("call", spec.grid, beta.reshape(21, -1), request.level_table, interfaces,
                         request.surface_temperature, request.surface_emissivity,
                         request.scatterer_knots, request.scatterer_optics, request.diffusivity)
    assert np.array_equal(inputs.edges, request.edge_temperature)
    first = surface == "first"
    got = sc.longwave_mirror(LD, inputs, first, linear)
    names = dict(zip(("upward_flux", "downward_flux"), tc.QUANTITIES))
    close((method, surface), out, on_interfaces(got, names, 7, first), got["scale"][:, None, :],
          LONGWAVE_BOUND)
    space = 7 if surface == "first" else 0
    assert np.all(np.asarray(out["downward_flux"])[:, space] == 0.)


# ---------------------------------------------------------------------------------------------
# Flat tables.
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("surface", ["first", "last"])
def test_flat_tables_give_every_quantity_of_the_grey_call_bit_for_bit(fine, method, surface):
    spec = fine[0]
    cloud = grey_cloud()
    for bands in (None, EDGES):
        common = dict(surface=surface, quantities=quantities_of(method), band_edges=bands)
        grey = call(spec, method, fine, **common, **cloud)
        for m in (2, 5):
            knots = np.linspace(590., 710., m) if m == 5 else np.array([650.005, 650.015])
            got = call(spec, method, fine, scatterer_wavenumber=knots, **common,
                       **flat(cloud, m))
            for q in quantities_of(method):
                assert np.array_equal(np.asarray(got[q]), np.asarray(grey[q]), equal_nan=True), \
                    (bands is not None, m, q)
        assert np.any(np.asarray(grey["heating_rate"]) != 0.)


# ---------------------------------------------------------------------------------------------
# Runs.
@pytest.mark.parametrize("method", METHODS)
def test_one_path_per_run_gives_the_same_bits(fine, method):
    spec = fine[0]
    n = spec.grid.size
    cloud = spectral_cloud()
    quantities = quantities_of(method)
    calls = [dict(quantities=quantities), dict(surface="last", quantities=("upward_flux",)),
             dict(band_edges=np.arange(600., 700.1, 2.5), quantities=quantities)]
    whole = [call(spec, method, fine, scatterer_wavenumber=KNOTS, **cloud, **one)
             for one in calls]
    other = spectroscopy(SHAPE)
    # beta, two work rows and the interface rows on the grid per level (four of them in the
    # shortwave, two in the longwave), seven levels a path, and the knot table's few bytes: one
    # path fits, two do not (with bands, where the interface rows do not count, two paths of the
    # shortwave call fit and three do not).
    blocks = 7 if method == "compute_solar_flux" else 5
    other.device_output_limit = int(1.5*blocks*7*n*8)
    for one, expect in zip(calls, whole):
        got = call(other, method, fine, scatterer_wavenumber=KNOTS, **cloud, **one)
        for q in one["quantities"]:
            assert np.array_equal(np.asarray(got[q]), np.asarray(expect[q]), equal_nan=True), q
    # The table counts: a limit that holds the blocks of one path to the byte (beta and the two
    # work rows; their rows are as long as the engine's grid) does not hold it.
    v0, vn, n_per_v = synthetic.grid_arguments(spec.grid)
    other.device_output_limit = 3*7*(vn - v0)*n_per_v*8
    with pytest.raises(ValueError, match="does not hold one path"):
        call(other, method, fine, scatterer_wavenumber=KNOTS, band_edges=[600., 650.],
             quantities=("upward_flux",), **cloud)
    call(other, method, fine, band_edges=[600., 650.], quantities=("upward_flux",))


# ---------------------------------------------------------------------------------------------
# Properties.
def test_a_conservative_spectral_cloud_over_a_white_surface_keeps_the_net_flux_at_zero(fine):
    """Layers of no thickness hold no gas: a spectral scatterer with omega_c = 1 at every knot
    over A = 1 sends all of F0 back to space, and the net flux is 0 at every interface."""
    spec = fine[0]
    cloud = spectral_cloud()
    cloud[OMEGA] = np.ones_like(cloud[OMEGA])
    _, _, thickness, sigma, _ = fine
    out = spec.compute_solar_flux_spectral(
        0.*thickness, MU0, surface_albedo=1., quantities=paths.SOLAR_FLUX_INTERFACE_QUANTITIES,
        remove_pedestal=False, scatterer_wavenumber=KNOTS, **cloud)
    f0 = np.asarray(out["direct_irradiance"])[:, 7]
    up, down = np.asarray(out["upward_flux"]), np.asarray(out["downward_flux"])
    allowed = SHORTWAVE_BOUND*f0.astype(LD)
    assert np.all(f0 > 0.) and np.all(np.isfinite(up)) and np.all(np.isfinite(down))
    assert np.all(np.abs(up[:, 7].astype(LD) - f0) <= allowed)
    print("net flux / bound: %.3g" % float(np.max(
        np.abs(up.astype(LD) - down)/allowed[:, None, :])))
    assert np.all(np.abs(up.astype(LD) - down) <= allowed[:, None, :])
    assert np.any(np.asarray(out["diffuse_downward_flux"])[:, 0] > 0.)


def test_equal_temperatures_give_the_isothermal_spectral_call_bit_for_bit():
    """Every level and interface of a path at one temperature: dB = 0 everywhere."""
    spec = spectroscopy(SHAPE, temperature=260.)
    thickness = thickness_for(total_of(spec))
    interfaces = np.full((SHAPE[0], SHAPE[1] + 1), 260.)
    common = dict(surface_emissivity=EMISSIVITY, quantities=THERMAL, remove_pedestal=False,
                  scatterer_wavenumber=KNOTS)
    common.update(spectral_cloud())
    linear = spec.compute_thermal_flux_spectral(thickness, SURFACE_T,
                                                interface_temperature=interfaces, **common)
    plain = spec.compute_thermal_flux_spectral(thickness, SURFACE_T, **common)
    for q in THERMAL:
        assert np.array_equal(np.asarray(linear[q]), np.asarray(plain[q])), q

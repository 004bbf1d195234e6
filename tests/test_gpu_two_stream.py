"""Spectroscopy.compute_solar_flux on the GPU, on the synthetic database of the other product
tests: against the long-double mirror of its definition (tests/two_stream_cases.py) over
compute_absorption("total") of the same Spectroscopy, against what two-stream theory demands
(conservation), against compute_solar where nothing scatters, runs of whole paths, bands and
heating rates.

Bounds, none taken from the code under test.  Every flux is within (4*E_cpu + 1e-13)*F0 of the
long-double mirror, F0 = mu0*S the column's incident flux as the call returned it: E_cpu =
1.61e-11 is the worst |float64 mirror - long-double mirror|/F0 that tests/test_two_stream_host.py
measures over the committed case tables (recorded as two_stream_cases.E_CPU = 1.7e-11); the factor
4 because the device's exp and expm1 are a few ulp where numpy's are about one and both pass
through the same adding recurrences; the floor for benign columns.  Without scattering the direct
irradiance is within 4*eps*sum_l(1 + t_l/mu0) relative of compute_solar's (each factor's exponent is
rounded once, here per level and there in the running sum) and the upward flux at the surface is
A times the downward flux there to 4*eps.  Band fluxes are within 1e-12 relative of the numpy
reduction of the grid results, as tests/test_gpu_flux.py holds its own."""
import numpy as np
import pytest

from pylbl_amd import paths, synthetic
from tests import two_stream_cases as ts
from tests.test_gpu_flux import band_fluxes, spectroscopy, thickness_for, total_of

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
EPS = 2.**-52
SHAPE = (3, 7)
MU0 = np.array([1., 0.35, 0.08])
ALBEDO = np.array([1., 0.3, 0.])
FLUX_BOUND = LD(4.*ts.E_CPU + ts.FLUX_FLOOR)
INTERFACES = paths.SOLAR_FLUX_INTERFACE_QUANTITIES
ALL = paths.SOLAR_FLUX_QUANTITIES
NAMES = dict(zip(INTERFACES, ts.QUANTITIES))


def cloud():
    """A grey scatterer in levels 2 and 3 of every path, conservative in path 1."""
    tau_c = np.zeros(SHAPE)
    tau_c[:, 2], tau_c[:, 3] = [0.5, 8., 40.], [2., 0.05, 3.]
    omega_c = np.full(SHAPE, 0.96)
    omega_c[1] = 1.
    g_c = np.full(SHAPE, 0.85)
    g_c[2] = 0.3
    return dict(scatterer_optical_depth=tau_c, scatterer_single_scattering_albedo=omega_c,
                scatterer_asymmetry=g_c)


@pytest.fixture(scope="module")
def fine():
    """(spec, beta [3, 7, N], thickness, sigma on the grid, the grid results of every quantity
    per surface): the references every test shares."""
    spec = spectroscopy(SHAPE)
    beta = total_of(spec)
    assert np.all(beta >= 0.)
    thickness = thickness_for(beta)
    # Air columns are ~1e25 m-2 per metre: cross-sections that put the Rayleigh depth of a level
    # between 0 and ~0.3, with columns where there is none.
    column = spec.atmosphere.pressure/(paths.K_B*spec.atmosphere.temperature)*thickness
    sigma = np.random.default_rng(9).uniform(0., 0.3, size=spec.grid.size)/column.max()
    sigma[::11] = 0.
    results = {surface: spec.compute_solar_flux(
        thickness, MU0, surface=surface, surface_albedo=ALBEDO, rayleigh_cross_section=sigma,
        quantities=ALL, remove_pedestal=False, **cloud()) for surface in ("first", "last")}
    return spec, beta, thickness, sigma, results


def mirror_of(spec, beta, request, sigma, surface, f0):
    """The long-double mirror of a call: {quantity: [3, 8, N]} on the result's interface dim."""
    levels = beta.shape[1]
    order = list(range(levels - 1, -1, -1)) if surface == "first" else list(range(levels))
    table = request.level_table.reshape(3, levels, 5)[:, order]          # the Sun's order
    inputs = ts.layer_inputs(np.moveaxis(table, 1, 0)[:, :, None, :], MU0[None, :, None],
                             np.moveaxis(beta[:, order], 1, 0), sigma[None, None, :])
    albedo = request.albedo[:, None] if request.albedo.ndim == 1 else \
        paths.interpolate_emissivity(request.albedo_knots, request.albedo, spec.grid)
    got = ts.adding(LD, ts.layer(LD, inputs), albedo, f0)
    out = {}
    for q, name in NAMES.items():
        rows = np.moveaxis(got[name], 0, 1)                             # [3, 8, N], interface 0 first
        out[q] = rows[:, ::-1] if surface == "first" else rows
    return out


def request_of(spec, thickness, surface, sigma, rayleigh=True, albedo=ALBEDO, knots=None,
               scatterers=None):
    scatterers = cloud() if scatterers is None else scatterers
    return spec._solar_flux_request(
        thickness, MU0, None, None, 1., surface, albedo, knots, rayleigh, sigma,
        scatterers.get("scatterer_optical_depth"),
        scatterers.get("scatterer_single_scattering_albedo"),
        scatterers.get("scatterer_asymmetry"), INTERFACES, None, "reference")


def close(what, out, reference, f0):
    for q in INTERFACES:
        got = np.asarray(out[q])
        assert got.shape == reference[q].shape and np.all(np.isfinite(got)), (what, q)
        error = np.abs(got.astype(LD) - reference[q])
        allowed = FLUX_BOUND*f0[:, None, :].astype(LD)
        print("%s, %s: worst error / bound %.3g" % (what, q, float(np.max(error/allowed))))
        assert np.all(error <= allowed), (what, q)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_every_quantity_matches_the_mirror(fine, surface):
    spec, beta, thickness, sigma, results = fine
    out = results[surface]
    assert set(out) == set(ALL) | {"wavenumber"}
    space = 7 if surface == "first" else 0
    direct = np.asarray(out["direct_irradiance"])
    assert direct.shape == (3, 8, spec.grid.size)
    # F0 = mu0*S of the Sun's blackbody: compute_solar's, bit for bit.
    f0 = direct[:, space]
    sun = np.asarray(spec.compute_solar(thickness, MU0, surface=surface,
                                        remove_pedestal=False)["direct_irradiance"])[:, space]
    assert np.array_equal(f0, sun) and np.all(f0 > 0.)
    request = request_of(spec, thickness, surface, sigma)
    close(surface, out, mirror_of(spec, beta, request, sigma, surface, f0), f0)
    up, down = np.asarray(out["upward_flux"]), np.asarray(out["downward_flux"])
    assert np.array_equal(down, direct + np.asarray(out["diffuse_downward_flux"]))
    assert np.all(np.asarray(out["diffuse_downward_flux"])[:, space] == 0.)
    expect = paths.heating_rate(up, down, spec.atmosphere.pressure, spec.atmosphere.temperature,
                                thickness, surface)
    assert np.array_equal(np.asarray(out["heating_rate"]), expect)
    # A black surface sends nothing up; light is absorbed, so heating somewhere.
    ground = 0 if surface == "first" else 7
    assert np.all(up[2, ground] == 0.) and np.any(expect > 0.)


def test_the_default_fit_and_a_spectral_albedo_match_the_mirror(fine):
    spec, beta, thickness, _, results = fine
    knots, values = np.array([590., 650., 720.]), np.array([0., 0.5, 1.])
    out = spec.compute_solar_flux(thickness, MU0, surface_albedo=values, albedo_wavenumber=knots,
                                  quantities=INTERFACES, remove_pedestal=False, **cloud())
    f0 = np.asarray(results["first"]["direct_irradiance"])[:, 7]
    assert np.array_equal(np.asarray(out["direct_irradiance"])[:, 7], f0)
    sigma = paths.rayleigh_cross_section(spec.grid)
    request = request_of(spec, thickness, "first", None, albedo=values, knots=knots)
    close("fit, spectral albedo", out, mirror_of(spec, beta, request, sigma, "first", f0), f0)


def test_nothing_is_lost_without_absorption(fine):
    """Layers of no thickness hold no gas: a conservative scatterer over a white surface sends
    all of F0 back to space, and the net flux is 0 at every interface."""
    spec, beta, thickness, sigma, results = fine
    scatterers = cloud()
    scatterers["scatterer_single_scattering_albedo"] = np.ones(SHAPE)
    out = spec.compute_solar_flux(0.*thickness, MU0, surface_albedo=1., quantities=INTERFACES,
                                  remove_pedestal=False, **scatterers)
    f0 = np.asarray(results["first"]["direct_irradiance"])[:, 7]
    up, down = np.asarray(out["upward_flux"]), np.asarray(out["downward_flux"])
    allowed = FLUX_BOUND*f0.astype(LD)
    assert np.all(np.abs(up[:, 7].astype(LD) - f0) <= allowed)
    assert np.all(np.abs(up.astype(LD) - down) <= allowed[:, None, :])
    assert np.any(np.asarray(out["diffuse_downward_flux"])[:, 0] > 0.)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_without_scattering_it_is_compute_solars_beam(fine, surface):
    spec, beta, thickness, sigma, results = fine
    out = spec.compute_solar_flux(thickness, MU0, surface=surface, surface_albedo=ALBEDO,
                                  rayleigh=False, quantities=INTERFACES, remove_pedestal=False)
    beam = np.asarray(spec.compute_solar(thickness, MU0, surface=surface,
                                         remove_pedestal=False)["direct_irradiance"])
    direct = np.asarray(out["direct_irradiance"])
    # sum_l (1 + t_l/mu0) over the levels above each interface, in the Sun's order.
    t = thickness[:, :, None]*beta/MU0[:, None, None]
    order = slice(None, None, -1) if surface == "first" else slice(None)
    above = np.cumsum((1. + t)[:, order], axis=1)
    above = np.concatenate([np.zeros((3, 1, spec.grid.size)), above], axis=1)[:, order]
    error = np.abs(direct.astype(LD) - beam)
    assert np.all(error <= 4*EPS*above*beam.astype(LD))
    assert np.all(np.asarray(out["diffuse_downward_flux"]) == 0.)
    ground = 0 if surface == "first" else 7
    up, down = np.asarray(out["upward_flux"]), np.asarray(out["downward_flux"])
    assert np.all(np.abs(up[:, ground].astype(LD) - ALBEDO[:, None]*down[:, ground].astype(LD))
                  <= 4*EPS*down[:, ground])
    assert np.any(up[:2, ground] > 0.)


def test_one_path_per_run_gives_the_same_bits(fine):
    spec, beta, thickness, sigma, results = fine
    n = spec.grid.size
    edges = np.arange(600., 700.1, 2.5)
    calls = [dict(quantities=ALL), dict(surface="last", quantities=("upward_flux",)),
             dict(band_edges=edges, quantities=ALL)]
    common = dict(surface_albedo=ALBEDO, rayleigh_cross_section=sigma, remove_pedestal=False)
    common.update(cloud())
    whole = [spec.compute_solar_flux(thickness, MU0, **common, **call) for call in calls]
    other = spectroscopy(SHAPE)
    # beta, two work rows and four interface rows per level, seven levels a path: one path fits,
    # two do not (with bands, where the interface rows do not count, two fit and three do not).
    other.device_output_limit = int(1.5*7*7*n*8)
    for call, expect in zip(calls, whole):
        got = other.compute_solar_flux(thickness, MU0, **common, **call)
        for q in call["quantities"]:
            assert np.array_equal(np.asarray(got[q]), np.asarray(expect[q]), equal_nan=True), q
    other.device_output_limit = int(0.9*4*7*n*8)
    with pytest.raises(ValueError, match="does not hold one path"):
        other.compute_solar_flux(thickness, MU0, quantities=("upward_flux",))


@pytest.mark.parametrize("surface", ["first", "last"])
def test_band_edges_reduce_the_grid_results(fine, surface):
    spec, beta, thickness, sigma, results = fine
    edges = np.concatenate([[550., 600.5, 600.5005], np.arange(601.3, 700.1, 1.), [720.]])
    out = spec.compute_solar_flux(thickness, MU0, surface=surface, surface_albedo=ALBEDO,
                                  rayleigh_cross_section=sigma, quantities=ALL, band_edges=edges,
                                  remove_pedestal=False, **cloud())
    starts = np.searchsorted(spec.grid, edges, side="left")
    _, _, n_per_v = synthetic.grid_arguments(spec.grid)
    grid = results[surface]
    for q in INTERFACES:
        expect = band_fluxes(np.asarray(grid[q]), starts, n_per_v)
        got = np.asarray(out[q])
        assert np.array_equal(np.isnan(got), np.isnan(expect)) and np.any(np.isnan(expect))
        ok = ~np.isnan(expect)
        assert np.all(np.abs(got[ok] - expect[ok]) <= 1e-12*np.abs(expect[ok])), q
    up, down = np.asarray(out["upward_flux"]), np.asarray(out["downward_flux"])
    expect = paths.heating_rate(up, down, spec.atmosphere.pressure, spec.atmosphere.temperature,
                                thickness, surface)
    assert np.array_equal(np.asarray(out["heating_rate"]), expect, equal_nan=True)
    assert np.array_equal(np.asarray(out["band_points"]), np.diff(starts))

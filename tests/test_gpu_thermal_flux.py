"""Spectroscopy.compute_thermal_flux on the GPU, on the synthetic database of the other product
tests: against the long-double mirror of its definition (tests/thermal_cases.py) over
compute_absorption("total") of the same Spectroscopy, on the grid and in bands, against
compute_flux with one angle where nothing scatters, what an opaque cloud does to the fluxes, heating
rates, and runs of whole paths.

Bounds, none taken from the code under test.  Every flux is within (4*E_cpu + 1e-13)*scale of the
long-double mirror, scale = pi*max B(nu, T) over the path's level temperatures and T_s: E_cpu =
6.64e-15 is the worst |float64 mirror - long-double mirror|/scale that tests/test_thermal_host.py
measures over the committed case tables (recorded as thermal_cases.E_CPU = 7e-15); the factor 4
because the device's exp and expm1 are a few ulp where numpy's are about one and both pass through
the same adding recurrences; the floor for benign columns.  A band flux is the mean of its
columns' fluxes times the band's width, so it is held to the same multiple of the band's mean
scale.  Without scatterers the result is within 16*2^-53*(L + 1)*scale of
compute_flux(angles=([1/D], [1.])): x = D*(s*beta) against (s/mu)*beta differs by at most 4 ulp,
so exp(-x) by under 1.5*2^-53 absolute, about six more roundings where pi enters, at most 8*2^-53
per level and sweep, two sweeps."""
import numpy as np
import pytest

from pylbl_amd import paths, synthetic
from tests import thermal_cases as tc
from tests.test_gpu_flux import band_fluxes, spectroscopy, thickness_for, total_of

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
SHAPE = (3, 7)
SURFACE_T = np.array([300., 288., 270.])
EMISSIVITY = np.array([1., 0.3, 0.])
FLUX_BOUND = LD(4.*tc.E_CPU + tc.FLUX_FLOOR)
FLUXES = ("upward_flux", "downward_flux")
ALL = paths.THERMAL_FLUX_QUANTITIES
NAMES = dict(zip(FLUXES, tc.QUANTITIES))


def cloud():
    """A grey scatterer in levels 2 and 3 of every path, conservative in path 1."""
    tau_c = np.zeros(SHAPE)
    tau_c[:, 2], tau_c[:, 3] = [0.5, 8., 40.], [2., 0.05, 3.]
    omega_c = np.full(SHAPE, 0.6)
    omega_c[1] = 1.
    g_c = np.full(SHAPE, 0.85)
    g_c[2] = 0.3
    return dict(scatterer_optical_depth=tau_c, scatterer_single_scattering_albedo=omega_c,
                scatterer_asymmetry=g_c)


@pytest.fixture(scope="module")
def fine():
    """(spec, beta [3, 7, N], thickness, the grid results of every quantity per surface): the
    references every test shares."""
    spec = spectroscopy(SHAPE)
    beta = total_of(spec)
    assert np.all(beta >= 0.)
    thickness = thickness_for(beta)
    results = {surface: spec.compute_thermal_flux(
        thickness, SURFACE_T, EMISSIVITY, surface=surface, quantities=ALL, remove_pedestal=False,
        **cloud()) for surface in ("first", "last")}
    return spec, beta, thickness, results


def request_of(spec, thickness, surface, emissivity=EMISSIVITY, knots=None, diffusivity=1.66,
               scatterers=None):
    scatterers = cloud() if scatterers is None else scatterers
    return spec._thermal_flux_request(
        thickness, SURFACE_T, emissivity, knots, surface, diffusivity,
        scatterers.get("scatterer_optical_depth"),
        scatterers.get("scatterer_single_scattering_albedo"),
        scatterers.get("scatterer_asymmetry"), FLUXES, None, "reference")


def mirror_of(spec, beta, request):
    """The long-double mirror of a call: ({quantity: [3, 8, N]} on the result's interface dim,
    scale [3, 1, N])."""
    levels = beta.shape[1]
    emissivity = request.surface_emissivity if request.emissivity_knots is None else \
        paths.interpolate_emissivity(request.emissivity_knots, request.surface_emissivity,
                                     spec.grid)
    inputs = tc.Inputs("call", spec.grid, beta.reshape(3*levels, -1), request.level_table,
                       request.surface_temperature, emissivity, request.diffusivity)
    first = request.surface == "first"
    got = tc.mirror(LD, inputs, first)
    out = {}
    for q, name in NAMES.items():
        below = got[name].reshape(3, levels, -1)
        top = got["top_" + name][:, None, :]
        out[q] = np.concatenate([below, top] if first else [top, below], axis=1)
    return out, got["scale"][:, None, :]


_CLOUD_MIRRORS = {}


def cloud_mirror(spec, beta, thickness, surface):
    """mirror_of the fixture's call for `surface`, formed once."""
    if surface not in _CLOUD_MIRRORS:
        _CLOUD_MIRRORS[surface] = mirror_of(spec, beta, request_of(spec, thickness, surface))
    return _CLOUD_MIRRORS[surface]


def close(what, out, reference, scale):
    for q in FLUXES:
        got = np.asarray(out[q])
        assert got.shape == reference[q].shape and np.all(np.isfinite(got)), (what, q)
        error = np.abs(got.astype(LD) - reference[q])
        allowed = FLUX_BOUND*scale
        print("%s, %s: worst error / bound %.3g" % (what, q, float(np.max(error/allowed))))
        assert np.all(error <= allowed), (what, q)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_every_quantity_matches_the_mirror(fine, surface):
    spec, beta, thickness, results = fine
    out = results[surface]
    assert set(out) == set(ALL) | {"wavenumber"}
    up, down = np.asarray(out["upward_flux"]), np.asarray(out["downward_flux"])
    assert up.shape == down.shape == (3, 8, spec.grid.size)
    reference, scale = cloud_mirror(spec, beta, thickness, surface)
    assert np.all(scale > 0.)
    close(surface, out, reference, scale)
    space, ground = (7, 0) if surface == "first" else (0, 7)
    assert np.all(down[:, space] == 0.) and np.all(up[:, space] > 0.)
    # A mirror for a surface sends back what comes down.
    assert np.array_equal(up[2, ground], down[2, ground])
    expect = paths.heating_rate(up, down, spec.atmosphere.pressure, spec.atmosphere.temperature,
                                thickness, surface)
    assert np.array_equal(np.asarray(out["heating_rate"]), expect)
    assert np.any(expect < 0.)


def test_a_spectral_emissivity_and_the_hemispheric_mean_match_the_mirror(fine):
    spec, beta, thickness, _ = fine
    knots, values = np.array([590., 650., 720.]), np.array([0., 0.5, 1.])
    out = spec.compute_thermal_flux(thickness, SURFACE_T, values, emissivity_wavenumber=knots,
                                    diffusivity=2., quantities=FLUXES, remove_pedestal=False,
                                    **cloud())
    request = request_of(spec, thickness, "first", emissivity=values, knots=knots, diffusivity=2.)
    reference, scale = mirror_of(spec, beta, request)
    close("spectral emissivity, D = 2", out, reference, scale)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_band_results_match_the_mirror(fine, surface):
    spec, beta, thickness, results = fine
    edges = np.concatenate([[550., 600.5, 600.5005], np.arange(601.3, 700.1, 1.), [720.]])
    out = spec.compute_thermal_flux(thickness, SURFACE_T, EMISSIVITY, surface=surface,
                                    quantities=ALL, band_edges=edges, remove_pedestal=False,
                                    **cloud())
    starts = np.searchsorted(spec.grid, edges, side="left")
    _, _, n_per_v = synthetic.grid_arguments(spec.grid)
    reference, scale = cloud_mirror(spec, beta, thickness, surface)
    allowed = FLUX_BOUND*band_fluxes(np.broadcast_to(scale, reference["upward_flux"].shape),
                                     starts, LD(n_per_v))
    for q in FLUXES:
        expect = band_fluxes(reference[q], starts, LD(n_per_v))
        got = np.asarray(out[q])
        assert np.array_equal(np.isnan(got), np.isnan(expect)) and np.any(np.isnan(expect))
        ok = ~np.isnan(expect)
        error = np.abs(got[ok].astype(LD) - expect[ok])
        print("%s bands, %s: worst error / bound %.3g" % (
            surface, q, float(np.max(error/allowed[ok]))))
        assert np.all(error <= allowed[ok]), q
    up, down = np.asarray(out["upward_flux"]), np.asarray(out["downward_flux"])
    expect = paths.heating_rate(up, down, spec.atmosphere.pressure, spec.atmosphere.temperature,
                                thickness, surface)
    assert np.array_equal(np.asarray(out["heating_rate"]), expect, equal_nan=True)
    assert np.array_equal(np.asarray(out["band_points"]), np.diff(starts))


@pytest.mark.parametrize("d", [1.66, 2.])
@pytest.mark.parametrize("surface", ["first", "last"])
def test_without_scatterers_it_is_compute_flux_with_one_angle(fine, surface, d):
    spec, beta, thickness, _ = fine
    out = spec.compute_thermal_flux(thickness, SURFACE_T, EMISSIVITY, surface=surface,
                                    diffusivity=d, quantities=FLUXES, remove_pedestal=False)
    plain = spec.compute_flux(thickness, SURFACE_T, EMISSIVITY, surface=surface,
                              angles=([1./d], [1.]), quantities=FLUXES, remove_pedestal=False)
    _, scale = mirror_of(spec, beta, request_of(spec, thickness, surface, diffusivity=d,
                                                scatterers={}))
    bound = LD(16.*2.**-53*(SHAPE[1] + 1))*scale
    for q in FLUXES:
        error = np.abs(np.asarray(out[q]).astype(LD) - np.asarray(plain[q]))
        print("D = %g, %s, %s: worst error / bound %.3g" % (
            d, surface, q, float(np.max(error/bound))))
        assert np.all(error <= bound), q


def test_an_opaque_cloud_cools_the_top_and_warms_the_surface(fine):
    """tau_c = 50, omega_c = 0.5 in level 4 (colder than the surface): in a window column less
    goes out to space than under a clear sky, and more comes down at the surface."""
    spec, beta, thickness, _ = fine
    tau_c = np.zeros(SHAPE)
    tau_c[:, 4] = 50.
    opaque = dict(scatterer_optical_depth=tau_c,
                  scatterer_single_scattering_albedo=np.full(SHAPE, 0.5),
                  scatterer_asymmetry=np.full(SHAPE, 0.85))
    cloudy = spec.compute_thermal_flux(thickness, SURFACE_T, quantities=FLUXES,
                                       remove_pedestal=False, **opaque)
    clear = spec.compute_thermal_flux(thickness, SURFACE_T, quantities=FLUXES,
                                      remove_pedestal=False)
    assert np.all(spec.atmosphere.temperature[:, 4] < SURFACE_T - 10.)
    window = np.argmin(np.sum(thickness[:, :, None]*beta, axis=1), axis=1)
    for p in range(3):
        j = window[p]
        depth = np.sum(thickness[p]*beta[p, :, j])
        top = [np.asarray(x["upward_flux"])[p, 7, j] for x in (cloudy, clear)]
        ground = [np.asarray(x["downward_flux"])[p, 0, j] for x in (cloudy, clear)]
        print("path %d, column %d, optical depth %.3g: up at the top %.6g against %.6g, down at "
              "the surface %.6g against %.6g" % (p, j, depth, *top, *ground))
        assert depth < 1.
        assert top[0] < top[1] and ground[0] > ground[1]


def test_both_surface_ends_cut_into_runs_give_the_same_bits(fine):
    spec, beta, thickness, results = fine
    n = spec.grid.size
    edges = np.arange(600., 700.1, 2.5)
    calls = [dict(quantities=ALL), dict(surface="last", quantities=ALL),
             dict(surface="last", quantities=("upward_flux",)),
             dict(band_edges=edges, quantities=ALL)]
    common = dict(surface_emissivity=EMISSIVITY, remove_pedestal=False)
    common.update(cloud())
    whole = [results["first"], results["last"]] + \
        [spec.compute_thermal_flux(thickness, SURFACE_T, **common, **call) for call in calls[2:]]
    other = spectroscopy(SHAPE)
    # beta, two work rows and two flux rows per level, seven levels a path: two paths fit, three
    # do not -- two runs (with bands, where the flux rows do not count, three fit: one run more
    # than the limit needs is never made).
    other.device_output_limit = int(2.5*5*7*n*8)
    for call, expect in zip(calls, whole):
        got = other.compute_thermal_flux(thickness, SURFACE_T, **common, **call)
        for q in call["quantities"]:
            assert np.array_equal(np.asarray(got[q]), np.asarray(expect[q]), equal_nan=True), q
    # One path per run.
    other.device_output_limit = int(1.5*5*7*n*8)
    got = other.compute_thermal_flux(thickness, SURFACE_T, **common, quantities=ALL)
    for q in ALL:
        assert np.array_equal(np.asarray(got[q]), np.asarray(results["first"][q])), q
    other.device_output_limit = int(0.9*3*7*n*8)
    with pytest.raises(ValueError, match="does not hold one path"):
        other.compute_thermal_flux(thickness, SURFACE_T, quantities=("upward_flux",))

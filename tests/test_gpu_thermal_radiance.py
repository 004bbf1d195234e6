"""Spectroscopy.compute_thermal_radiance on the GPU, on the synthetic database of the other product
tests (400 grid points, 3 paths of 4 levels): against the long-double mirror of its definition
(tests/thermal_radiance_cases.py) fed compute_absorption("total") and compute_thermal_flux's fluxes
of the same Spectroscopy, against compute_radiance bit for bit where nothing scatters, with an
instrument against Instrument.response applied in numpy, in bands, cut into runs of whole paths,
and beside the calls it shares kernels and blocks with.

Bounds, none taken from the code under test.  Every radiance is within (4*E_cpu + 1e-13)*scale of
the long-double mirror, scale = max B(nu, T) over the path's level temperatures and T_s: E_cpu =
1.9e-11 is the worst |float64 mirror - long-double mirror|/scale that
tests/test_thermal_radiance_host.py measures over the committed case tables (recorded as
thermal_radiance_cases.E_CPU = 2e-11); the factor 4 because the device's exp and expm1 are a few
ulp where numpy's are about one; the floor for benign columns.  Channel radiances are held to
tests/test_gpu_instrument.py's bound for compute_radiance, 1e-12*sum|w v|/|sum w|; band means to
1e-12*magnitude of the long-double means of the fine result."""
import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, paths, synthetic
from pylbl_amd.instrument import Instrument, brightness_temperature
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as rc
from tests import test_gpu_flux as flux_tests
from tests.test_gpu_flux import thickness_for, total_of
from tests.test_gpu_instrument import check as check_channels

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
SHAPE = (3, 4)
GRID = np.arange(600., 604., 0.01)
SURFACE_T = np.array([300., 288., 270.])
EMISSIVITY = np.array([1., 0.3, 0.])
MU = np.array([1., 0.6, 0.05])
BOUND = LD(4.*rc.E_CPU + rc.FLOOR)
BOTH = ("radiance", "brightness_temperature")


def spectroscopy(**keywords):
    if "small" not in flux_tests._TABLES:
        flux_tests._TABLES["small"] = [
            synthetic.line_table(name, 576., 724., num_lines=3000, seed=40 + i)
            for i, name in enumerate(flux_tests.GASES)]
    return Spectroscopy(flux_tests.atmosphere(SHAPE), GRID,
                        MemoryDatabase(flux_tests._TABLES["small"]), **keywords)


def cloud():
    """A grey scatterer in levels 1 and 2 of every path, conservative in path 1."""
    tau_c = np.zeros(SHAPE)
    tau_c[:, 1], tau_c[:, 2] = [0.5, 8., 40.], [2., 0.05, 3.]
    omega_c = np.full(SHAPE, 0.6)
    omega_c[1] = 1.
    g_c = np.full(SHAPE, 0.85)
    g_c[2] = 0.3
    return dict(scatterer_optical_depth=tau_c, scatterer_single_scattering_albedo=omega_c,
                scatterer_asymmetry=g_c)


@pytest.fixture(scope="module")
def fine():
    """(spec, beta [3, 4, N], thickness, the grid results per surface): what every test shares."""
    spec = spectroscopy()
    beta = total_of(spec)
    assert np.all(beta >= 0.) and spec.grid.size == 400
    thickness = thickness_for(beta)
    results = {surface: spec.compute_thermal_radiance(
        thickness, SURFACE_T, MU, EMISSIVITY, surface=surface, quantities=BOTH,
        remove_pedestal=False, **cloud()) for surface in ("first", "last")}
    return spec, beta, thickness, results


def mirror_of(spec, beta, thickness, surface, emissivity=EMISSIVITY, knots=None, diffusivity=1.66):
    """The long-double mirror of a call, fed the fluxes compute_thermal_flux returns for it."""
    scatterers = cloud()
    fluxes = spec.compute_thermal_flux(
        thickness, SURFACE_T, emissivity, emissivity_wavenumber=knots, surface=surface,
        diffusivity=diffusivity, remove_pedestal=False, **scatterers)
    request = spec._thermal_flux_request(
        thickness, SURFACE_T, emissivity, knots, surface, diffusivity,
        scatterers["scatterer_optical_depth"], scatterers["scatterer_single_scattering_albedo"],
        scatterers["scatterer_asymmetry"], ("upward_flux", "downward_flux"), None, "reference")
    eps = request.surface_emissivity if knots is None else paths.interpolate_emissivity(
        request.emissivity_knots, request.surface_emissivity, spec.grid)
    levels = SHAPE[1]
    inputs = tc.Inputs("call", spec.grid, beta.reshape(3*levels, -1), request.level_table,
                       request.surface_temperature, eps, request.diffusivity)
    first = surface == "first"
    # The rows at the interface below each level: interface l with the surface behind level 0,
    # interface l + 1 with it behind the last level.
    below = slice(0, levels) if first else slice(1, levels + 1)
    rows = {name: np.ascontiguousarray(np.asarray(fluxes[q])[:, below].reshape(3*levels, -1))
            for q, name in (("upward_flux", "up"), ("downward_flux", "down"))}
    return rc.mirror(LD, inputs, MU, first, rows)


def close(what, got, expect):
    value = np.asarray(got["radiance"])
    assert value.shape == expect["radiance"].shape and np.all(np.isfinite(value)), what
    error = np.abs(value.astype(LD) - expect["radiance"])
    allowed = BOUND*expect["scale"]
    print("%s: worst error / bound %.3g" % (what, float(np.max(error/allowed))))
    assert np.all(allowed > 0.) and np.all(error <= allowed), what


@pytest.mark.parametrize("surface", ["first", "last"])
def test_every_quantity_matches_the_mirror(fine, surface):
    spec, beta, thickness, results = fine
    out = results[surface]
    assert set(out) == set(BOTH) | {"wavenumber"}
    assert np.asarray(out["radiance"]).shape == (3, spec.grid.size)
    close(surface, out, mirror_of(spec, beta, thickness, surface))
    inverted = cases.brightness(LD, spec.grid[None, :], np.asarray(out["radiance"]))
    got = np.asarray(out["brightness_temperature"])
    assert np.all(got > 0.) and np.all(np.abs(got.astype(LD) - inverted) <= LD(1e-13)*inverted)


def test_a_spectral_emissivity_and_the_hemispheric_mean_match_the_mirror(fine):
    spec, beta, thickness, _ = fine
    knots, values = np.array([600.5, 602., 603.]), np.array([0., 0.5, 1.])
    out = spec.compute_thermal_radiance(thickness, SURFACE_T, MU, values,
                                        emissivity_wavenumber=knots, diffusivity=2.,
                                        remove_pedestal=False, **cloud())
    close("spectral emissivity, D = 2", out,
          mirror_of(spec, beta, thickness, "first", emissivity=values, knots=knots,
                    diffusivity=2.))


@pytest.mark.parametrize("surface", ["first", "last"])
def test_without_scatterers_it_is_compute_radiance_bit_for_bit(fine, surface):
    spec, _, thickness, _ = fine
    out = spec.compute_thermal_radiance(thickness, SURFACE_T, surface=surface, quantities=BOTH,
                                        remove_pedestal=False)
    direction = "toward_last" if surface == "first" else "toward_first"
    plain = spec.compute_radiance(thickness, boundary_temperature=SURFACE_T, direction=direction,
                                  quantities=BOTH, remove_pedestal=False)
    for q in BOTH:
        assert np.array_equal(np.asarray(out[q]), np.asarray(plain[q])), q
    assert np.all(np.asarray(out["radiance"]) > 0.)


def test_an_instrument_reduces_the_fine_result(fine):
    spec, _, thickness, results = fine
    centers = np.arange(600.6, 603.4, 0.25)
    for instrument in (Instrument.gaussian(centers, 0.5, half_width=0.55),
                       Instrument.boxcar(centers, 0.7)):
        got = spec.compute_thermal_radiance(thickness, SURFACE_T, MU, EMISSIVITY,
                                            quantities=BOTH, instrument=instrument,
                                            remove_pedestal=False, **cloud())
        assert np.asarray(got["radiance"]).shape == (3, len(centers))
        check_channels(got["radiance"], instrument, spec.grid, results["first"]["radiance"])
        assert np.all(np.isfinite(np.asarray(got["radiance"])))
        expect = brightness_temperature(np.asarray(got["radiance"]), centers)
        assert np.array_equal(np.asarray(got["brightness_temperature"]), expect)
        assert np.array_equal(np.asarray(got["channel_center"]), centers)


def test_band_means_of_the_fine_result(fine):
    spec, _, thickness, results = fine
    edges = np.array([599., 600.503, 601.3, 602.3, 604.5, 605.])
    got = spec.compute_thermal_radiance(thickness, SURFACE_T, MU, EMISSIVITY, band_edges=edges,
                                        remove_pedestal=False, **cloud())
    starts = np.searchsorted(spec.grid, edges, side="left")
    expect = cases.band_means(LD, np.asarray(results["first"]["radiance"]), starts)
    mean = np.asarray(got["radiance"])
    empty = np.isnan(expect)
    assert np.array_equal(np.isnan(mean), empty) and np.any(empty) and np.any(~empty)
    assert np.all(np.abs(mean[~empty].astype(LD) - expect[~empty]) <=
                  LD(1e-12)*np.abs(expect[~empty]))
    assert np.array_equal(np.asarray(got["band_points"]), np.diff(starts))


def test_runs_of_whole_paths_give_the_same_bits(fine):
    spec, _, thickness, results = fine
    n = spec.grid.size
    common = dict(surface_emissivity=EMISSIVITY, remove_pedestal=False, quantities=BOTH)
    common.update(cloud())
    other = spectroscopy()
    # Five blocks per level, four levels a path: two paths fit, then one.
    for paths_per_run in (2.5, 1.5):
        other.device_output_limit = int(paths_per_run*5*4*n*8)
        for surface in ("first", "last"):
            got = other.compute_thermal_radiance(thickness, SURFACE_T, MU, surface=surface,
                                                 **common)
            for q in BOTH:
                assert np.array_equal(np.asarray(got[q]), np.asarray(results[surface][q])), q
    other.device_output_limit = int(0.9*5*4*n*8)
    with pytest.raises(ValueError, match="does not hold one path"):
        other.compute_thermal_radiance(thickness, SURFACE_T)


def test_the_calls_beside_it_return_what_they_returned(fine):
    spec, _, thickness, results = fine
    flux = dict(surface_emissivity=EMISSIVITY, remove_pedestal=False, **cloud())
    before = (spec.compute_thermal_flux(thickness, SURFACE_T, **flux),
              spec.compute_radiance(thickness, boundary_temperature=SURFACE_T,
                                    remove_pedestal=False))
    again = spec.compute_thermal_radiance(thickness, SURFACE_T, MU, EMISSIVITY, quantities=BOTH,
                                          remove_pedestal=False, **cloud())
    after = (spec.compute_thermal_flux(thickness, SURFACE_T, **flux),
             spec.compute_radiance(thickness, boundary_temperature=SURFACE_T,
                                   remove_pedestal=False))
    for q in BOTH:
        assert np.array_equal(np.asarray(again[q]), np.asarray(results["first"][q])), q
    for q in ("upward_flux", "downward_flux"):
        assert np.array_equal(np.asarray(before[0][q]), np.asarray(after[0][q])), q
    assert np.array_equal(np.asarray(before[1]["radiance"]), np.asarray(after[1]["radiance"]))

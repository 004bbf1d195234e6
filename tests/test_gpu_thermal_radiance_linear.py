"""Spectroscopy.compute_thermal_radiance_linear on the GPU, on the synthetic database of the other
product tests (400 grid points, 3 paths of 4 levels): against the long-double mirror of its
definition (tests/thermal_radiance_source_cases.py) fed compute_absorption("total") of the same
Spectroscopy and the mirror's own float64 flux rows, against compute_radiance(source=
"linear_in_tau") bit for bit where nothing scatters, against compute_thermal_radiance bit for bit on
all-cloudy paths of one temperature, with an instrument against Instrument.response applied in
numpy, in bands, cut into runs of whole paths, and beside the calls it shares kernels and blocks
with.

Bounds, none taken from the code under test.  Every radiance is within (4*E_cpu + 1e-13)*scale of
the long-double mirror, scale = max B(nu, T) over the path's interface temperatures and T_s: E_cpu
= 8.78e-10 is the worst |float64 mirror - long-double mirror|/scale that
tests/test_thermal_radiance_source_host.py measures over the committed case tables (recorded as
thermal_radiance_source_cases.E_CPU = 9e-10); the factor 4 because the device's exp and expm1 are a
few ulp where numpy's are about one; the floor for benign columns.  Channel radiances are held to
tests/test_gpu_instrument.py's bound for compute_radiance, 1e-12*sum|w v|/|sum w|; band means to
1e-12*magnitude of the long-double means of the fine result."""
import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, paths
from pylbl_amd.instrument import Instrument, brightness_temperature
from tests import sweep_cases as cases
from tests import thermal_radiance_source_cases as vc
from tests import thermal_source_cases as sc
from tests import test_gpu_flux as flux_tests
from tests import test_gpu_thermal_radiance as grey_tests
from tests.test_gpu_flux import thickness_for, total_of
from tests.test_gpu_instrument import check as check_channels

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
SHAPE, GRID = grey_tests.SHAPE, grey_tests.GRID
SURFACE_T, EMISSIVITY, MU = grey_tests.SURFACE_T, grey_tests.EMISSIVITY, grey_tests.MU
BOUND = LD(4.*vc.E_CPU + vc.FLOOR)
BOTH = ("radiance", "brightness_temperature")
EQUAL_T = 260.
# An inversion in path 0, 30 K jumps in path 1, a smooth profile in path 2; no T_s among them.
INTERFACES = np.array([[215., 240., 232., 262., 255.],
                       [225., 255., 225., 255., 225.],
                       [212., 231., 251., 272., 291.]])
cloud, spectroscopy = grey_tests.cloud, grey_tests.spectroscopy


@pytest.fixture(scope="module")
def fine():
    """(spec, beta [3, 4, N], thickness, the grid results per surface): what every test shares."""
    spec = spectroscopy()
    beta = total_of(spec)
    assert np.all(beta >= 0.) and spec.grid.size == 400
    thickness = thickness_for(beta)
    results = {surface: spec.compute_thermal_radiance_linear(
        thickness, SURFACE_T, INTERFACES, MU, EMISSIVITY, surface=surface, quantities=BOTH,
        remove_pedestal=False, **cloud()) for surface in ("first", "last")}
    return spec, beta, thickness, results


def mirror_of(spec, beta, thickness, surface, emissivity=EMISSIVITY, knots=None, diffusivity=1.66):
    """The long-double mirror of a call, on the mirror's own float64 flux rows."""
    scatterers = cloud()
    request = spec._thermal_radiance_linear_request(
        thickness, SURFACE_T, INTERFACES, MU, emissivity, knots, surface, diffusivity,
        scatterers["scatterer_optical_depth"], scatterers["scatterer_single_scattering_albedo"],
        scatterers["scatterer_asymmetry"], BOTH, None, None, "reference")
    eps = request.surface_emissivity if knots is None else paths.interpolate_emissivity(
        request.emissivity_knots, request.surface_emissivity, spec.grid)
    levels = SHAPE[1]
    inputs = sc.Inputs("call", spec.grid, beta.reshape(3*levels, -1), request.level_table,
                       INTERFACES, request.surface_temperature, eps, request.diffusivity)
    assert np.array_equal(inputs.edges, request.edge_temperature)
    return vc.mirror(LD, inputs, MU, surface == "first")


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
    assert set(out) >= set(BOTH) | {"wavenumber"}
    assert np.asarray(out["radiance"]).shape == (3, spec.grid.size)
    attributes = out.attrs if hasattr(out, "attrs") else out
    assert attributes["source"] == "linear_in_tau"
    close(surface, out, mirror_of(spec, beta, thickness, surface))
    # Brightness temperature on the grid: the inversion of the radiance beside it.
    inverted = cases.brightness(LD, spec.grid[None, :], np.asarray(out["radiance"]))
    got = np.asarray(out["brightness_temperature"])
    assert np.all(got > 0.) and np.all(np.abs(got.astype(LD) - inverted) <= LD(1e-13)*inverted)
    # The source matters: the isothermal call differs by far more than the bound.
    plain = spec.compute_thermal_radiance(fine[2], SURFACE_T, MU, EMISSIVITY, surface=surface,
                                          remove_pedestal=False, **cloud())
    gap = np.abs(np.asarray(plain["radiance"]) - np.asarray(out["radiance"]))
    assert np.max(gap/np.asarray(out["radiance"])) > 1e-3


def test_a_spectral_emissivity_and_the_hemispheric_mean_match_the_mirror(fine):
    spec, beta, thickness, _ = fine
    knots, values = np.array([600.5, 602., 603.]), np.array([0., 0.5, 1.])
    out = spec.compute_thermal_radiance_linear(thickness, SURFACE_T, INTERFACES, MU, values,
                                               emissivity_wavenumber=knots, diffusivity=2.,
                                               remove_pedestal=False, **cloud())
    close("spectral emissivity, D = 2", out,
          mirror_of(spec, beta, thickness, "first", emissivity=values, knots=knots,
                    diffusivity=2.))


@pytest.mark.parametrize("surface", ["first", "last"])
def test_without_scatterers_it_is_compute_radiance_linear_bit_for_bit(fine, surface):
    spec, _, thickness, _ = fine
    out = spec.compute_thermal_radiance_linear(thickness, SURFACE_T, INTERFACES, surface=surface,
                                               quantities=BOTH, remove_pedestal=False)
    direction = "toward_last" if surface == "first" else "toward_first"
    plain = spec.compute_radiance(thickness, boundary_temperature=SURFACE_T, direction=direction,
                                  quantities=BOTH, remove_pedestal=False, source="linear_in_tau",
                                  interface_temperature=INTERFACES)
    for q in BOTH:
        assert np.array_equal(np.asarray(out[q]), np.asarray(plain[q])), q
    assert np.all(np.asarray(out["radiance"]) > 0.)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_one_temperature_on_cloudy_paths_is_compute_thermal_radiance_bit_for_bit(surface):
    """Every level cloudy, every level and interface at one temperature, T_s apart from it."""
    if "small" not in flux_tests._TABLES:
        spectroscopy()                                          # forms the line tables
    spec = Spectroscopy(flux_tests.atmosphere(SHAPE, EQUAL_T), GRID,
                        MemoryDatabase(flux_tests._TABLES["small"]))
    thickness = thickness_for(total_of(spec))
    scatterers = cloud()
    tau_c = scatterers["scatterer_optical_depth"]
    tau_c[:, 0], tau_c[:, 3] = [1e-3, 1., 20.], [0.3, 3., 0.01]
    assert np.all(tau_c > 0.)
    common = dict(surface_emissivity=EMISSIVITY, surface=surface, quantities=BOTH,
                  remove_pedestal=False, **scatterers)
    linear = spec.compute_thermal_radiance_linear(thickness, SURFACE_T,
                                                  np.full((3, 5), EQUAL_T), MU, **common)
    plain = spec.compute_thermal_radiance(thickness, SURFACE_T, MU, **common)
    for q in BOTH:
        assert np.array_equal(np.asarray(linear[q]), np.asarray(plain[q])), q
    assert np.all(np.asarray(linear["radiance"]) > 0.)


def test_an_instrument_reduces_the_fine_result(fine):
    spec, _, thickness, results = fine
    centers = np.arange(600.6, 603.4, 0.25)
    for instrument in (Instrument.gaussian(centers, 0.5, half_width=0.55),
                       Instrument.boxcar(centers, 0.7)):
        got = spec.compute_thermal_radiance_linear(thickness, SURFACE_T, INTERFACES, MU,
                                                   EMISSIVITY, quantities=BOTH,
                                                   instrument=instrument, remove_pedestal=False,
                                                   **cloud())
        assert np.asarray(got["radiance"]).shape == (3, len(centers))
        check_channels(got["radiance"], instrument, spec.grid, results["first"]["radiance"])
        assert np.all(np.isfinite(np.asarray(got["radiance"])))
        # Brightness temperature per channel: the inversion at the channel centres.
        expect = brightness_temperature(np.asarray(got["radiance"]), centers)
        assert np.array_equal(np.asarray(got["brightness_temperature"]), expect)
        assert np.array_equal(np.asarray(got["channel_center"]), centers)


def test_band_means_of_the_fine_result(fine):
    spec, _, thickness, results = fine
    edges = np.array([599., 600.503, 601.3, 602.3, 604.5, 605.])
    got = spec.compute_thermal_radiance_linear(thickness, SURFACE_T, INTERFACES, MU, EMISSIVITY,
                                               band_edges=edges, remove_pedestal=False, **cloud())
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
            got = other.compute_thermal_radiance_linear(thickness, SURFACE_T, INTERFACES, MU,
                                                        surface=surface, **common)
            for q in BOTH:
                assert np.array_equal(np.asarray(got[q]), np.asarray(results[surface][q])), q
    # A path too large for device_output_limit.
    other.device_output_limit = int(0.9*5*4*n*8)
    with pytest.raises(ValueError, match="does not hold one path"):
        other.compute_thermal_radiance_linear(thickness, SURFACE_T, INTERFACES)


def test_the_calls_beside_it_return_what_they_returned(fine):
    spec, _, thickness, results = fine
    flux = dict(surface_emissivity=EMISSIVITY, remove_pedestal=False, **cloud())

    def beside():
        return (spec.compute_thermal_radiance(thickness, SURFACE_T, MU, quantities=BOTH, **flux),
                spec.compute_thermal_flux_linear(thickness, SURFACE_T, INTERFACES, **flux),
                spec.compute_radiance(thickness, boundary_temperature=SURFACE_T,
                                      remove_pedestal=False, source="linear_in_tau",
                                      interface_temperature=INTERFACES))
    before = beside()
    again = spec.compute_thermal_radiance_linear(thickness, SURFACE_T, INTERFACES, MU, EMISSIVITY,
                                                 quantities=BOTH, remove_pedestal=False, **cloud())
    after = beside()
    for q in BOTH:
        assert np.array_equal(np.asarray(again[q]), np.asarray(results["first"][q])), q
        assert np.array_equal(np.asarray(before[0][q]), np.asarray(after[0][q])), q
    for q in ("upward_flux", "downward_flux"):
        assert np.array_equal(np.asarray(before[1][q]), np.asarray(after[1][q])), q
    assert np.array_equal(np.asarray(before[2]["radiance"]), np.asarray(after[2]["radiance"]))

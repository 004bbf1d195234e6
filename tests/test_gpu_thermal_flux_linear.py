"""Spectroscopy.compute_thermal_flux_linear on the GPU, on the synthetic atmosphere of
tests/test_gpu_thermal_flux.py: fluxes and heating rates against the long-double mirror of its
definition (tests/thermal_source_cases.py) over compute_absorption("total") of the same
Spectroscopy, for both surface ends, on the grid and in bands; equal temperatures against
compute_thermal_flux; runs of whole paths; the mark on the result.

Bounds, none taken from the code under test.  Every flux is within (4*E_cpu + 1e-13)*scale of the
long-double mirror, scale = pi*max B(nu, T) over the path's interface temperatures and T_s: E_cpu =
4.73e-15 is the worst |float64 mirror - long-double mirror|/scale that
tests/test_thermal_source_host.py measures over the committed case tables (recorded as
thermal_source_cases.E_CPU = 5e-15); the factor 4 and the floor as in
tests/test_gpu_thermal_flux.py.  A band flux is held to the same multiple of the band's mean
scale.  Heating rates are paths.heating_rate of the returned fluxes, bit for bit."""
import numpy as np
import pytest

from pylbl_amd import paths, synthetic
from tests import thermal_cases as tc
from tests import thermal_source_cases as sc
from tests.test_gpu_flux import band_fluxes, spectroscopy, thickness_for, total_of
from tests.test_gpu_thermal_flux import EMISSIVITY, SHAPE, SURFACE_T, cloud

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
FLUX_BOUND = LD(4.*sc.E_CPU + sc.FLUX_FLOOR)
FLUXES = ("upward_flux", "downward_flux")
ALL = paths.THERMAL_FLUX_QUANTITIES
NAMES = dict(zip(FLUXES, tc.QUANTITIES))


def interfaces_of(spec):
    """Interface temperatures [3, 8]: the mean of the neighbouring levels inside, 6 K beyond the
    outer levels, and path 1 with an inversion of 25 K at interface 3."""
    t = np.asarray(spec.atmosphere.temperature, dtype=F64)
    inner = (t[:, :-1] + t[:, 1:])/2.
    out = np.concatenate([t[:, :1] + 6., inner, t[:, -1:] - 6.], axis=1)
    out[1, 3] += 25.
    return out


@pytest.fixture(scope="module")
def fine():
    """(spec, beta [3, 7, N], thickness, interfaces, the grid results of every quantity per
    surface, their long-double mirrors): the references every test shares."""
    spec = spectroscopy(SHAPE)
    beta = total_of(spec)
    thickness = thickness_for(beta)
    interfaces = interfaces_of(spec)
    results, mirrors = {}, {}
    for surface in ("first", "last"):
        results[surface] = spec.compute_thermal_flux_linear(
            thickness, SURFACE_T, interfaces, EMISSIVITY, surface=surface, quantities=ALL,
            remove_pedestal=False, **cloud())
        mirrors[surface] = mirror_of(spec, beta, thickness, interfaces, surface)
    return spec, beta, thickness, interfaces, results, mirrors


def mirror_of(spec, beta, thickness, interfaces, surface):
    """({quantity: [3, 8, N]} on the result's interface dim, scale [3, 1, N]) in long double."""
    scatterers = cloud()
    request = spec._thermal_flux_linear_request(
        thickness, SURFACE_T, interfaces, EMISSIVITY, None, surface, 1.66,
        scatterers["scatterer_optical_depth"], scatterers["scatterer_single_scattering_albedo"],
        scatterers["scatterer_asymmetry"], FLUXES, None, "reference")
    levels = beta.shape[1]
    inputs = sc.Inputs("call", spec.grid, beta.reshape(3*levels, -1), request.level_table,
                       interfaces, request.surface_temperature, request.surface_emissivity,
                       request.diffusivity)
    assert np.array_equal(inputs.edges, request.edge_temperature)
    first = surface == "first"
    got = sc.mirror(LD, inputs, first)
    out = {}
    for q, name in NAMES.items():
        below = got[name].reshape(3, levels, -1)
        top = got["top_" + name][:, None, :]
        out[q] = np.concatenate([below, top] if first else [top, below], axis=1)
    return out, got["scale"][:, None, :]


@pytest.mark.parametrize("surface", ["first", "last"])
def test_fluxes_and_heating_rates_match_the_mirror(fine, surface):
    spec, beta, thickness, interfaces, results, mirrors = fine
    out = results[surface]
    mark = out.attrs["source"] if hasattr(out, "attrs") else out["source"]
    assert mark == "linear_in_tau"
    reference, scale = mirrors[surface]
    assert np.all(scale > 0.)
    for q in FLUXES:
        got = np.asarray(out[q])
        assert got.shape == (3, 8, spec.grid.size) and np.all(np.isfinite(got)), q
        error = np.abs(got.astype(LD) - reference[q])
        print("%s, %s: worst error / bound %.3g" % (
            surface, q, float(np.max(error/(FLUX_BOUND*scale)))))
        assert np.all(error <= FLUX_BOUND*scale), q
    up, down = np.asarray(out["upward_flux"]), np.asarray(out["downward_flux"])
    space = 7 if surface == "first" else 0
    assert np.all(down[:, space] == 0.) and np.all(up[:, space] > 0.)
    expect = paths.heating_rate(up, down, spec.atmosphere.pressure, spec.atmosphere.temperature,
                                thickness, surface)
    assert np.array_equal(np.asarray(out["heating_rate"]), expect)
    # The linear source is not the isothermal one: the fluxes differ where a layer has a gradient.
    plain = spec.compute_thermal_flux(thickness, SURFACE_T, EMISSIVITY, surface=surface,
                                      quantities=FLUXES, remove_pedestal=False, **cloud())
    assert not hasattr(plain, "attrs") or "source" not in plain.attrs
    assert np.max(np.abs(np.asarray(plain["upward_flux"]) - up)/scale) > 1e-6


@pytest.mark.parametrize("surface", ["first", "last"])
def test_band_results_match_the_mirror(fine, surface):
    spec, beta, thickness, interfaces, _, mirrors = fine
    edges = np.concatenate([[550., 600.5, 600.5005], np.arange(601.3, 700.1, 1.), [720.]])
    out = spec.compute_thermal_flux_linear(
        thickness, SURFACE_T, interfaces, EMISSIVITY, surface=surface, quantities=ALL,
        band_edges=edges, remove_pedestal=False, **cloud())
    starts = np.searchsorted(spec.grid, edges, side="left")
    _, _, n_per_v = synthetic.grid_arguments(spec.grid)
    reference, scale = mirrors[surface]
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


def test_equal_temperatures_give_compute_thermal_flux_bit_for_bit():
    """Every level and interface of a path at one temperature: dB = 0 everywhere."""
    spec = spectroscopy(SHAPE, temperature=260.)
    thickness = thickness_for(total_of(spec))
    interfaces = np.full((SHAPE[0], SHAPE[1] + 1), 260.)
    common = dict(surface_emissivity=EMISSIVITY, quantities=ALL, remove_pedestal=False)
    common.update(cloud())
    linear = spec.compute_thermal_flux_linear(thickness, SURFACE_T, interfaces, **common)
    plain = spec.compute_thermal_flux(thickness, SURFACE_T, **common)
    for q in ALL:
        assert np.array_equal(np.asarray(linear[q]), np.asarray(plain[q])), q


def test_runs_of_whole_paths_give_the_same_bits_and_one_path_must_fit(fine):
    spec, beta, thickness, interfaces, results, _ = fine
    n = spec.grid.size
    common = dict(surface_emissivity=EMISSIVITY, remove_pedestal=False)
    common.update(cloud())
    other = spectroscopy(SHAPE)
    # beta, two work rows and two flux rows per level, seven levels a path: two paths fit, three
    # do not -- two runs; then one path per run (tests/test_thermal_source_host.py counts the runs
    # of such limits on the stand-in engine).
    for limit, surface in ((2.5, "first"), (2.5, "last"), (1.5, "first")):
        other.device_output_limit = int(limit*5*7*n*8)
        got = other.compute_thermal_flux_linear(thickness, SURFACE_T, interfaces, surface=surface,
                                                quantities=ALL, **common)
        for q in ALL:
            assert np.array_equal(np.asarray(got[q]), np.asarray(results[surface][q])), q
    other.device_output_limit = int(0.9*3*7*n*8)
    with pytest.raises(ValueError, match="does not hold one path"):
        other.compute_thermal_flux_linear(thickness, SURFACE_T, interfaces,
                                          quantities=("upward_flux",))

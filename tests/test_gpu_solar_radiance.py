"""Spectroscopy.compute_solar_radiance on the GPU, on the synthetic database of the other product
tests (2400 grid points, 3 paths of 4 levels): against the long-double mirror of its definition
(tests/solar_radiance_cases.py) fed compute_absorption("total") and compute_solar_flux's fluxes of
the same Spectroscopy, against compute_solar's "reflected_radiance" where nothing scatters, with a
spectral albedo, a user's solar table and a Rayleigh row of the caller's cross-sections, with an
instrument against Instrument.response applied in numpy, in bands, cut into runs of whole paths,
and beside the calls it shares kernels and blocks with.

Bounds, none taken from the code under test.  Every radiance is within (4*E_cpu + 1e-13)*scale of
the long-double mirror, scale = max(F0/pi, the mirror's largest |I| at the path's interfaces):
E_cpu = 7.9e-12 is the worst |float64 mirror - long-double mirror|/scale that
tests/test_solar_radiance_host.py measures over the committed case tables (recorded as
solar_radiance_cases.E_CPU = 8e-12); the factor 4 because the device's exp and expm1 are a few ulp
where numpy's are about one; the floor for benign columns.  Without scattering the call and
compute_solar each form (A*F0/pi)*exp(-sum tau/mu0)*exp(-sum tau/mu) in their own order: each is
within 4*8 roundings per level of A*F0/pi of it (8: measured on the CPU as 2.68, reasoned in
solar_radiance_cases; 4 as above).  Channel radiances are held to tests/test_gpu_instrument.py's
bound, 1e-12*sum|w v|/|sum w|; band means to 1e-12*magnitude of the long-double means of the fine
result."""
import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, paths, synthetic
from pylbl_amd.instrument import Instrument
from tests import solar_radiance_cases as sc
from tests import sweep_cases as cases
from tests import test_gpu_flux as flux_tests
from tests import two_stream_cases as ts
from tests.test_gpu_flux import thickness_for, total_of
from tests.test_gpu_instrument import check as check_channels

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
SHAPE = (3, 4)
GRID = np.arange(600., 624., 0.01)
MU0 = np.array([1., 0.35, 0.08])
MU = np.array([1., 0.6, 0.05])
PHI = np.array([0., 90., 180.])
ALBEDO = np.array([1., 0.3, 0.])
BOUND = LD(4.*sc.E_CPU + sc.FLOOR)
FLUXES = (("upward_flux", "up"), ("direct_irradiance", "direct"),
          ("diffuse_downward_flux", "diffuse"))


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
    omega_c = np.full(SHAPE, 0.96)
    omega_c[1] = 1.
    g_c = np.full(SHAPE, 0.85)
    g_c[2] = 0.3
    return dict(scatterer_optical_depth=tau_c, scatterer_single_scattering_albedo=omega_c,
                scatterer_asymmetry=g_c)


@pytest.fixture(scope="module")
def fine():
    """(spec, beta [3, 4, N], thickness, sigma on the grid, S on the grid, the grid results per
    surface): what every test shares."""
    spec = spectroscopy()
    beta = total_of(spec)
    assert np.all(beta >= 0.) and spec.grid.size == 2400
    thickness = thickness_for(beta)
    column = spec.atmosphere.pressure/(paths.K_B*spec.atmosphere.temperature)*thickness
    sigma = np.random.default_rng(9).uniform(0., 0.3, size=spec.grid.size)/column.max()
    sigma[::11] = 0.
    # S: the direct beam at space under mu0 = 1.
    solar = np.asarray(spec.compute_solar_flux(
        thickness, 1., rayleigh=False, quantities="direct_irradiance",
        remove_pedestal=False)["direct_irradiance"])[0, -1]
    results = {surface: spec.compute_solar_radiance(
        thickness, MU0, MU, PHI, surface=surface, surface_albedo=ALBEDO,
        rayleigh_cross_section=sigma, remove_pedestal=False, **cloud())
        for surface in ("first", "last")}
    return spec, beta, thickness, sigma, solar, results


def mirror_of(spec, beta, thickness, sigma, solar, surface, albedo=ALBEDO, knots=None,
              rayleigh=True, scatterers=None, **sun):
    """(the long-double mirror of a call fed the fluxes compute_solar_flux returns for it, its
    scale)."""
    scatterers = cloud() if scatterers is None else scatterers
    fluxes = spec.compute_solar_flux(
        thickness, MU0, surface=surface, surface_albedo=albedo, albedo_wavenumber=knots,
        rayleigh=rayleigh, rayleigh_cross_section=sigma if rayleigh else None,
        quantities=[q for q, _ in FLUXES], remove_pedestal=False, **scatterers, **sun)
    request = spec._solar_flux_request(
        thickness, MU0, sun.get("solar_irradiance"), sun.get("solar_wavenumber"), 1., surface,
        albedo, knots, rayleigh, sigma if rayleigh else None,
        scatterers.get("scatterer_optical_depth"),
        scatterers.get("scatterer_single_scattering_albedo"),
        scatterers.get("scatterer_asymmetry"), ("upward_flux",), None, "reference")
    rows_albedo = request.albedo if knots is None else paths.interpolate_emissivity(
        request.albedo_knots, request.albedo, spec.grid)
    levels = SHAPE[1]
    on_grid = sigma if rayleigh else np.zeros(spec.grid.size)
    inputs = ts.Inputs("call", beta.reshape(3*levels, -1), request.level_table, MU0, solar,
                       on_grid, rows_albedo)
    first = surface == "first"
    space = levels if first else 0
    assert np.array_equal(np.asarray(fluxes["direct_irradiance"])[:, space], inputs.f0())
    # The rows at the interface below each level: interface l with the surface behind level 0,
    # interface l + 1 with it behind the last level.
    below = slice(0, levels) if first else slice(1, levels + 1)
    rows = {name: np.ascontiguousarray(np.asarray(fluxes[q])[:, below].reshape(3*levels, -1))
            for q, name in FLUXES}
    high = sc.mirror(LD, inputs, MU, sc.scattering_cosine(MU, MU0, PHI), first, rows)
    return high, sc.scale(inputs, high)


def close(what, got, expect):
    high, scale = expect
    value = np.asarray(got["radiance"])
    assert value.shape == high["radiance"].shape and np.all(np.isfinite(value)), what
    error = np.abs(value.astype(LD) - high["radiance"])
    allowed = BOUND*scale
    print("%s: worst error / bound %.3g" % (what, float(np.max(error/allowed))))
    assert np.all(allowed > 0.) and np.all(error <= allowed), what
    assert np.all(value >= 0.)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_the_radiance_matches_the_mirror(fine, surface):
    spec, beta, thickness, sigma, solar, results = fine
    out = results[surface]
    assert set(out) == {"radiance", "wavenumber"}
    assert np.asarray(out["radiance"]).shape == (3, spec.grid.size)
    close(surface, out, mirror_of(spec, beta, thickness, sigma, solar, surface))
    # Over a black surface what is seen was scattered: path 2.
    assert np.all(np.asarray(out["radiance"])[2] > 0.)


def test_the_default_fit_a_spectral_albedo_and_a_solar_table_match_the_mirror(fine):
    spec, beta, thickness, _, _, _ = fine
    knots, values = np.array([600.5, 611., 623.]), np.array([0., 0.5, 1.])
    sun = dict(solar_irradiance=np.array([0.8, 0.2, 0.5, 0.9]),
               solar_wavenumber=np.array([599., 607., 615., 640.]))
    out = spec.compute_solar_radiance(thickness, MU0, MU, PHI, surface_albedo=values,
                                      albedo_wavenumber=knots, remove_pedestal=False, **cloud(),
                                      **sun)
    solar = np.asarray(spec.compute_solar_flux(
        thickness, 1., rayleigh=False, quantities="direct_irradiance", remove_pedestal=False,
        **sun)["direct_irradiance"])[0, -1]
    sigma = paths.rayleigh_cross_section(spec.grid)
    # The fit's sigma on the device is within rounding of numpy's: the fluxes fed to the mirror
    # are the device's, and tau_R enters the level with c_l*sigma of 1e-9 at these wavenumbers.
    close("fit, spectral albedo, solar table", out,
          mirror_of(spec, beta, thickness, sigma, solar, "first", albedo=values, knots=knots,
                    **sun))


@pytest.mark.parametrize("surface", ["first", "last"])
def test_without_scattering_it_is_compute_solars_reflected_radiance(fine, surface):
    spec, _, thickness, _, _, results = fine
    out = np.asarray(spec.compute_solar_radiance(
        thickness, MU0, MU, PHI, surface=surface, surface_albedo=ALBEDO, rayleigh=False,
        remove_pedestal=False)["radiance"])
    plain = spec.compute_solar(
        thickness, MU0, surface=surface, surface_albedo=ALBEDO,
        view_path_length=thickness/MU[:, None],
        quantities=("direct_irradiance", "reflected_radiance"), remove_pedestal=False)
    space = SHAPE[1] if surface == "first" else 0
    f0 = np.asarray(plain["direct_irradiance"])[:, space]
    size = ALBEDO[:, None].astype(LD)*f0.astype(LD)/LD(cases.FLUX_PI)
    allowed = 2.*(4.*sc.NO_SCATTERING_ROUNDINGS*SHAPE[1]*2.**-53)*size
    error = np.abs(out.astype(LD) - np.asarray(plain["reflected_radiance"]))
    lit = size > 0.
    print("no scattering, %s: worst error / bound %.3g" % (
        surface, float(np.max(error[lit]/allowed[lit]))))
    assert np.all(error <= allowed) and np.all(out[2] == 0.) and np.all(out[:2] > 0.)
    # Scattering changes it.
    assert not np.array_equal(out, np.asarray(results[surface]["radiance"]))


def test_an_instrument_reduces_the_fine_result(fine):
    spec, _, thickness, sigma, _, results = fine
    centers = np.arange(600.6, 623.4, 1.25)
    for instrument in (Instrument.gaussian(centers, 0.5, half_width=0.55),
                       Instrument.boxcar(centers, 0.7)):
        got = spec.compute_solar_radiance(thickness, MU0, MU, PHI, surface_albedo=ALBEDO,
                                          rayleigh_cross_section=sigma, instrument=instrument,
                                          remove_pedestal=False, **cloud())
        assert np.asarray(got["radiance"]).shape == (3, len(centers))
        check_channels(got["radiance"], instrument, spec.grid, results["first"]["radiance"])
        assert np.all(np.isfinite(np.asarray(got["radiance"])))
        assert np.array_equal(np.asarray(got["channel_center"]), centers)


def test_band_means_of_the_fine_result(fine):
    spec, _, thickness, sigma, _, results = fine
    edges = np.array([599., 600.503, 601.3, 612.3, 624.5, 625.])
    got = spec.compute_solar_radiance(thickness, MU0, MU, PHI, surface_albedo=ALBEDO,
                                      rayleigh_cross_section=sigma, band_edges=edges,
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
    spec, _, thickness, sigma, _, results = fine
    n = spec.grid.size
    common = dict(surface_albedo=ALBEDO, rayleigh_cross_section=sigma, remove_pedestal=False)
    common.update(cloud())
    other = spectroscopy()
    # Six blocks per level, four levels a path: two paths fit, then one.
    for paths_per_run in (2.5, 1.5):
        other.device_output_limit = int(paths_per_run*6*4*n*8)
        for surface in ("first", "last"):
            got = other.compute_solar_radiance(thickness, MU0, MU, PHI, surface=surface, **common)
            assert np.array_equal(np.asarray(got["radiance"]),
                                  np.asarray(results[surface]["radiance"])), surface
    other.device_output_limit = int(0.9*6*4*n*8)
    with pytest.raises(ValueError, match="does not hold one path"):
        other.compute_solar_radiance(thickness, MU0)


def test_the_calls_beside_it_return_what_they_returned(fine):
    spec, _, thickness, sigma, _, results = fine
    flux = dict(surface_albedo=ALBEDO, rayleigh_cross_section=sigma, remove_pedestal=False,
                **cloud())
    beam = dict(surface_albedo=ALBEDO, view_path_length=thickness,
                quantities=("direct_irradiance", "reflected_radiance"), remove_pedestal=False)
    before = (spec.compute_solar_flux(thickness, MU0, **flux),
              spec.compute_solar(thickness, MU0, **beam))
    again = spec.compute_solar_radiance(thickness, MU0, MU, PHI, **flux)
    after = (spec.compute_solar_flux(thickness, MU0, **flux),
             spec.compute_solar(thickness, MU0, **beam))
    assert np.array_equal(np.asarray(again["radiance"]),
                          np.asarray(results["first"]["radiance"]))
    for q in ("upward_flux", "downward_flux"):
        assert np.array_equal(np.asarray(before[0][q]), np.asarray(after[0][q])), q
    for q in beam["quantities"]:
        assert np.array_equal(np.asarray(before[1][q]), np.asarray(after[1][q])), q

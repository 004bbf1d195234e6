"""Spectroscopy.compute_solar on the GPU, on the synthetic database of the other product tests:
against the numpy mirror of its definitions over compute_absorption("total") of the same
Spectroscopy, against compute_path's transmittance, and against numpy reductions of its own grid
results for bands and instruments; runs of levels, both surfaces, the albedo table.

Bounds: 1.2e-15 relative for F0*exp(-tau) (the suite's 1e-15 for exp plus one rounding of the
product); 1e-12 relative for band fluxes and 1e-12*sum|w v|/|sum w| for channels, as
tests/test_gpu_flux.py and tests/test_gpu_instrument.py hold theirs."""
import numpy as np
import pytest

from pylbl_amd import Instrument, paths, synthetic
from tests import sweep_cases as cases
from tests.test_gpu_flux import band_fluxes, spectroscopy, thickness_for, total_of
from tests.test_gpu_instrument import check as check_channels

pytestmark = pytest.mark.gpu

LD = np.longdouble
SHAPE = (3, 7)
MU0 = np.array([1., 0.35, 0.08])
EXP_BOUND = 1.2e-15
ALL = paths.SOLAR_QUANTITIES


@pytest.fixture(scope="module")
def fine():
    """(spec, beta [3, 7, N], thickness, view lengths, the grid results of every quantity per
    surface): the references every test shares."""
    spec = spectroscopy(SHAPE)
    beta = total_of(spec)
    assert np.all(beta >= 0.)
    thickness = thickness_for(beta)
    view = 1.3*thickness_for(beta, seed=1)
    results = {surface: spec.compute_solar(
        thickness, MU0, surface=surface, surface_albedo=[1., 0.3, 0.], view_path_length=view,
        quantities=ALL, remove_pedestal=False) for surface in ("first", "last")}
    return spec, beta, thickness, view, results


def mirror(spec, beta, thickness, view, surface, albedo, solar_lengths=None):
    """compute_solar's definitions in float64 numpy, in the stated order: (F0 [3, N], tau and tv
    at every interface in the Sun's order [3, 8, N], F, reflected [3, N])."""
    levels = beta.shape[-2]
    s = paths.SOLAR_SOLID_ANGLE*cases.planck(np.float64, spec.grid, paths.SOLAR_TEMPERATURE)
    f0 = MU0[:, None]*s
    a = thickness/MU0[:, None] if solar_lengths is None else solar_lengths
    tau = np.zeros((3, levels + 1, spec.grid.size))
    tv = np.zeros_like(tau)
    order = range(levels - 1, -1, -1) if surface == "first" else range(levels)
    t, v = np.zeros((3, spec.grid.size)), np.zeros((3, spec.grid.size))
    for l in order:
        t = t + a[:, l, None]*beta[:, l]
        v = v + view[:, l, None]*beta[:, l]
        at = l if surface == "first" else l + 1
        tau[:, at], tv[:, at] = t, v
    ground = 0 if surface == "first" else levels
    albedo = np.broadcast_to(np.asarray(albedo, dtype=np.float64), (3,)).reshape(3, 1) \
        if np.ndim(albedo) < 2 else np.asarray(albedo, dtype=np.float64)
    reflected = ((albedo*f0)/np.pi)*np.exp(-(tau[:, ground] + tv[:, ground]))
    return f0, tau, tv, f0[:, None]*np.exp(-tau), reflected


def relative(got, reference, bound, what):
    got, reference = np.asarray(got), np.asarray(reference, dtype=LD)
    assert got.shape == reference.shape and np.all(np.isfinite(got)), what
    error = np.abs(got.astype(LD) - reference)
    worst = float(np.max(error/np.maximum(np.abs(reference), LD(1e-300))))
    print("%s: worst relative error %.3g" % (what, worst))
    assert np.all(error <= LD(bound)*np.abs(reference) + LD(5e-324)), (what, worst)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_every_quantity_matches_the_mirror(fine, surface):
    spec, beta, thickness, view, results = fine
    out = results[surface]
    assert set(out) == set(ALL) | {"wavenumber"}
    blackbody, tau, tv, _, _ = mirror(spec, beta, thickness, view, surface, [1., 0.3, 0.])
    space, ground = (7, 0) if surface == "first" else (0, 7)
    direct = np.asarray(out["direct_irradiance"])
    assert direct.shape == (3, 8, spec.grid.size)
    # F0 = mu0*S of the Sun's blackbody within the project's Planck bound; everything below it
    # is held to the F0 the call returned.
    f0 = direct[:, space]
    relative(f0, blackbody, 1e-12, "F0")
    with np.errstate(under="ignore"):
        relative(direct, f0[:, None].astype(LD)*np.exp(-tau.astype(LD)), EXP_BOUND, "direct")
        lead = (np.array([[1.], [0.3], [0.]])*f0)/np.pi
        depth = tau[:, ground] + tv[:, ground]
        relative(out["reflected_radiance"], lead.astype(LD)*np.exp(-depth.astype(LD)), EXP_BOUND,
                 "reflected")
    assert np.array_equal(np.asarray(out["surface_irradiance"]), direct[:, ground])
    assert np.all(np.asarray(out["reflected_radiance"])[2] == 0.)
    # The heating rate is paths.heating_rate of the returned irradiance, and never negative.
    expect = paths.heating_rate(np.zeros_like(direct), direct, spec.atmosphere.pressure,
                                spec.atmosphere.temperature, thickness, surface)
    assert np.array_equal(np.asarray(out["heating_rate"]), expect)
    assert np.all(expect >= 0.) and np.any(expect > 0.)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_direct_beam_is_f0_times_compute_paths_transmittance(fine, surface):
    spec, beta, thickness, view, results = fine
    lengths = thickness/MU0[:, None]
    cumulative = "from_last" if surface == "first" else "from_first"
    trans = np.asarray(spec.compute_path(lengths, quantities="transmittance",
                                         cumulative=cumulative,
                                         remove_pedestal=False)["transmittance"])
    direct = np.asarray(results[surface]["direct_irradiance"])
    f0 = direct[:, 7 if surface == "first" else 0]
    below = direct[:, :7] if surface == "first" else direct[:, 1:]
    relative(below, f0[:, None].astype(LD)*trans.astype(LD), EXP_BOUND, "F0*transmittance")
    # Given explicitly, the same slant lengths give the same bits.
    again = spec.compute_solar(thickness, MU0, solar_path_length=lengths, surface=surface,
                               remove_pedestal=False)
    assert np.array_equal(np.asarray(again["direct_irradiance"]), direct)


def test_a_white_surface_seen_from_the_ground_returns_f_over_pi(fine):
    spec, beta, thickness, view, results = fine
    out = spec.compute_solar(thickness, MU0, surface_albedo=1., view_path_length=0.*thickness,
                             quantities=("surface_irradiance", "reflected_radiance"),
                             remove_pedestal=False)
    surface_irradiance = np.asarray(out["surface_irradiance"])
    assert np.array_equal(surface_irradiance, np.asarray(results["first"]["surface_irradiance"]))
    # (F0/pi)*exp(-tau) beside (F0*exp(-tau))/pi: one rounding each way.
    # each way the roundings are at most 2^-53 relative: three in all.
    relative(out["reflected_radiance"], surface_irradiance.astype(LD)/LD(np.pi), 3*2.**-53,
             "F/pi")


def test_a_flat_albedo_table_gives_the_scalars_bits(fine):
    spec, beta, thickness, view, results = fine
    keywords = dict(view_path_length=view, quantities="reflected_radiance", remove_pedestal=False)
    scalar = spec.compute_solar(thickness, MU0, surface_albedo=0.37, **keywords)
    table = spec.compute_solar(thickness, MU0, surface_albedo=[0.37, 0.37, 0.37],
                               albedo_wavenumber=[590., 650., 720.], **keywords)
    assert np.array_equal(np.asarray(table["reflected_radiance"]),
                          np.asarray(scalar["reflected_radiance"]))
    sloped = spec.compute_solar(thickness, MU0, surface_albedo=[0., 0.5, 1.],
                                albedo_wavenumber=[590., 650., 720.], **keywords)
    albedo = paths.interpolate_emissivity(np.array([590., 650., 720.]), np.array([0., 0.5, 1.]),
                                          spec.grid)
    _, tau, tv, _, _ = mirror(spec, beta, thickness, view, "first", 0.)
    f0 = np.asarray(results["first"]["direct_irradiance"])[:, 7]
    with np.errstate(under="ignore"):
        relative(sloped["reflected_radiance"], ((albedo*f0)/np.pi).astype(LD) *
                 np.exp(-(tau[:, 0] + tv[:, 0]).astype(LD)), EXP_BOUND, "spectral albedo")


def test_solar_tables_and_the_distance_factor(fine):
    spec, beta, thickness, view, results = fine
    base = np.asarray(results["first"]["direct_irradiance"])
    s = paths.SOLAR_SOLID_ANGLE*cases.planck(np.float64, spec.grid, paths.SOLAR_TEMPERATURE)
    on_grid = np.asarray(spec.compute_solar(thickness, MU0, solar_irradiance=s,
                                            remove_pedestal=False)["direct_irradiance"])
    assert np.array_equal(on_grid[:, 7], MU0[:, None]*s)
    relative(on_grid, base, 1.1e-12, "S on the grid")
    knots = np.linspace(590., 710., 4001)
    values = np.random.default_rng(3).uniform(0.2, 1., knots.size)
    out = spec.compute_solar(thickness, MU0, solar_irradiance=values, solar_wavenumber=knots,
                             distance_factor=1.0334, remove_pedestal=False)
    expect = 1.0334*paths.interpolate_emissivity(knots, values, spec.grid)
    assert np.array_equal(np.asarray(out["direct_irradiance"])[:, 7], MU0[:, None]*expect)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_band_edges_reduce_the_grid_results(fine, surface):
    spec, beta, thickness, view, results = fine
    edges = np.concatenate([[550., 600.5, 600.5005], np.arange(601.3, 700.1, 1.), [720.]])
    out = spec.compute_solar(thickness, MU0, surface=surface, surface_albedo=[1., 0.3, 0.],
                             view_path_length=view, quantities=ALL, band_edges=edges,
                             remove_pedestal=False)
    starts = np.searchsorted(spec.grid, edges, side="left")
    _, _, n_per_v = synthetic.grid_arguments(spec.grid)
    grid = results[surface]
    for q in ("direct_irradiance", "surface_irradiance"):
        expect = band_fluxes(np.asarray(grid[q]), starts, n_per_v)
        got = np.asarray(out[q])
        assert np.array_equal(np.isnan(got), np.isnan(expect)) and np.any(np.isnan(expect))
        ok = ~np.isnan(expect)
        assert np.all(np.abs(got[ok] - expect[ok]) <= 1e-12*np.abs(expect[ok])), q
    with np.errstate(invalid="ignore", divide="ignore"):
        means = band_fluxes(np.asarray(grid["reflected_radiance"]), starts, n_per_v) / \
            (np.diff(starts)/n_per_v)
    got = np.asarray(out["reflected_radiance"])
    ok = ~np.isnan(means)
    assert np.array_equal(np.isnan(got), ~ok)
    assert np.all(np.abs(got[ok] - means[ok]) <= 1e-12*np.abs(means[ok]))
    ground = 0 if surface == "first" else 7
    assert np.array_equal(np.asarray(out["surface_irradiance"]),
                          np.asarray(out["direct_irradiance"])[:, ground], equal_nan=True)
    direct = np.asarray(out["direct_irradiance"])
    expect = paths.heating_rate(np.zeros_like(direct), direct, spec.atmosphere.pressure,
                                spec.atmosphere.temperature, thickness, surface)
    assert np.array_equal(np.asarray(out["heating_rate"]), expect, equal_nan=True)
    assert np.array_equal(np.asarray(out["band_points"]), np.diff(starts))


def test_instrument_reduces_the_rows_per_path(fine):
    spec, beta, thickness, view, results = fine
    x = Instrument.gaussian(np.arange(603., 697., 0.5), 0.5, half_width=1.5)
    quantities = ("surface_irradiance", "reflected_radiance")
    out = spec.compute_solar(thickness, MU0, surface_albedo=[1., 0.3, 0.], view_path_length=view,
                             quantities=quantities, instrument=x, remove_pedestal=False)
    for q in quantities:
        assert np.asarray(out[q]).shape == (3, len(x))
        check_channels(out[q], x, spec.grid, results["first"][q])
    np.testing.assert_array_equal(np.asarray(out["channel_center"]), x.centers)


def test_runs_of_levels_give_the_same_bits(fine):
    spec, beta, thickness, view, results = fine
    n = spec.grid.size
    edges = np.arange(600., 700.1, 2.5)
    calls = [dict(surface_albedo=[1., 0.3, 0.], view_path_length=view, quantities=ALL),
             dict(surface="last", quantities=("direct_irradiance", "surface_irradiance")),
             dict(surface_albedo=0.5, view_path_length=view, band_edges=edges, quantities=ALL)]
    whole = [spec.compute_solar(thickness, MU0, remove_pedestal=False, **call) for call in calls]
    other = spectroscopy(SHAPE)
    for limit in (2*5*n*8, 2*n*8):          # runs of 5 levels, of one level
        other.device_output_limit = limit
        for call, expect in zip(calls, whole):
            got = other.compute_solar(thickness, MU0, remove_pedestal=False, **call)
            for q in call["quantities"]:
                assert np.array_equal(np.asarray(got[q]), np.asarray(expect[q]),
                                      equal_nan=True), (limit, q)


def test_the_flipped_atmosphere_gives_the_flipped_result(fine):
    spec, beta, thickness, view, results = fine
    full = synthetic.standard_atmosphere(int(np.prod(SHAPE)))
    from tests.test_gpu_flux import GASES, _TABLES
    from pylbl_amd import MemoryDatabase, Spectroscopy
    flip = lambda x: np.ascontiguousarray(x.reshape(SHAPE)[:, ::-1])
    atmosphere = synthetic.Atmos(p=flip(full.p), t=flip(full.t),
                                 vmr={k: flip(full.vmr[k]) for k in GASES})
    flipped = Spectroscopy(atmosphere, spec.grid, MemoryDatabase(_TABLES["small"]))
    out = flipped.compute_solar(thickness[:, ::-1], MU0, surface="last",
                                surface_albedo=[1., 0.3, 0.], view_path_length=view[:, ::-1],
                                quantities=ALL, remove_pedestal=False)
    base = results["first"]
    assert np.array_equal(np.asarray(out["direct_irradiance"]),
                          np.asarray(base["direct_irradiance"])[:, ::-1])
    assert np.array_equal(np.asarray(out["heating_rate"]),
                          np.asarray(base["heating_rate"])[:, ::-1])
    for q in ("surface_irradiance", "reflected_radiance"):
        assert np.array_equal(np.asarray(out[q]), np.asarray(base[q]))

"""Spectroscopy.compute_radiance behind a surface with a spectral emissivity that reflects, on the
small synthetic atmosphere of tests/test_gpu_radiance.py (3 gases, 3 paths of 7 levels, 10 000 grid
points): against the long-double mirror of tests/surface_cases.py fed with
compute_absorption("total"); band means, instrument channels, brightness temperature, per-level
rows and the linear-in-tau source, each with reflection; runs of levels; and against compute_flux
with one angle, which has had the reflected term since it was merged.

Bounds: 1e-12 of the magnitude a radiance is formed from (surface_cases); for band means the mean
of that magnitude; channels as tests/test_gpu_instrument.py checks them; 1e-12 relative between
compute_flux and pi times the radiance (the same non-negative terms, pi applied once)."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import linear_source_cases as linear
from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests import test_gpu_instrument as instrument_tests
from tests import test_gpu_linear_source as linear_tests
from tests import test_gpu_radiance as radiance_tests

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
SHAPE = radiance_tests.SHAPE
DOWNWELLING = surface.DOWNWELLING
BOUND = LD(1e-12)
KNOTS = np.array([590., 620., 620.005, 655., 699.99, 720.])
TABLE = np.array([[0.98, 0.95, 0.7, 0.72, 0.99, 1.],
                  [1., 1., 1., 1., 1., 1.],
                  [0., 0.3, 0.9, 0.5, 0.2, 0.6]])
BOUNDARY_T = np.array([288., 300., 265.])
DIRECTIONS = ["toward_last", "toward_first"]


def mark(out, name):
    return out.attrs.get(name) if hasattr(out, "attrs") else out.get(name)


@pytest.fixture(scope="module")
def fine():
    """radiance_tests' (3, 7) atmosphere without the pedestal, as a sweep_cases-like problem."""
    assert SHAPE[0] == cases.PATHS
    spec = radiance_tests.spectroscopy()
    beta = radiance_tests.total_of(spec)
    assert np.all(beta >= 0.)
    lengths = radiance_tests.lengths_for(beta)
    interfaces = linear_tests.interfaces_for(SHAPE)
    problem = SimpleNamespace(
        nu=spec.grid, beta=beta.reshape(-1, spec.grid.size), thickness=lengths.ravel(),
        temperature=spec.atmosphere.temperature.ravel(), levels_per_path=SHAPE[1],
        boundary_t=BOUNDARY_T, edges=linear.edge_table(interfaces))
    return spec, problem, lengths, interfaces


def mirror(problem, direction, e, reflection_lengths, linear_source=False, store={}):
    key = (direction, np.asarray(e).tobytes(), None if reflection_lengths is None
           else np.asarray(reflection_lengths).tobytes(), linear_source)
    if key not in store:
        store[key] = surface.two_pass(
            LD, problem, direction == "toward_first", e,
            None if reflection_lengths is None else np.asarray(reflection_lengths).ravel(),
            problem.edges if linear_source else None)
    return store[key]


def final(problem, direction, values):
    return values[surface.final_rows(problem.levels_per_path, direction == "toward_first")]


def close(what, got, reference, magnitude):
    got = np.asarray(got, dtype=F64).reshape(reference.shape)
    error = np.abs(got.astype(LD) - reference)
    assert np.all(np.isfinite(got)), what
    worst = float(np.max(error/(BOUND*magnitude)))
    print("worst error / bound, %s: %.3g" % (what, worst))
    assert np.all(error <= BOUND*magnitude), (what, worst)


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_spectral_reflecting_surface_meets_the_mirror(fine, direction):
    spec, problem, lengths, _ = fine
    e = surface.emissivity(LD, KNOTS, TABLE, spec.grid)
    reflection = 1.66*lengths
    expect = mirror(problem, direction, e, reflection)
    keywords = dict(boundary_temperature=BOUNDARY_T, boundary_emissivity=TABLE,
                    emissivity_wavenumber=KNOTS, reflection_path_length=reflection,
                    direction=direction, remove_pedestal=False)
    out = spec.compute_radiance(lengths, quantities=("radiance", "brightness_temperature",
                                                     DOWNWELLING), **keywords)
    assert mark(out, "surface") == "reflecting" and mark(out, "emissivity") == "spectral"
    assert mark(out, "source") is None
    rad, mag = expect["up"]
    close("radiance", out["radiance"], final(problem, direction, rad),
          final(problem, direction, mag))
    close("downwelling", out[DOWNWELLING], *expect["down"])
    assert np.asarray(out[DOWNWELLING]).shape == (3, spec.grid.size)
    bt = cases.brightness(LD, spec.grid, final(problem, direction, rad))
    bt_mag = cases.brightness_magnitude(LD, spec.grid, final(problem, direction, rad),
                                        final(problem, direction, mag))
    close("brightness temperature", out["brightness_temperature"], bt, bt_mag)
    # Per level: the rows are the up pass's.
    levels = spec.compute_radiance(lengths, cumulative=True, **keywords)
    close("per level", np.asarray(levels["radiance"]).reshape(rad.shape), rad, mag)
    # The reflected term is there: path 1 is black, the others gain what they reflect.
    plain = np.asarray(spec.compute_radiance(
        lengths, **{k: v for k, v in keywords.items() if k != "reflection_path_length"})
        ["radiance"])
    got = np.asarray(out["radiance"])
    assert np.array_equal(got[1], plain[1])
    assert np.all(got[[0, 2]] >= plain[[0, 2]]) and np.any(got[2] > plain[2]*1.001)
    # A flat table is the scalar emissivity, bit for bit; only D asked for: the down pass alone.
    flat = spec.compute_radiance(lengths, boundary_temperature=BOUNDARY_T, direction=direction,
                                 boundary_emissivity=[0.9, 0.9], emissivity_wavenumber=[1., 2.],
                                 reflection_path_length=reflection, remove_pedestal=False)
    grey = spec.compute_radiance(lengths, boundary_temperature=BOUNDARY_T, direction=direction,
                                 boundary_emissivity=0.9, reflection_path_length=reflection,
                                 remove_pedestal=False)
    assert linear_tests.same_bits(flat["radiance"], grey["radiance"])
    assert mark(grey, "emissivity") is None and mark(grey, "surface") == "reflecting"
    alone = spec.compute_radiance(lengths, quantities=DOWNWELLING, **keywords)
    assert linear_tests.same_bits(alone[DOWNWELLING], out[DOWNWELLING])
    opposite = DIRECTIONS[1 - DIRECTIONS.index(direction)]
    sky = spec.compute_radiance(reflection, direction=opposite, remove_pedestal=False)
    assert linear_tests.same_bits(sky["radiance"], out[DOWNWELLING])


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_linear_source_bands_and_channels_with_reflection(fine, direction):
    spec, problem, lengths, interfaces = fine
    e = surface.emissivity(LD, KNOTS, TABLE, spec.grid)
    keywords = dict(boundary_temperature=BOUNDARY_T, boundary_emissivity=TABLE,
                    emissivity_wavenumber=KNOTS, reflection_path_length=lengths,
                    direction=direction, remove_pedestal=False, source="linear_in_tau",
                    interface_temperature=interfaces)
    expect = mirror(problem, direction, e, lengths, linear_source=True)
    rad, mag = expect["up"]
    out = spec.compute_radiance(lengths, quantities=("radiance", DOWNWELLING), **keywords)
    assert mark(out, "source") == "linear_in_tau" and mark(out, "surface") == "reflecting"
    close("linear radiance", out["radiance"], final(problem, direction, rad),
          final(problem, direction, mag))
    close("linear downwelling", out[DOWNWELLING], *expect["down"])

    edges = np.concatenate([[550., 580.], np.arange(600., 700.1, 1.), [720.]])
    starts = np.searchsorted(spec.grid, edges, side="left")
    bands = spec.compute_radiance(lengths, band_edges=edges,
                                  quantities=("radiance", DOWNWELLING), **keywords)
    for name, (values, magnitude) in (("radiance", (final(problem, direction, rad),
                                                    final(problem, direction, mag))),
                                      (DOWNWELLING, expect["down"])):
        means = cases.band_means(LD, values, starts)
        scale = cases.band_means(LD, magnitude, starts)
        got = np.asarray(bands[name])
        assert got.shape == means.shape
        assert np.array_equal(np.isnan(got), np.isnan(means)) and np.any(np.isnan(means))
        ok = ~np.isnan(means)
        close("band " + name, got[ok], means[ok], scale[ok])
    per_level = spec.compute_radiance(lengths, band_edges=edges, cumulative=True, **keywords)
    means = cases.band_means(LD, rad, starts)
    ok = ~np.isnan(means)
    close("cumulative bands", np.asarray(per_level["radiance"]).reshape(means.shape)[ok],
          means[ok], cases.band_means(LD, mag, starts)[ok])

    x = instrument_tests.SHAPES["gaussian"](np.arange(603., 697., 0.5))
    channels = spec.compute_radiance(
        lengths, instrument=x, quantities=("radiance", "brightness_temperature", DOWNWELLING),
        **keywords)
    instrument_tests.check(channels["radiance"], x, spec.grid, np.asarray(out["radiance"]))
    instrument_tests.check(channels[DOWNWELLING], x, spec.grid, np.asarray(out[DOWNWELLING]))
    assert np.all(np.asarray(channels["brightness_temperature"]) > 0.)
    cumulative = spec.compute_radiance(lengths, instrument=x, cumulative=True, **keywords)
    fine_levels = spec.compute_radiance(lengths, cumulative=True, **keywords)
    instrument_tests.check(cumulative["radiance"], x, spec.grid,
                           np.asarray(fine_levels["radiance"]).reshape(-1, spec.grid.size))


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_runs_of_levels_recompute_the_absorption(fine, direction):
    """device_output_limit of 4 levels: 21 levels in six runs that cut paths; the up pass computes
    five of them again.  Every sweep is the whole call's, bit for bit."""
    spec, problem, lengths, _ = fine
    keywords = dict(boundary_temperature=BOUNDARY_T, boundary_emissivity=TABLE,
                    emissivity_wavenumber=KNOTS, reflection_path_length=1.66*lengths,
                    direction=direction, remove_pedestal=False,
                    quantities=("radiance", DOWNWELLING))
    whole = spec.compute_radiance(lengths, **keywords)
    cut = radiance_tests.spectroscopy()
    cut.device_output_limit = 4*spec.grid.size*8
    for more in (dict(), dict(cumulative=True, quantities=("radiance",))):
        a = spec.compute_radiance(lengths, **dict(keywords, **more))
        b = cut.compute_radiance(lengths, **dict(keywords, **more))
        for q in dict(keywords, **more)["quantities"]:
            assert linear_tests.same_bits(a[q], b[q]), (direction, more, q)
    assert linear_tests.same_bits(whole["radiance"], a["radiance"][:, -1 if direction ==
                                                                   "toward_last" else 0])


@pytest.mark.parametrize("surface_at", ["first", "last"])
@pytest.mark.parametrize("source", ["isothermal", "linear_in_tau"])
def test_one_angle_flux_is_pi_times_the_radiance(fine, surface_at, source):
    """compute_flux(angles=([1.], [1.])) sweeps one radiance along the layer thickness, reflects
    (1 - eps) of it at the surface and multiplies by pi: the top upward flux is pi times the
    reflecting radiance, the surface downward flux pi times D."""
    spec, _, lengths, interfaces = fine
    direction = "toward_last" if surface_at == "first" else "toward_first"
    more = dict(source=source)
    if source == "linear_in_tau":
        more["interface_temperature"] = interfaces
    emissivity = np.array([0.9, 1., 0.35])
    flux = spec.compute_flux(lengths, BOUNDARY_T, emissivity, surface=surface_at,
                             angles=([1.], [1.]), remove_pedestal=False, **more)
    out = spec.compute_radiance(lengths, boundary_temperature=BOUNDARY_T,
                                boundary_emissivity=emissivity, reflection_path_length=lengths,
                                direction=direction, quantities=("radiance", DOWNWELLING),
                                remove_pedestal=False, **more)
    top, bottom = (-1, 0) if surface_at == "first" else (0, -1)
    radiance_tests.assert_relative(np.asarray(flux["upward_flux"])[:, top],
                                   np.pi*np.asarray(out["radiance"]), 1e-12)
    radiance_tests.assert_relative(np.asarray(flux["downward_flux"])[:, bottom],
                                   np.pi*np.asarray(out[DOWNWELLING]), 1e-12)

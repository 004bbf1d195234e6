"""Spectroscopy.compute_radiance on the GPU against a numpy loop, in the stated order of
operations, over compute_absorption("total") of the same Spectroscopy (itself pinned to the
oracle by the rest of the suite); physical invariants; runs of levels, determinism and threads."""
import threading

import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from pylbl_amd.spectroscopy import PLANCK_C1, PLANCK_C2

pytestmark = pytest.mark.gpu

GASES = ("H2O", "CO2", "O3")
SHAPE = (3, 7)
_TABLES = {}


def atmosphere(shape, temperature=None):
    full = synthetic.standard_atmosphere(int(np.prod(shape)))
    t = full.t if temperature is None else np.full(full.t.shape, float(temperature))
    return synthetic.Atmos(p=full.p.reshape(shape), t=t.reshape(shape),
                           vmr={k: full.vmr[k].reshape(shape) for k in GASES})


def spectroscopy(shape=SHAPE, temperature=None, **keywords):
    if "small" not in _TABLES:
        _TABLES["small"] = [synthetic.line_table(name, 576., 724., num_lines=3000, seed=40 + i)
                            for i, name in enumerate(GASES)]
    return Spectroscopy(atmosphere(shape, temperature), np.arange(600., 700., 0.01),
                        MemoryDatabase(_TABLES["small"]), **keywords)


def total_of(spec, remove_pedestal=False):
    return np.asarray(spec.compute_absorption("total", remove_pedestal=remove_pedestal)
                      ["absorption"])


def lengths_for(beta, seed=0, depth=20.):
    """Path lengths [m] that keep the optical depth of a path below ~depth."""
    lengths = np.random.default_rng(seed).uniform(0.5, 1.5, size=beta.shape[:-1])
    return lengths*depth/np.max(np.sum(np.abs(beta), axis=-2))


def planck(nu, t):
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        b = (((PLANCK_C1*nu)*nu)*nu)/np.expm1((PLANCK_C2*nu)/t)
    return np.where(nu > 0., b, 0.)


def brightness(nu, radiance):
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        t = (PLANCK_C2*nu)/np.log1p((((PLANCK_C1*nu)*nu)*nu)/radiance)
    return np.where((nu > 0.) & (radiance > 0.), t, 0.)


def per_path(value, paths_shape):
    return None if value is None else np.broadcast_to(np.asarray(value, float), paths_shape)


def numpy_radiance(spec, beta, lengths, boundary_temperature=None, boundary_emissivity=1.,
                   direction="toward_last", cumulative=False, magnitude=False):
    """The sweep of compute_radiance in numpy: beta [..., L, N], lengths [..., L]; with
    `magnitude` also the same recurrence over |terms| (a scale for rounding bounds)."""
    nu = spec.grid
    temperature = spec.atmosphere.temperature
    lead = beta.shape[:-2]
    levels = beta.shape[-2]
    tb = per_path(boundary_temperature, lead)
    eb = per_path(boundary_emissivity, lead)
    if tb is None:
        rad = np.zeros(lead + nu.shape)
    else:
        rad = eb[..., None]*planck(nu, tb[..., None])
    mag = np.abs(rad)
    out = np.zeros(beta.shape) if cumulative else None
    mags = np.zeros(beta.shape) if cumulative else None
    order = range(levels - 1, -1, -1) if direction == "toward_first" else range(levels)
    for l in order:
        x = lengths[..., l, None]*beta[..., l, :]
        t = np.exp(-x)
        a = -np.expm1(-x)
        b = planck(nu, temperature[..., l, None])
        rad = rad*t + b*a
        mag = mag*np.abs(t) + np.abs(b*a)
        if cumulative:
            out[..., l, :] = rad
            mags[..., l, :] = mag
    result = out if cumulative else rad
    if magnitude:
        return result, (mags if cumulative else mag)
    return result


def numpy_band_means(values, starts):
    means = np.full(values.shape[:-1] + (starts.size - 1,), np.nan)
    for b in range(starts.size - 1):
        if starts[b + 1] > starts[b]:
            means[..., b] = values[..., starts[b]:starts[b + 1]].mean(axis=-1)
    return means


def assert_relative(got, expect, bound):
    got, expect = np.asarray(got), np.asarray(expect)
    assert got.shape == expect.shape
    assert np.array_equal(np.isnan(got), np.isnan(expect))
    ok = ~np.isnan(expect)
    error = np.abs(got[ok] - expect[ok])/np.maximum(np.abs(expect[ok]), 1.e-300)
    assert error.size == 0 or error.max() <= bound, error.max()


BOUNDARIES = {
    "none": dict(),
    "scalar": dict(boundary_temperature=288.),
    "scalar grey": dict(boundary_temperature=295., boundary_emissivity=0.93),
    "per path": dict(boundary_temperature=np.array([270., 288., 305.]),
                     boundary_emissivity=np.array([1., 0.8, 0.])),
}


@pytest.fixture(scope="module")
def fine():
    """A (3, 7) atmosphere without the pedestal: beta >= 0, no cancellation in the sweep."""
    spec = spectroscopy()
    beta = total_of(spec)
    assert np.all(beta >= 0.)
    return spec, beta, lengths_for(beta)


@pytest.mark.parametrize("direction", ["toward_last", "toward_first"])
@pytest.mark.parametrize("boundary", list(BOUNDARIES))
def test_radiance_and_brightness_temperature_match_numpy(fine, direction, boundary):
    spec, beta, lengths = fine
    keywords = BOUNDARIES[boundary]
    out = spec.compute_radiance(lengths, direction=direction,
                                quantities=("radiance", "brightness_temperature"),
                                remove_pedestal=False, **keywords)
    expect = numpy_radiance(spec, beta, lengths, direction=direction, **keywords)
    assert set(out) == {"wavenumber", "radiance", "brightness_temperature"}
    assert np.array_equal(out["wavenumber"], spec.grid)
    assert np.all(expect > 0.)
    assert_relative(out["radiance"], expect, 1.e-12)
    assert_relative(out["brightness_temperature"], brightness(spec.grid, expect), 1.e-12)
    assert np.all(out["brightness_temperature"] > 0.)


@pytest.mark.parametrize("direction", ["toward_last", "toward_first"])
def test_cumulative(fine, direction):
    spec, beta, lengths = fine
    keywords = BOUNDARIES["per path"]
    out = spec.compute_radiance(lengths, direction=direction, cumulative=True,
                                quantities=("radiance", "brightness_temperature"),
                                remove_pedestal=False, **keywords)
    expect = numpy_radiance(spec, beta, lengths, direction=direction, cumulative=True, **keywords)
    assert out["radiance"].shape == SHAPE + (spec.grid.size,)
    assert_relative(out["radiance"], expect, 1.e-12)
    assert_relative(out["brightness_temperature"], brightness(spec.grid, expect), 1.e-12)
    final = spec.compute_radiance(lengths, direction=direction, remove_pedestal=False, **keywords)
    last = -1 if direction == "toward_last" else 0
    assert np.array_equal(out["radiance"][:, last], final["radiance"])


@pytest.mark.parametrize("direction", ["toward_last", "toward_first"])
@pytest.mark.parametrize("cumulative", [False, True])
def test_band_means(fine, direction, cumulative):
    spec, beta, lengths = fine
    grid = spec.grid
    keywords = BOUNDARIES["scalar grey"]
    expect = numpy_radiance(spec, beta, lengths, direction=direction, cumulative=cumulative,
                            **keywords)
    edge_sets = {
        "1 cm-1": np.arange(600., 700.1, 1.),
        "outside and empty": [550., 580., 600.5, 600.5005, 601.3, 690., 720.],
        "straddling segments": np.concatenate([[599.], grid[[7, 4095, 4096, 4097]] - 0.001,
                                               [650.02, 681.]]),
    }
    for label, edges in edge_sets.items():
        out = spec.compute_radiance(lengths, direction=direction, cumulative=cumulative,
                                    band_edges=edges, remove_pedestal=False, **keywords)
        starts = np.searchsorted(grid, edges, side="left")
        assert set(out) == {"band_lower", "band_upper", "band_points", "radiance"}, label
        assert np.array_equal(out["band_points"], np.diff(starts)), label
        assert_relative(out["radiance"], numpy_band_means(expect, starts), 1.e-12)


def test_pedestal_order_of_operations():
    """With the pedestal removed beta goes negative at some points (t > 1, a < 0) and the update
    can cancel: the error is bounded by the magnitudes of the terms, not by the result."""
    spec = spectroscopy()
    beta = total_of(spec, remove_pedestal=True)
    assert np.any(beta < 0.)
    lengths = lengths_for(beta, seed=3)
    for direction in ("toward_last", "toward_first"):
        keywords = BOUNDARIES["per path"]
        out = spec.compute_radiance(lengths, direction=direction, cumulative=True,
                                    remove_pedestal=True, **keywords)
        expect, scale = numpy_radiance(spec, beta, lengths, direction=direction,
                                       cumulative=True, magnitude=True, **keywords)
        error = np.abs(out["radiance"] - expect)/np.maximum(scale, 1.e-300)
        assert error.max() <= 1.e-12, error.max()


def test_zero_lengths_leave_the_boundary_term():
    spec = spectroscopy()
    zero = np.zeros(SHAPE)
    keywords = BOUNDARIES["per path"]
    out = spec.compute_radiance(zero, quantities=("radiance", "brightness_temperature"),
                                **keywords)
    expect = keywords["boundary_emissivity"][:, None]*planck(
        spec.grid, keywords["boundary_temperature"][:, None])
    assert_relative(out["radiance"][:2], expect[:2], 1.e-14)
    assert np.all(out["radiance"][2] == 0.)                 # emissivity 0
    assert np.all(out["brightness_temperature"][2] == 0.)
    assert_relative(out["brightness_temperature"][0], np.full(spec.grid.size, 270.), 1.e-12)
    none = spec.compute_radiance(zero, direction="toward_first", cumulative=True)
    assert np.all(none["radiance"] == 0.)


def test_isothermal_atmosphere_with_a_black_boundary_is_planck():
    spec = spectroscopy(temperature=250.)
    beta = total_of(spec)
    lengths = lengths_for(beta, seed=4)
    for direction in ("toward_last", "toward_first"):
        out = spec.compute_radiance(lengths, boundary_temperature=250., direction=direction,
                                    quantities=("radiance", "brightness_temperature"),
                                    remove_pedestal=False)
        assert_relative(out["radiance"], np.broadcast_to(planck(spec.grid, 250.),
                                                         out["radiance"].shape), 1.e-14)
        assert_relative(out["brightness_temperature"],
                        np.full(out["brightness_temperature"].shape, 250.), 1.e-12)


def test_very_long_paths_see_only_the_last_level(fine):
    spec, beta, lengths = fine
    # (beta of the top levels is small: lengths this long make nearly every layer opaque)
    long = lengths*1.e200
    temperature = spec.atmosphere.temperature
    for direction, last in (("toward_last", -1), ("toward_first", 0)):
        out = spec.compute_radiance(long, boundary_temperature=300., direction=direction,
                                    remove_pedestal=False)
        x = long[:, last, None]*beta[:, last, :]
        opaque = x > 50.
        assert opaque.mean() > 0.9
        expect = planck(spec.grid, temperature[:, last, None])
        assert_relative(out["radiance"][opaque], np.broadcast_to(expect, opaque.shape)[opaque],
                        1.e-14)


def test_isothermal_emission_is_planck_times_absorptance():
    """No boundary, one temperature: I = B(T) (1 - exp(-tau)), with exp(-tau) from compute_path."""
    spec = spectroscopy(temperature=240.)
    beta = total_of(spec)
    lengths = lengths_for(beta, seed=6)
    for direction in ("toward_last", "toward_first"):
        out = spec.compute_radiance(lengths, direction=direction, remove_pedestal=False)
        trans = spec.compute_path(lengths, quantities="transmittance",
                                  remove_pedestal=False)["transmittance"]
        where = trans <= 0.5
        assert where.mean() > 0.05
        expect = np.broadcast_to(planck(spec.grid, 240.), trans.shape)*(1. - trans)
        assert_relative(out["radiance"][where], expect[where], 1.e-12)


@pytest.mark.parametrize("direction", ["toward_last", "toward_first"])
@pytest.mark.parametrize("cumulative", [False, True])
def test_runs_of_levels_give_the_same_bits(direction, cumulative):
    spec = spectroscopy()
    lengths = lengths_for(total_of(spec, True), seed=7)
    edges = np.arange(600., 700.1, 0.37)
    keywords = dict(direction=direction, cumulative=cumulative, **BOUNDARIES["per path"])
    quantities = ("radiance", "brightness_temperature")
    whole = spec.compute_radiance(lengths, quantities=quantities, **keywords)
    whole_bands = spec.compute_radiance(lengths, band_edges=edges, **keywords)
    v0, vn, n_per_v = synthetic.grid_arguments(spec.grid)
    level_bytes = (vn - v0)*n_per_v*8
    for limit in (0, 2*level_bytes, 5*level_bytes):
        spec.device_output_limit = limit
        chunked = spec.compute_radiance(lengths, quantities=quantities, **keywords)
        chunked_bands = spec.compute_radiance(lengths, band_edges=edges, **keywords)
        for q in quantities:
            assert np.array_equal(chunked[q], whole[q]), (limit, q)
        assert np.array_equal(chunked_bands["radiance"], whole_bands["radiance"],
                              equal_nan=True), limit


def test_repeated_calls_and_threads_give_the_same_bits():
    spec = spectroscopy()
    lengths = lengths_for(total_of(spec, True), seed=9)
    edges = np.arange(600., 700.1, 1.)
    calls = [dict(boundary_temperature=290.), dict(band_edges=edges),
             dict(direction="toward_first", cumulative=True, band_edges=edges),
             dict(cumulative=True, quantities="brightness_temperature")]
    first = [spec.compute_radiance(lengths, **c) for c in calls]
    again = [spec.compute_radiance(lengths, **c) for c in calls]
    for a, b in zip(again, first):
        for q in ("radiance", "brightness_temperature"):
            if q in b:
                assert np.array_equal(a[q], b[q], equal_nan=True)
    got = {}

    def worker(index):
        got[index] = [spec.compute_radiance(lengths, **c) for c in calls]
    threads = [threading.Thread(target=worker, args=(i,)) for i in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for index in range(3):
        for result, expect in zip(got[index], first):
            for q in ("radiance", "brightness_temperature"):
                if q in expect:
                    assert np.array_equal(result[q], expect[q], equal_nan=True)

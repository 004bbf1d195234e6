"""Spectroscopy.compute_jacobian on the GPU against the float64 numpy mirror of
tests/jacobian_cases.py over compute_absorption("total") of the same Spectroscopy; the radiance
against compute_radiance bit for bit; finite differences through the public interface; physical
invariants; band and channel means; runs of whole paths and determinism.

Bounds: the project's 1e-12 applied to the magnitude each result is formed from (the mirror's
magnitudes: (|B_k| + |I_k|)*trail_k for dI/dx, times x_k for the log form, the value itself for
the temperature and boundary Jacobians)."""
import numpy as np
import pytest

from pylbl_amd.instrument import Instrument
from pylbl_amd.spectroscopy import band_columns
from tests import jacobian_cases as jac
from tests.test_gpu_radiance import BOUNDARIES, SHAPE, lengths_for, spectroscopy, total_of

pytestmark = pytest.mark.gpu

BOUND = 1e-12
EVERYTHING = jac.OUTPUTS
PER_LEVEL_ONLY = ("radiance",) + jac.PER_LEVEL


def bits(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float64).view(np.uint64)


def mirror(spec, beta, lengths, direction="toward_last", boundary_temperature=None,
           boundary_emissivity=1., kind=np.float64):
    """jacobian_cases.jacobian for the Spectroscopy's atmosphere: flat rows."""
    shape = spec.atmosphere.temperature.shape
    paths = int(np.prod(shape[:-1]))
    per_path = lambda v: None if v is None else \
        np.broadcast_to(np.asarray(v, dtype=np.float64), shape[:-1]).ravel()
    return jac.jacobian(kind, spec.grid, np.asarray(beta).reshape(-1, spec.grid.size),
                        np.asarray(lengths).ravel(), spec.atmosphere.temperature.ravel(), shape[-1],
                        direction == "toward_first", per_path(boundary_temperature),
                        per_path(boundary_emissivity) if boundary_temperature is not None
                        else np.ones(paths))


def assert_close(got, values, magnitudes, quantities, what=""):
    for q in quantities:
        g = np.asarray(got[q]).reshape(values[q].shape)
        assert np.all(np.isfinite(g)), (what, q)
        error, allowed = np.abs(g - values[q]), BOUND*magnitudes[q]
        worst = float(np.max(error/np.where(allowed > 0., allowed, 1.)))
        assert np.all(error <= allowed), (what, q, worst)


@pytest.fixture(scope="module")
def fine():
    spec = spectroscopy()
    beta = total_of(spec)
    assert np.all(beta >= 0.)
    return spec, beta, lengths_for(beta)


@pytest.mark.parametrize("direction", ["toward_last", "toward_first"])
@pytest.mark.parametrize("boundary", list(BOUNDARIES))
def test_every_quantity_matches_the_mirror(fine, direction, boundary):
    spec, beta, lengths = fine
    keywords = BOUNDARIES[boundary]
    quantities = EVERYTHING if keywords else PER_LEVEL_ONLY
    out = spec.compute_jacobian(lengths, direction=direction, quantities=quantities,
                                remove_pedestal=False, **keywords)
    assert set(out) == set(quantities) | {"wavenumber"}
    assert np.array_equal(out["wavenumber"], spec.grid)
    for q in quantities:
        lead = SHAPE if q in jac.PER_LEVEL else SHAPE[:-1]
        assert np.asarray(out[q]).shape == lead + (spec.grid.size,), q
    values, magnitudes = mirror(spec, beta, lengths, direction, **keywords)
    assert_close(out, values, magnitudes, quantities, (direction, boundary))
    radiance = spec.compute_radiance(lengths, direction=direction, remove_pedestal=False,
                                     **keywords)["radiance"]
    assert np.array_equal(bits(out["radiance"]), bits(radiance))


def test_default_quantities_and_single_selection(fine):
    spec, beta, lengths = fine
    out = spec.compute_jacobian(lengths, boundary_temperature=288., remove_pedestal=False)
    assert set(out) == {"wavenumber", "radiance", "optical_depth_jacobian",
                        "temperature_jacobian"}
    everything = spec.compute_jacobian(lengths, boundary_temperature=288., quantities=EVERYTHING,
                                       remove_pedestal=False)
    for q in ("radiance", "optical_depth_jacobian", "temperature_jacobian"):
        assert np.array_equal(bits(out[q]), bits(everything[q])), q
    for q in EVERYTHING:
        one = spec.compute_jacobian(lengths, boundary_temperature=288., quantities=q,
                                    remove_pedestal=False)
        assert set(one) == {"wavenumber", q}
        assert np.array_equal(bits(one[q]), bits(everything[q])), q


def test_finite_differences_through_the_public_interface(fine):
    """Scaling one level's path_length by 1 +- d against log_optical_depth_jacobian,
    boundary_temperature +- h against boundary_temperature_jacobian, two emissivities against
    boundary_emissivity_jacobian (exactly linear).  d = 1e-5 and h = 1e-2 K: truncation (d^2/6 and
    h^2/6 times the third derivative, ~1e-10 and ~1e-9 of the scale) and float64 rounding
    (1e-16/d, 1e-16/h of I: 1e-11, 1e-14 K-1) both stay far below the Jacobians.  The residues of
    the GPU are bounded by 10 times those of the float64 mirror for the same differences."""
    spec, beta, lengths = fine
    d, h, level = 1e-5, 1e-2, 3
    tb, eb = 288., 0.9
    keywords = dict(boundary_temperature=tb, boundary_emissivity=eb, remove_pedestal=False)

    def gpu(s=lengths, **changes):
        return np.asarray(spec.compute_radiance(s, **dict(keywords, **changes))["radiance"])

    def cpu(s=lengths, boundary_temperature=tb, boundary_emissivity=eb):
        values, _ = mirror(spec, beta, s, "toward_last", boundary_temperature,
                           boundary_emissivity)
        return values["radiance"].reshape(SHAPE[:-1] + (-1,))

    def scaled(factor):
        s = lengths.copy()
        s[..., level] = s[..., level]*factor
        return s

    out = spec.compute_jacobian(lengths, quantities=EVERYTHING, **keywords)
    values, _ = mirror(spec, beta, lengths, "toward_last", tb, eb)
    residues = {}
    for name, radiance, jacobian in (
            ("gpu", gpu, {q: np.asarray(out[q]) for q in EVERYTHING}),
            ("mirror", cpu, {q: values[q].reshape(np.asarray(out[q]).shape)
                             for q in EVERYTHING})):
        base = radiance()
        log = (radiance(scaled(1. + d)) - radiance(scaled(1. - d)))/(2.*d)
        k = jacobian["log_optical_depth_jacobian"][..., level, :]
        residues[name, "log"] = float(np.max(np.abs(log - k)/(np.abs(k) + base)))
        dt = (radiance(boundary_temperature=tb + h) - radiance(boundary_temperature=tb - h))/(2.*h)
        k = jacobian["boundary_temperature_jacobian"]
        residues[name, "boundary T"] = float(np.max(np.abs(dt - k)/(np.abs(k) + base/300.)))
        de = (radiance(boundary_emissivity=1.) - radiance(boundary_emissivity=0.5))/0.5
        k = jacobian["boundary_emissivity_jacobian"]
        residues[name, "emissivity"] = float(np.max(np.abs(de - k)/(np.abs(k) + base)))
    print("\nfinite-difference residues:", residues)
    for what in ("log", "boundary T", "emissivity"):
        assert residues["gpu", what] <= 10.*residues["mirror", what], (what, residues)
        assert residues["mirror", what] < 1e-7, (what, residues)     # the formulas, not rounding


def test_isothermal_atmosphere_behind_a_black_boundary():
    """I = B everywhere: dI/dx vanishes to rounding, and the temperature Jacobians with the
    boundary's add up to dB(nu, T) (sum_k a_k*trail_k + trail_b telescopes to 1)."""
    t = 250.
    spec = spectroscopy(temperature=t)
    beta = total_of(spec)
    lengths = lengths_for(beta, depth=6.)
    for direction in ("toward_last", "toward_first"):
        out = spec.compute_jacobian(lengths, boundary_temperature=t, direction=direction,
                                    quantities=EVERYTHING, remove_pedestal=False)
        _, magnitudes = mirror(spec, beta, lengths, direction, t)
        source = jac.cases.planck(np.float64, spec.grid, t)
        dx = np.asarray(out["optical_depth_jacobian"]).reshape(-1, spec.grid.size)
        # The magnitude is (|B| + |I|)*trail = 2 B trail here.
        assert np.all(np.abs(dx) <= BOUND*magnitudes["optical_depth_jacobian"])
        assert np.all(magnitudes["optical_depth_jacobian"] <= 2.*source*(1. + 1e-9))
        total = np.asarray(out["temperature_jacobian"]).sum(axis=-2) + \
            np.asarray(out["boundary_temperature_jacobian"])
        expected = jac.planck_dt(np.float64, spec.grid, t)
        assert np.max(np.abs(total - expected)/expected) <= BOUND


def test_very_long_and_zero_paths(fine):
    spec, beta, lengths = fine
    thinnest = np.min(lengths[..., None]*beta)
    assert thinnest > 0.
    long = lengths*(1000./thinnest)         # every layer saturates at every point: x >= 1000
    out = spec.compute_jacobian(long, boundary_temperature=288., quantities=EVERYTHING,
                                remove_pedestal=False)
    for q in EVERYTHING:
        assert np.all(np.isfinite(np.asarray(out[q]))), q
    for q in jac.PER_LEVEL:
        assert np.all(np.asarray(out[q])[..., :-1, :] == 0.), q
    assert np.all(np.asarray(out["boundary_temperature_jacobian"]) == 0.)
    assert np.all(np.asarray(out["boundary_emissivity_jacobian"]) == 0.)
    assert np.any(np.asarray(out["temperature_jacobian"])[..., -1, :] > 0.)
    out = spec.compute_jacobian(np.zeros(SHAPE), boundary_temperature=288.,
                                quantities=EVERYTHING, remove_pedestal=False)
    assert np.all(np.asarray(out["temperature_jacobian"]) == 0.)
    assert np.all(np.asarray(out["log_optical_depth_jacobian"]) == 0.)
    assert np.all(np.isfinite(np.asarray(out["optical_depth_jacobian"])))
    values, magnitudes = mirror(spec, beta, np.zeros(SHAPE), "toward_last", 288.)
    assert_close(out, values, magnitudes, EVERYTHING, "zero lengths")


def weighted(rows, weights):
    """(mean, 1e-12 * sum w|v| / sum w) of rows [..., N] under weights [C, N]; NaN rows where the
    weights sum to 0."""
    total = weights.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (rows @ weights.T)/total, BOUND*(np.abs(rows) @ np.abs(weights).T)/np.abs(total)


def assert_reduced(got, fine_rows, weights, nan, what):
    mean, bound = weighted(np.asarray(fine_rows), weights)
    got = np.asarray(got)
    assert got.shape == mean.shape, what
    assert np.array_equal(np.isnan(got), np.broadcast_to(nan, got.shape)), what
    ok = ~np.isnan(got)
    assert np.all(np.abs(got[ok] - mean[ok]) <= bound[ok] + 1e-300), what


@pytest.mark.parametrize("direction", ["toward_last", "toward_first"])
def test_band_means(fine, direction):
    spec, beta, lengths = fine
    edges = np.array([590., 600., 600.005, 612.3, 612.3 + 1e-9, 650., 699.99, 720.])
    keywords = dict(boundary_temperature=288., boundary_emissivity=0.95, direction=direction,
                    quantities=EVERYTHING, remove_pedestal=False)
    full = spec.compute_jacobian(lengths, **keywords)
    out = spec.compute_jacobian(lengths, band_edges=edges, **keywords)
    starts = band_columns(spec.grid, edges)
    weights = np.zeros((edges.size - 1, spec.grid.size))
    for b in range(edges.size - 1):
        weights[b, starts[b]:starts[b + 1]] = 1.
    empty = np.diff(starts) == 0
    assert empty.any() and not empty.all()
    assert np.array_equal(out["band_points"], np.diff(starts))
    for q in EVERYTHING:
        assert_reduced(out[q], full[q], weights, empty, (direction, q))
    some = spec.compute_jacobian(lengths, band_edges=edges, **dict(
        keywords, quantities=("temperature_jacobian", "boundary_emissivity_jacobian")))
    for q in ("temperature_jacobian", "boundary_emissivity_jacobian"):
        assert np.array_equal(bits(some[q]), bits(out[q])), q


INSTRUMENTS = {
    "boxcar": Instrument.boxcar(np.arange(603., 697., 0.25), 0.7),
    "overlapping gaussian": Instrument.gaussian(np.arange(603., 697., 0.25), 0.5, half_width=1.5),
    "partly outside": Instrument.gaussian(np.array([599.5, 600.2, 650., 699.8, 705.]), 0.5,
                                          half_width=1.5),
}


@pytest.mark.parametrize("name", sorted(INSTRUMENTS))
def test_instrument_channels(fine, name):
    spec, beta, lengths = fine
    x = INSTRUMENTS[name]
    keywords = dict(boundary_temperature=288., direction="toward_first", quantities=EVERYTHING,
                    remove_pedestal=False)
    full = spec.compute_jacobian(lengths, **keywords)
    out = spec.compute_jacobian(lengths, instrument=x, **keywords)
    weights = x.response(spec.grid)
    nan = ~x.covered(spec.grid) | ~(weights.sum(axis=1) > 0.)
    assert nan.any() == (name == "partly outside") and not nan.all()
    assert np.array_equal(out["channel_center"], x.centers)
    for q in EVERYTHING:
        lead = SHAPE if q in jac.PER_LEVEL else SHAPE[:-1]
        assert np.asarray(out[q]).shape == lead + (len(x),), q
        assert_reduced(out[q], full[q], weights, nan, (name, q))


def test_runs_of_whole_paths_and_repeats(fine):
    spec, beta, lengths = fine
    keywords = dict(boundary_temperature=np.array([270., 288., 305.]), quantities=EVERYTHING,
                    remove_pedestal=False)
    base = spec.compute_jacobian(lengths, **keywords)
    again = spec.compute_jacobian(lengths, **keywords)
    row = spec.grid.size*8
    blocks = 2 + len(jac.PER_LEVEL)         # beta, the work block, one per per-level quantity
    x = INSTRUMENTS["overlapping gaussian"]
    edges = [600., 620., 660., 700.]
    reduced = {"instrument": spec.compute_jacobian(lengths, instrument=x, **keywords),
               "bands": spec.compute_jacobian(lengths, band_edges=edges, **keywords)}
    split = spectroscopy()
    for paths_per_run in (1, 2):
        split.device_output_limit = paths_per_run*SHAPE[-1]*blocks*row + row
        for direction in ("toward_last", "toward_first"):
            whole = base if direction == "toward_last" else \
                spec.compute_jacobian(lengths, direction=direction, **keywords)
            got = split.compute_jacobian(lengths, direction=direction, **keywords)
            for q in EVERYTHING:
                assert np.array_equal(bits(got[q]), bits(whole[q])), (paths_per_run, direction, q)
        got = {"instrument": split.compute_jacobian(lengths, instrument=x, **keywords),
               "bands": split.compute_jacobian(lengths, band_edges=edges, **keywords)}
        for kind in got:
            for q in EVERYTHING:
                assert np.array_equal(bits(got[kind][q]), bits(reduced[kind][q])), (kind, q)
    for q in EVERYTHING:
        assert np.array_equal(bits(again[q]), bits(base[q])), q
    split.device_output_limit = SHAPE[-1]*blocks*row - 1
    with pytest.raises(ValueError, match="device_output_limit"):
        split.compute_jacobian(lengths, **keywords)


def test_group_is_not_implemented():
    spec = spectroscopy(group=True)
    with pytest.raises(NotImplementedError, match="compute_jacobian"):
        spec.compute_jacobian(np.ones(SHAPE))


def test_pedestal_removed_by_default_matches_its_absorption():
    """remove_pedestal=None follows the continua backend as in compute_radiance; the block may then
    hold small negative beta: the mirror's magnitudes (recurrences over absolute values) apply."""
    spec = spectroscopy()
    beta = total_of(spec, remove_pedestal=True)
    lengths = lengths_for(beta)
    out = spec.compute_jacobian(lengths, boundary_temperature=288., quantities=EVERYTHING,
                                remove_pedestal=True)
    values, magnitudes = mirror(spec, beta, lengths, "toward_last", 288.)
    assert_close(out, values, magnitudes, EVERYTHING, "pedestal")

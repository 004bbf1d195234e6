"""Spectroscopy.compute_radiance and compute_flux with source="linear_in_tau" on the GPU, on the
small synthetic atmosphere of tests/test_gpu_radiance.py: the isothermal limit, the opaque and the
thin limit, the sign of swapping a layer's edges, band means and instrument channels of the linear
radiance, fluxes against the radiance, heating rates, runs of levels, and that the default source
is bit for bit what a call without the keyword gives.

Bounds: where two GPU results are compared that sum the same non-negative terms in another order
(the isothermal limit) 1e-12 relative, the suite's bound for a radiance with beta >= 0; limits of
the update to the first neglected order, stated where they are used."""
import numpy as np
import pytest

from tests import linear_source_cases as linear
from tests import test_gpu_instrument as instrument_tests
from tests import test_gpu_radiance as radiance_tests

pytestmark = pytest.mark.gpu

LD = np.longdouble
SHAPE = radiance_tests.SHAPE
planck = radiance_tests.planck


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def source_of(out):
    return out.attrs.get("source") if hasattr(out, "attrs") else out.get("source")


def interfaces_for(shape, seed=0):
    """Interface temperatures that fall from 295 K by 4 to 9 K per level, per path."""
    rng = np.random.default_rng(seed)
    steps = rng.uniform(4., 9., size=shape[:-1] + (shape[-1] + 1,))
    return 295. - np.cumsum(steps, axis=-1)


@pytest.fixture(scope="module")
def fine():
    """radiance_tests' (3, 7) atmosphere without the pedestal: beta >= 0."""
    spec = radiance_tests.spectroscopy()
    beta = radiance_tests.total_of(spec)
    assert np.all(beta >= 0.)
    return spec, beta, radiance_tests.lengths_for(beta), interfaces_for(SHAPE)


def numpy_linear(spec, beta, lengths, interfaces, direction, boundary_temperature=None):
    """The long-double mirror for [..., L, N] blocks: (I, magnitude) after every level."""
    nu = spec.grid.astype(LD)
    lead = beta.shape[:-2]
    levels = beta.shape[-2]
    rad = np.zeros(lead + nu.shape, dtype=LD)
    if boundary_temperature is not None:
        rad = rad + linear.cases.planck(LD, nu, LD(boundary_temperature))
    mag = np.abs(rad)
    out, mags = np.zeros(beta.shape, dtype=LD), np.zeros(beta.shape, dtype=LD)
    from_last = direction == "toward_first"
    for l in (range(levels - 1, -1, -1) if from_last else range(levels)):
        enter, leave = (l + 1, l) if from_last else (l, l + 1)
        x = lengths[..., l, None].astype(LD)*beta[..., l, :].astype(LD)
        rad, mag = linear.update(
            LD, rad, mag, x, linear.cases.planck(LD, nu, interfaces[..., enter, None].astype(LD)),
            linear.cases.planck(LD, nu, interfaces[..., leave, None].astype(LD)))
        out[..., l, :], mags[..., l, :] = rad, mag
    return out, mags


@pytest.mark.parametrize("direction", ["toward_last", "toward_first"])
def test_radiance_meets_the_mirror(fine, direction):
    spec, beta, lengths, interfaces = fine
    out = spec.compute_radiance(lengths, boundary_temperature=288., direction=direction,
                                cumulative=True, remove_pedestal=False, source="linear_in_tau",
                                interface_temperature=interfaces)
    assert source_of(out) == "linear_in_tau"
    expect, magnitude = numpy_linear(spec, beta, lengths, interfaces, direction, 288.)
    got = np.asarray(out["radiance"])
    assert got.shape == beta.shape
    error = np.abs(got.astype(LD) - expect)
    print("worst error / bound:", float(np.max(error/(LD(1e-12)*magnitude))))
    assert np.all(error <= LD(1e-12)*magnitude)


@pytest.mark.parametrize("direction", ["toward_last", "toward_first"])
def test_equal_interface_temperatures_are_the_isothermal_atmosphere(direction):
    """T = 250 K everywhere: B_in = B_out = B and B*u_in + B*w = B*a up to rounding (all terms
    >= 0: 1e-12 relative is the suite's bound for such sums).  Not bit for bit."""
    spec = radiance_tests.spectroscopy(temperature=250.)
    beta = radiance_tests.total_of(spec)
    lengths = radiance_tests.lengths_for(beta)
    interfaces = np.full((SHAPE[0], SHAPE[1] + 1), 250.)
    keywords = dict(boundary_temperature=288., direction=direction, cumulative=True,
                    remove_pedestal=False)
    isothermal = np.asarray(spec.compute_radiance(lengths, **keywords)["radiance"])
    got = np.asarray(spec.compute_radiance(lengths, source="linear_in_tau",
                                           interface_temperature=interfaces,
                                           **keywords)["radiance"])
    radiance_tests.assert_relative(got, isothermal, 1e-12)
    flux_keywords = dict(surface_temperature=288., surface_emissivity=0.9,
                         surface="first" if direction == "toward_last" else "last",
                         remove_pedestal=False)
    thickness = lengths
    isothermal = spec.compute_flux(thickness, **flux_keywords)
    got = spec.compute_flux(thickness, source="linear_in_tau",
                            interface_temperature=interfaces, **flux_keywords)
    for q in ("upward_flux", "downward_flux"):
        radiance_tests.assert_relative(np.asarray(got[q]), np.asarray(isothermal[q]), 1e-12)


def test_opaque_and_thin_limits_and_swapped_edges():
    """One-level paths.  Opaque (x >= 50): I = B_out - (B_out - B_in)/x to exp(-50) = 2e-22 of B.
    Thin (x <= 1e-6): I = x*(B_in + B_out)/2 to x/3 relative.  Swapped edges: for every x > 0
    w > u_in, so the radiance is larger with the hotter edge on the side it leaves through."""
    shape = (2, 1)
    spec = radiance_tests.spectroscopy(shape)
    beta = radiance_tests.total_of(spec)
    assert np.all(beta > 0.)
    nu = spec.grid
    interfaces = np.array([[250., 300.], [280., 230.]])
    for direction, enter, leave in (("toward_last", 0, 1), ("toward_first", 1, 0)):
        b_in, b_out = planck(nu, interfaces[:, enter, None]), planck(nu, interfaces[:, leave, None])
        keywords = dict(direction=direction, remove_pedestal=False, source="linear_in_tau")
        opaque = np.full(shape, 50./beta.min())
        got = np.asarray(spec.compute_radiance(opaque, interface_temperature=interfaces,
                                               **keywords)["radiance"])
        x = opaque*beta[:, 0, :]
        np.testing.assert_allclose(got, b_out - (b_out - b_in)/x, rtol=1e-13, atol=0.)
        thin = np.full(shape, 1e-6/beta.max())
        got = np.asarray(spec.compute_radiance(thin, interface_temperature=interfaces,
                                               **keywords)["radiance"])
        x = thin*beta[:, 0, :]
        assert x.max() <= 1e-6*(1. + 1e-15)
        np.testing.assert_allclose(got, x*(b_in + b_out)/2., rtol=1e-6, atol=0.)
        middle = radiance_tests.lengths_for(beta, depth=2.)
        one = np.asarray(spec.compute_radiance(middle, interface_temperature=interfaces,
                                               **keywords)["radiance"])
        other = np.asarray(spec.compute_radiance(middle,
                                                 interface_temperature=interfaces[:, ::-1],
                                                 **keywords)["radiance"])
        hotter_out = interfaces[:, leave] > interfaces[:, enter]
        assert hotter_out.tolist() == ([True, False] if enter == 0 else [False, True])
        assert np.all(one[hotter_out] > other[hotter_out])
        assert np.all(one[~hotter_out] < other[~hotter_out])


def test_band_means_and_channels_reduce_the_linear_radiance(fine):
    spec, beta, lengths, interfaces = fine
    keywords = dict(boundary_temperature=290., remove_pedestal=False, source="linear_in_tau",
                    interface_temperature=interfaces)
    fine_grid = np.asarray(spec.compute_radiance(lengths, **keywords)["radiance"])
    edges = np.array([600., 612.5, 612.5004, 650., 699.995, 701.])
    banded = spec.compute_radiance(lengths, band_edges=edges, **keywords)
    assert source_of(banded) == "linear_in_tau"
    starts = np.searchsorted(spec.grid, edges, side="left")
    radiance_tests.assert_relative(np.asarray(banded["radiance"]),
                                   radiance_tests.numpy_band_means(fine_grid, starts), 1e-12)
    x = instrument_tests.SHAPES["gaussian"](np.arange(603., 697., 0.5))
    channels = spec.compute_radiance(lengths, instrument=x, **keywords)
    assert source_of(channels) == "linear_in_tau"
    instrument_tests.check(channels["radiance"], x, spec.grid, fine_grid)
    isothermal = np.asarray(spec.compute_radiance(lengths, boundary_temperature=290.,
                                                  remove_pedestal=False)["radiance"])
    assert not np.allclose(fine_grid, isothermal, rtol=1e-3, atol=0.)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_flux_of_one_vertical_angle_is_pi_times_the_radiance(fine, surface):
    spec, beta, lengths, interfaces = fine
    flux = spec.compute_flux(lengths, np.array([270., 288., 305.]), surface_emissivity=1.,
                             surface=surface, angles=([1.], [1.]),
                             quantities=("upward_flux", "downward_flux", "heating_rate"),
                             remove_pedestal=False, source="linear_in_tau",
                             interface_temperature=interfaces)
    assert source_of(flux) == "linear_in_tau"
    up_direction, down_direction = ("toward_last", "toward_first") if surface == "first" else \
        ("toward_first", "toward_last")
    keywords = dict(cumulative=True, remove_pedestal=False, source="linear_in_tau",
                    interface_temperature=interfaces)
    up = np.asarray(spec.compute_radiance(
        lengths, boundary_temperature=np.array([270., 288., 305.]), direction=up_direction,
        **keywords)["radiance"])
    down = np.asarray(spec.compute_radiance(lengths, direction=down_direction,
                                            **keywords)["radiance"])
    inner_up = slice(1, None) if surface == "first" else slice(0, -1)
    inner_down = slice(0, -1) if surface == "first" else slice(1, None)
    assert same_bits(np.asarray(flux["upward_flux"])[:, inner_up], np.pi*(1.*up))
    assert same_bits(np.asarray(flux["downward_flux"])[:, inner_down], np.pi*(1.*down))
    assert np.all(np.isfinite(np.asarray(flux["heating_rate"])))
    assert np.any(np.asarray(flux["heating_rate"]) != 0.)


def test_small_output_limit_gives_the_same_bits(fine):
    spec, beta, lengths, interfaces = fine
    n = spec.grid.size
    keywords = dict(remove_pedestal=False, source="linear_in_tau",
                    interface_temperature=interfaces)
    whole_rad = spec.compute_radiance(lengths, boundary_temperature=288., **keywords)
    whole_flux = spec.compute_flux(lengths, 288., surface_emissivity=0.8, **keywords)
    # Five levels of two blocks: runs that cut the paths of seven levels in the middle.
    small = radiance_tests.spectroscopy()
    small.device_output_limit = 5*2*n*8
    for direction in ("toward_last", "toward_first"):
        a = spec.compute_radiance(lengths, boundary_temperature=288., direction=direction,
                                  cumulative=True, **keywords)
        b = small.compute_radiance(lengths, boundary_temperature=288., direction=direction,
                                   cumulative=True, **keywords)
        assert same_bits(a["radiance"], b["radiance"])
    assert same_bits(small.compute_radiance(lengths, boundary_temperature=288.,
                                            **keywords)["radiance"], whole_rad["radiance"])
    got = small.compute_flux(lengths, 288., surface_emissivity=0.8, **keywords)
    for q in ("upward_flux", "downward_flux"):
        assert same_bits(got[q], whole_flux[q])


def test_isothermal_keyword_is_the_call_without_it(fine):
    spec, beta, lengths, interfaces = fine
    keywords = dict(boundary_temperature=288., quantities=("radiance", "brightness_temperature"),
                    cumulative=True)
    plain = spec.compute_radiance(lengths, **keywords)
    named = spec.compute_radiance(lengths, source="isothermal", **keywords)
    assert source_of(plain) is None and source_of(named) is None
    assert set(plain) == set(named)
    for q in ("radiance", "brightness_temperature"):
        assert same_bits(plain[q], named[q])
    plain = spec.compute_flux(lengths, 288., quantities=("upward_flux", "downward_flux",
                                                         "heating_rate"))
    named = spec.compute_flux(lengths, 288., source="isothermal",
                              quantities=("upward_flux", "downward_flux", "heating_rate"))
    assert source_of(named) is None and set(plain) == set(named)
    for q in ("upward_flux", "downward_flux", "heating_rate"):
        assert same_bits(plain[q], named[q])

"""Spectroscopy.compute_flux on the GPU against a numpy implementation of its definitions, in the
stated order of operations, over compute_absorption("total") of the same Spectroscopy; against
compute_radiance bit for bit with one angle; physical invariants; runs of levels, determinism
and threads."""
import threading

import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from pylbl_amd.spectroscopy import CP_DRY, PLANCK_C1, PLANCK_C2, R_DRY, flux_angles

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


def thickness_for(beta, seed=0, depth=5.):
    """Layer thicknesses [m] that keep the vertical optical depth of a path below ~depth."""
    lengths = np.random.default_rng(seed).uniform(0.5, 1.5, size=beta.shape[:-1])
    return lengths*depth/np.max(np.sum(np.abs(beta), axis=-2))


def planck(nu, t):
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        b = (((PLANCK_C1*nu)*nu)*nu)/np.expm1((PLANCK_C2*nu)/t)
    return np.where(nu > 0., b, 0.)


def weighted(weight, rad):
    """sum_k w_k*I_k from k = 0; rad [..., K, N]."""
    total = weight[0]*rad[..., 0, :]
    for k in range(1, weight.size):
        total = total + weight[k]*rad[..., k, :]
    return total


def numpy_flux(spec, beta, thickness, surface_temperature, surface_emissivity=1.,
               surface="first", angles=3, band_edges=None):
    """The definitions of compute_flux in numpy: {"upward_flux", "downward_flux",
    "heating_rate"} with the interfaces and levels of the result."""
    mu, weight = flux_angles(angles)
    nu = spec.grid
    temperature = spec.atmosphere.temperature
    lead = beta.shape[:-2]
    levels = beta.shape[-2]
    lengths = thickness[..., None]/mu                           # [..., L, K]
    ts = np.broadcast_to(np.asarray(surface_temperature, float), lead)
    es = np.broadcast_to(np.asarray(surface_emissivity, float), lead)
    down = np.zeros(lead + (levels + 1, nu.size))
    up = np.zeros(lead + (levels + 1, nu.size))
    toward_first = list(range(levels - 1, -1, -1))
    toward_last = list(range(levels))
    down_order, up_order = (toward_first, toward_last) if surface == "first" else \
        (toward_last, toward_first)

    def step(rad, l):
        x = lengths[..., l, :, None]*beta[..., l, None, :]
        source = planck(nu, temperature[..., l, None])[..., None, :]
        return rad*np.exp(-x) + source*(-np.expm1(-x))

    def at(l, order):
        return l if order is toward_first else l + 1

    rad = np.zeros(lead + (mu.size, nu.size))
    for l in down_order:
        rad = step(rad, l)
        down[..., at(l, down_order), :] = np.pi*weighted(weight, rad)
    reflected = weighted(weight, rad)
    start = es[..., None]*planck(nu, ts[..., None]) + (1. - es[..., None])*reflected
    rad = np.repeat(start[..., None, :], mu.size, axis=-2)
    up[..., 0 if surface == "first" else levels, :] = np.pi*weighted(weight, rad)
    for l in up_order:
        rad = step(rad, l)
        up[..., at(l, up_order), :] = np.pi*weighted(weight, rad)
    if band_edges is not None:
        starts = np.searchsorted(nu, band_edges, side="left")
        _, _, n_per_v = synthetic.grid_arguments(nu)
        up, down = (band_fluxes(f, starts, n_per_v) for f in (up, down))
    return {"upward_flux": up, "downward_flux": down,
            "heating_rate": heating(spec, up, down, thickness, surface)}


def band_fluxes(flux, starts, n_per_v):
    out = np.full(flux.shape[:-1] + (starts.size - 1,), np.nan)
    for b in range(starts.size - 1):
        count = starts[b + 1] - starts[b]
        if count > 0:
            out[..., b] = flux[..., starts[b]:starts[b + 1]].mean(axis=-1)*(count/n_per_v)
    return out


def net_difference(up, down, surface):
    """(Fnet at each level's interface nearer the surface, the other one)."""
    net = up - down
    return (net[..., :-1, :], net[..., 1:, :]) if surface == "first" else \
        (net[..., 1:, :], net[..., :-1, :])


def capacity(spec, thickness):
    rho = spec.atmosphere.pressure/(R_DRY*spec.atmosphere.temperature)
    return (rho*CP_DRY)*thickness


def heating(spec, up, down, thickness, surface):
    lower, upper = net_difference(up, down, surface)
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = (86400.*(lower - upper))/capacity(spec, thickness)[..., None]
    return np.where((thickness == 0.)[..., None], np.nan, rate)


def assert_relative(got, expect, bound):
    got, expect = np.asarray(got), np.asarray(expect)
    assert got.shape == expect.shape
    assert np.array_equal(np.isnan(got), np.isnan(expect))
    ok = ~np.isnan(expect)
    error = np.abs(got[ok] - expect[ok])/np.maximum(np.abs(expect[ok]), 1.e-300)
    assert error.size == 0 or error.max() <= bound, error.max()


def assert_heating(spec, got, expect, up, down, thickness, bound):
    """Heating rates are differences of fluxes: the error is bounded relative to the fluxes that
    enter them, not to the difference."""
    assert got.shape == expect.shape
    assert np.array_equal(np.isnan(got), np.isnan(expect))
    lower, upper = net_difference(np.abs(up), -np.abs(down), "first")
    scale = 86400.*(lower + upper)/capacity(spec, thickness)[..., None]
    ok = ~np.isnan(expect)
    error = np.abs(got[ok] - expect[ok])/np.maximum(scale[ok], 1.e-300)
    assert error.size == 0 or error.max() <= bound, error.max()


@pytest.fixture(scope="module")
def fine():
    """A (3, 7) atmosphere without the pedestal: beta >= 0, no cancellation in the sweeps."""
    spec = spectroscopy()
    beta = total_of(spec)
    assert np.all(beta >= 0.)
    return spec, beta, thickness_for(beta)


SURFACE_T = np.array([270., 288., 305.])
ALL = ("upward_flux", "downward_flux", "heating_rate")


@pytest.mark.parametrize("surface", ["first", "last"])
@pytest.mark.parametrize("emissivity", [1., 0.7, 0.])
@pytest.mark.parametrize("bands", [False, True])
def test_fluxes_and_heating_rates_match_numpy(fine, surface, emissivity, bands):
    spec, beta, thickness = fine
    edges = np.concatenate([[550., 600.5, 600.5005], np.arange(601.3, 700.1, 1.), [720.]]) \
        if bands else None
    out = spec.compute_flux(thickness, SURFACE_T, emissivity, surface=surface, quantities=ALL,
                            band_edges=edges, remove_pedestal=False)
    expect = numpy_flux(spec, beta, thickness, SURFACE_T, emissivity, surface, band_edges=edges)
    assert set(out) == set(ALL) | ({"band_lower", "band_upper", "band_points"} if bands
                                   else {"wavenumber"})
    for q in ("upward_flux", "downward_flux"):
        assert out[q].shape == (3, 8, spec.grid.size if not bands else edges.size - 1)
        assert_relative(out[q], expect[q], 1.e-12)
    assert_heating(spec, out["heating_rate"], expect["heating_rate"], expect["upward_flux"],
                   expect["downward_flux"], thickness, 1.e-12)
    space = -1 if surface == "first" else 0
    assert np.all(out["downward_flux"][:, space][~np.isnan(out["downward_flux"][:, space])] == 0.)


@pytest.mark.parametrize("angles", [1, 2, ([0.3, 0.9], [0.25, 0.75]), ([1./1.66], [1.])])
def test_other_angles_match_numpy(fine, angles):
    spec, beta, thickness = fine
    out = spec.compute_flux(thickness, 290., 0.9, angles=angles, remove_pedestal=False)
    expect = numpy_flux(spec, beta, thickness, 290., 0.9, angles=angles)
    for q in ("upward_flux", "downward_flux"):
        assert_relative(out[q], expect[q], 1.e-12)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_one_angle_is_compute_radiance_bit_for_bit(fine, surface):
    """K = 1, eps = 1: the fluxes are pi times compute_radiance's cumulative radiance along
    s/mu, downward without a boundary, upward from the surface as the boundary."""
    spec, beta, thickness = fine
    for angles in (1, ([0.37], [1.])):
        mu, _ = flux_angles(angles)
        out = spec.compute_flux(thickness, SURFACE_T, surface=surface, angles=angles,
                                remove_pedestal=False)
        toward_space, toward_surface = ("toward_last", "toward_first") if surface == "first" \
            else ("toward_first", "toward_last")
        down = spec.compute_radiance(thickness/mu[0], direction=toward_surface, cumulative=True,
                                     remove_pedestal=False)["radiance"]
        up = spec.compute_radiance(thickness/mu[0], boundary_temperature=SURFACE_T,
                                   direction=toward_space, cumulative=True,
                                   remove_pedestal=False)["radiance"]
        levels = slice(0, 7) if surface == "first" else slice(1, 8)
        above = slice(1, 8) if surface == "first" else slice(0, 7)
        assert np.array_equal(out["downward_flux"][:, levels], np.pi*down)
        assert np.array_equal(out["upward_flux"][:, above], np.pi*up)
        ground = 0 if surface == "first" else 7
        emitted = spec.compute_radiance(np.zeros(SHAPE), boundary_temperature=SURFACE_T)
        assert np.array_equal(out["upward_flux"][:, ground], np.pi*emitted["radiance"])


def test_zero_thickness_leaves_the_surface_term(fine):
    spec = fine[0]
    zero = np.zeros(SHAPE)
    emissivity = np.array([1., 0.6, 0.])
    for angles in (1, 3):
        out = spec.compute_flux(zero, SURFACE_T, emissivity, angles=angles, quantities=ALL)
        assert np.all(out["downward_flux"] == 0.)
        expect = np.pi*(emissivity[:, None]*planck(spec.grid, SURFACE_T[:, None]))
        emitted = spec.compute_radiance(zero, boundary_temperature=SURFACE_T,
                                        boundary_emissivity=emissivity)["radiance"]
        for i in range(8):
            assert_relative(out["upward_flux"][:, i], expect, 1.e-14)
            if angles == 1:
                # Exactly: the surface term goes through the levels unchanged.
                assert np.array_equal(out["upward_flux"][0, i], np.pi*emitted[0])
        assert np.all(out["upward_flux"][2] == 0.)
        assert np.all(np.isnan(out["heating_rate"]))


@pytest.mark.parametrize("surface", ["first", "last"])
def test_isothermal_atmosphere_over_a_black_surface_is_pi_planck(surface):
    spec = spectroscopy(temperature=250.)
    thickness = thickness_for(total_of(spec), seed=4)
    out = spec.compute_flux(thickness, 250., surface=surface, remove_pedestal=False)
    expect = np.broadcast_to(np.pi*planck(spec.grid, 250.), out["upward_flux"].shape)
    assert_relative(out["upward_flux"], expect, 1.e-13)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_a_perfect_reflector_sends_back_what_comes_down(fine, surface):
    spec, beta, thickness = fine
    ground = 0 if surface == "first" else 7
    for angles, bound in ((1, 0.), (3, 1.e-14)):
        out = spec.compute_flux(thickness, SURFACE_T, 0., surface=surface, angles=angles,
                                remove_pedestal=False)
        up, down = out["upward_flux"][:, ground], out["downward_flux"][:, ground]
        assert np.all(down > 0.)
        if bound == 0.:
            assert np.array_equal(up, down)
        else:
            assert_relative(up, down, bound)


@pytest.mark.parametrize("surface", ["first", "last"])
@pytest.mark.parametrize("bands", [False, True])
def test_heating_rates_add_up_to_the_net_flux_divergence(fine, surface, bands):
    spec, beta, thickness = fine
    edges = np.arange(600., 700.1, 2.5) if bands else None
    out = spec.compute_flux(thickness, SURFACE_T, 0.8, surface=surface, quantities=ALL,
                            band_edges=edges, remove_pedestal=False)
    heat = out["heating_rate"]*capacity(spec, thickness)[..., None]/86400.
    net = out["upward_flux"] - out["downward_flux"]
    ground, space = (0, -1) if surface == "first" else (-1, 0)
    expect = net[:, ground] - net[:, space]
    scale = np.abs(out["upward_flux"]).max(axis=1) + np.abs(out["downward_flux"]).max(axis=1)
    error = np.abs(np.sum(heat, axis=1) - expect)/scale
    assert error.max() <= 1.e-10, error.max()


@pytest.mark.parametrize("surface", ["first", "last"])
def test_pedestal_removed(surface):
    """With the pedestal removed beta goes negative at some points: still the numpy sweeps."""
    spec = spectroscopy()
    beta = total_of(spec, remove_pedestal=True)
    assert np.any(beta < 0.)
    thickness = thickness_for(beta, seed=3)
    out = spec.compute_flux(thickness, SURFACE_T, 0.9, surface=surface, remove_pedestal=True)
    expect = numpy_flux(spec, beta, thickness, SURFACE_T, 0.9, surface)
    for q in ("upward_flux", "downward_flux"):
        # (where the first layers emit a little less than nothing the flux passes through 0)
        scale = np.maximum(np.abs(expect[q]), 1.e-3*np.abs(expect[q]).max())
        error = np.abs(out[q] - expect[q])/scale
        assert error.max() <= 1.e-12, (q, error.max())


@pytest.mark.parametrize("surface", ["first", "last"])
def test_runs_of_levels_give_the_same_bits(surface):
    spec = spectroscopy()
    thickness = thickness_for(total_of(spec, True), seed=7)
    edges = np.arange(600., 700.1, 0.37)
    keywords = dict(surface=surface, quantities=ALL)
    whole = spec.compute_flux(thickness, SURFACE_T, 0.7, **keywords)
    whole_bands = spec.compute_flux(thickness, SURFACE_T, 0.7, band_edges=edges, **keywords)
    v0, vn, n_per_v = synthetic.grid_arguments(spec.grid)
    level_bytes = (vn - v0)*n_per_v*8
    for limit in (0, 4*level_bytes, 10*level_bytes):      # runs of 1, 2 and 5 levels
        spec.device_output_limit = limit
        chunked = spec.compute_flux(thickness, SURFACE_T, 0.7, **keywords)
        chunked_bands = spec.compute_flux(thickness, SURFACE_T, 0.7, band_edges=edges,
                                          **keywords)
        for q in ALL:
            assert np.array_equal(chunked[q], whole[q], equal_nan=True), (limit, q)
            assert np.array_equal(chunked_bands[q], whole_bands[q], equal_nan=True), (limit, q)


def test_repeated_calls_and_threads_give_the_same_bits():
    spec = spectroscopy()
    thickness = thickness_for(total_of(spec, True), seed=9)
    edges = np.arange(600., 700.1, 1.)
    calls = [dict(surface_temperature=290.),
             dict(surface_temperature=SURFACE_T, band_edges=edges, quantities=ALL),
             dict(surface_temperature=280., surface_emissivity=0.5, surface="last", angles=5),
             dict(surface_temperature=300., angles=([1./1.66], [1.]), band_edges=edges)]
    first = [spec.compute_flux(thickness, **c) for c in calls]
    again = [spec.compute_flux(thickness, **c) for c in calls]
    for a, b in zip(again, first):
        for q in ALL:
            if q in b:
                assert np.array_equal(a[q], b[q], equal_nan=True)
    got = {}

    def worker(index):
        got[index] = [spec.compute_flux(thickness, **c) for c in calls]
    threads = [threading.Thread(target=worker, args=(i,)) for i in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for index in range(3):
        for result, expect in zip(got[index], first):
            for q in ALL:
                if q in expect:
                    assert np.array_equal(result[q], expect[q], equal_nan=True)

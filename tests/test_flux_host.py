"""CPU-only checks of Spectroscopy.compute_flux: the argument checks (all raised before anything
touches the GPU), the quadrature, the dry-air constants, the heating-rate assembly, the C
header's declaration and flag, and the naming, dims, shapes and units of the result."""
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from pylbl_amd import spectroscopy
from pylbl_amd.spectroscopy import CP_DRY, R_DRY, flux_angles, heating_rate

ROOT = Path(__file__).resolve().parents[1]


def make_spectroscopy(shape=(5,), **keywords):
    tables = [synthetic.line_table("H2O", 590., 610., num_lines=50, seed=1)]
    full = synthetic.standard_atmosphere(int(np.prod(shape)))
    atmos = synthetic.Atmos(p=full.p.reshape(shape), t=full.t.reshape(shape),
                            vmr={"H2O": full.vmr["H2O"].reshape(shape)})
    return Spectroscopy(atmos, np.arange(600., 601., 0.01), MemoryDatabase(tables), **keywords)


@pytest.mark.parametrize("keywords, match", [
    (dict(layer_thickness=np.ones(4)), "shape"),
    (dict(layer_thickness=np.ones((3, 4))), "shape"),
    (dict(layer_thickness=np.ones((3, 5, 1))), "shape"),
    (dict(layer_thickness=-np.ones((3, 5))), ">= 0"),
    (dict(layer_thickness=np.full((3, 5), np.nan)), "finite"),
    (dict(layer_thickness=np.full((3, 5), np.inf)), "finite"),
    (dict(surface_temperature=np.ones(5)), "surface_temperature"),
    (dict(surface_temperature=np.ones((3, 5))), "surface_temperature"),
    (dict(surface_temperature=0.), "surface temperatures"),
    (dict(surface_temperature=-280.), "surface temperatures"),
    (dict(surface_temperature=np.inf), "surface temperatures"),
    (dict(surface_temperature=np.array([280., np.nan, 290.])), "surface temperatures"),
    (dict(surface_temperature=None), "surface temperatures"),
    (dict(surface_emissivity=1.5), "emissivities"),
    (dict(surface_emissivity=-0.1), "emissivities"),
    (dict(surface_emissivity=np.nan), "emissivities"),
    (dict(surface_emissivity=np.array([1., 1.01, 0.9])), "emissivities"),
    (dict(surface_emissivity=np.ones(4)), "surface_emissivity"),
    (dict(surface="top"), "surface"),
    (dict(surface=0), "surface"),
    (dict(angles=0), "angles"),
    (dict(angles=9), "angles"),
    (dict(angles=-1), "angles"),
    (dict(angles=True), "angles"),
    (dict(angles=2.), "angles"),
    (dict(angles="3"), "angles"),
    (dict(angles=([0.5, 0.5], [1.])), "angles"),
    (dict(angles=([[0.5]], [[1.]])), "angles"),
    (dict(angles=(np.full(9, 0.5), np.full(9, 1./9.))), "angles"),
    (dict(angles=([], [])), "angles"),
    (dict(angles=([0.], [1.])), r"\(0, 1\]"),
    (dict(angles=([-0.5], [1.])), r"\(0, 1\]"),
    (dict(angles=([1.2], [1.])), r"\(0, 1\]"),
    (dict(angles=([np.nan], [1.])), r"\(0, 1\]"),
    (dict(angles=([0.3, 0.7], [1.2, -0.2])), ">= 0"),
    (dict(angles=([0.5], [np.inf])), "finite"),
    (dict(angles=([0.6], [0.6])), "sum to 1"),
    (dict(angles=([0.2, 0.8], [0.5, 0.5 + 1.e-11])), "sum to 1"),
    (dict(angles=([0.2, 0.8], [0.1, 0.4])), "sum to 1"),     # w without the factor mu
    (dict(quantities=("upward_flux", "net_flux")), "quantities"),
    (dict(quantities="radiance"), "quantities"),
    (dict(quantities=()), "quantities"),
    (dict(band_edges=[600.5]), "band_edges"),
    (dict(band_edges=[601., 600.]), "increasing"),
    (dict(band_edges=[600., np.nan]), "finite"),
    (dict(range_policy="everything"), "range_policy"),
])
def test_bad_arguments_raise_before_the_gpu(keywords, match):
    spec = make_spectroscopy((3, 5))
    arguments = dict(layer_thickness=np.ones((3, 5)), surface_temperature=290.)
    arguments.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_flux(**arguments)
    assert spec.cache == {}             # no backend object was built: nothing touched the GPU


def test_weights_summing_to_one_within_rounding_are_taken():
    mu, weight = flux_angles(([0.2, 0.8], [0.5, 0.5 + 5.e-13]))
    assert np.array_equal(mu, [0.2, 0.8]) and np.array_equal(weight, [0.5, 0.5 + 5.e-13])
    mu, weight = flux_angles(([1./1.66], [1.]))
    assert mu[0] == 1./1.66 and weight[0] == 1.


def test_bad_level_temperatures_and_pressures_raise_before_the_gpu():
    spec = make_spectroscopy((5,))
    spec.atmosphere.temperature[2] = 0.
    with pytest.raises(ValueError, match="temperatures"):
        spec.compute_flux(np.ones(5), 290.)
    spec = make_spectroscopy((5,))
    spec.atmosphere.pressure[1] = -1.
    with pytest.raises(ValueError, match="pressures"):
        spec.compute_flux(np.ones(5), 290., quantities="heating_rate")
    assert spec.cache == {}


def test_group_is_not_implemented():
    spec = make_spectroscopy(group=True)
    with pytest.raises(NotImplementedError, match="compute_flux"):
        spec.compute_flux(np.ones(5), 290.)
    assert spec.cache == {}


@pytest.mark.parametrize("count", range(1, 9))
def test_gauss_legendre_nodes_and_weights(count):
    mu, weight = flux_angles(count)
    x, w = np.polynomial.legendre.leggauss(count)
    assert np.array_equal(mu, (x + 1.)/2.)
    assert np.array_equal(weight, ((x + 1.)/2.)*w)
    assert np.all((mu > 0.) & (mu <= 1.)) and np.all(weight > 0.)
    assert abs(np.sum(weight) - 1.) <= 1.e-14
    # sum_k weight_k mu_k^n = integral over (0, 1] of 2 mu mu^n = 2/(n + 2), for n <= 2K - 2.
    for n in range(2*count - 1):
        assert np.sum(weight*mu**n) == pytest.approx(2./(n + 2), rel=1.e-13, abs=0.), n


def test_dry_air_constants():
    assert R_DRY == 8.314462618/0.0289644
    assert CP_DRY == 3.5*R_DRY
    assert R_DRY == pytest.approx(287.05800, abs=1.e-5)
    assert CP_DRY == pytest.approx(1004.7030, abs=1.e-4)


@pytest.mark.parametrize("surface", ["first", "last"])
def test_heating_rate_assembly(surface):
    """Two paths of three levels: hand-made interface fluxes, written out level by level."""
    rng = np.random.default_rng(1)
    up = rng.uniform(100., 400., size=(2, 4, 3))
    down = rng.uniform(0., 300., size=(2, 4, 3))
    pressure = np.array([[1.e5, 8.e4, 6.e4], [9.e4, 7.e4, 5.e4]])
    temperature = np.array([[290., 280., 270.], [285., 275., 265.]])
    thickness = np.array([[500., 1000., 0.], [750., 250., 1500.]])
    got = heating_rate(up, down, pressure, temperature, thickness, surface)
    assert got.shape == (2, 3, 3)
    for p in range(2):
        for l in range(3):
            lower, upper = (l, l + 1) if surface == "first" else (l + 1, l)
            net_lower = up[p, lower] - down[p, lower]
            net_upper = up[p, upper] - down[p, upper]
            rho = pressure[p, l]/(R_DRY*temperature[p, l])
            if thickness[p, l] == 0.:
                assert np.all(np.isnan(got[p, l]))
                continue
            expect = (86400.*(net_lower - net_upper))/((rho*CP_DRY)*thickness[p, l])
            assert np.array_equal(got[p, l], expect)
    # A layer losing more net flux at its top than it gets at its base cools.
    up = np.zeros((1, 2, 1))
    down = np.zeros((1, 2, 1))
    up[0, 1 if surface == "first" else 0, 0] = 10.
    rate = heating_rate(up, down, [[1.e5]], [[300.]], [[1000.]], surface)
    assert rate[0, 0, 0] < 0.


def test_header_declares_lbl_path_flux_with_a_flag_of_its_own():
    header = (ROOT / "include" / "lbl_amd.h").read_text()
    assert re.search(r"int lbl_path_flux\(lbl_engine \*engine,", header)
    flags = {}
    for name, value in re.findall(r"#define\s+(LBL_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)\b", header):
        flags[name] = int(value, 0)
    up = flags["LBL_PATH_FLUX_UP"]
    assert up != 0 and up & (up - 1) == 0
    # Every flag that an entry point takes: the call flags and the path flags.
    others = ["LBL_OUT_DEVICE", "LBL_ASYNC", "LBL_SCALE_DENSITY", "LBL_ACCUMULATE",
              "LBL_FARFIELD", "LBL_DEFER_FINISH"] + \
        [n for n in flags if n.startswith("LBL_PATH_") and n != "LBL_PATH_FLUX_UP"]
    for name in others:
        assert flags[name] & up == 0, name
    from pylbl_amd import engine
    assert engine.PATH_FLUX_UP == up
    assert "lbl_path_flux" in engine.EXPORTED_SYMBOLS


def flux_request_of(spec, **keywords):
    arguments = dict(layer_thickness=np.ones(spec.atmosphere.temperature.shape),
                     surface_temperature=290., surface_emissivity=1., surface="first", angles=3,
                     quantities=spectroscopy.FLUX_QUANTITIES, band_edges=None,
                     range_policy="reference")
    arguments.update(keywords)
    return spec._flux_request(**arguments)


def test_request_broadcasts_the_surface_to_one_value_per_path():
    spec = make_spectroscopy((2, 3, 5))
    request = flux_request_of(spec, surface_temperature=280.,
                              surface_emissivity=np.full((2, 3), .5), surface="last",
                              angles=([1./1.66], [1.]))
    assert request.surface == "last"
    assert np.array_equal(request.surface_temperature, np.full(6, 280.))
    assert np.array_equal(request.surface_emissivity, np.full(6, .5))
    assert np.array_equal(request.mu, [1./1.66]) and np.array_equal(request.weight, [1.])
    assert request.quantities == spectroscopy.FLUX_QUANTITIES
    request = flux_request_of(spec, quantities=("heating_rate", "downward_flux"))
    assert request.quantities == ("downward_flux", "heating_rate")


def fake_sweeps(spec, request, seed=0):
    """What _sweep_runs hands back: per-level rows of each sweep and the surface rows."""
    per_path, paths = spectroscopy._path_layout(request.shape)
    width = spec.grid.size if request.starts is None else request.starts.size - 1
    rng = np.random.default_rng(seed)
    return {"downward_flux": rng.uniform(1., 2., (paths*per_path, width)),
            "upward_flux": rng.uniform(2., 3., (paths*per_path, width)),
            "surface_flux": rng.uniform(3., 4., (paths, width))}


@pytest.mark.parametrize("shape", [(5,), (3, 5)])
@pytest.mark.parametrize("bands", [False, True])
@pytest.mark.parametrize("surface", ["first", "last"])
def test_output_names_dims_and_shapes(monkeypatch, shape, bands, surface):
    """compute_flux with the GPU part monkeypatched: the interfaces are put together from the
    sweeps' rows, the bands scaled by their width, the heating rate formed from the result."""
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])     # the dict form, xarray or not
    spec = make_spectroscopy(shape)
    edges = [599., 600.2, 600.2001, 600.5] if bands else None
    thickness = np.full(shape, 100.)
    request = flux_request_of(spec, layer_thickness=thickness, band_edges=edges, surface=surface)
    sweeps = fake_sweeps(spec, request)
    calls = []

    def fake(self, request, passes, remove_pedestal, range_policy, sweeper, level_blocks=1):
        calls.append(passes)
        return sweeps
    monkeypatch.setattr(Spectroscopy, "_sweep_runs", fake)
    out = spec.compute_flux(thickness, 290., band_edges=edges, surface=surface,
                            quantities=spectroscopy.FLUX_QUANTITIES)
    (down_pass, up_pass), = calls
    assert down_pass.from_last == (surface == "first") and up_pass.from_last == (surface == "last")
    assert down_pass.level_quantities == ("downward_flux",)
    assert up_pass.level_quantities == ("upward_flux",)
    assert up_pass.path_quantities == ("surface_flux",)
    levels = shape[-1]
    width = 3 if bands else spec.grid.size
    lead = list(shape[:-1])
    assert set(out) == set(spectroscopy.FLUX_QUANTITIES) | (
        {"band_lower", "band_upper", "band_points"} if bands else {"wavenumber"})
    assert out["upward_flux"].shape == tuple(lead + [levels + 1, width])
    assert out["downward_flux"].shape == tuple(lead + [levels + 1, width])
    assert out["heating_rate"].shape == tuple(lead + [levels, width])
    scale = np.ones(width)
    if bands:
        starts = np.searchsorted(spec.grid, edges)
        scale = np.diff(starts)/100.            # n_b/n_per_v on a 0.01 cm-1 grid
        assert np.array_equal(out["band_points"], np.diff(starts))
    down = sweeps["downward_flux"].reshape(lead + [levels, width])
    up = sweeps["upward_flux"].reshape(lead + [levels, width])
    surface_row = sweeps["surface_flux"].reshape(lead + [width])
    got_down, got_up = out["downward_flux"], out["upward_flux"]
    space, ground = (-1, 0) if surface == "first" else (0, -1)
    inner = slice(0, levels) if surface == "first" else slice(1, levels + 1)
    assert np.array_equal(got_down[..., inner, :], down*scale)
    assert np.array_equal(got_up[..., ground, :], surface_row*scale)
    inner_up = slice(1, levels + 1) if surface == "first" else slice(0, levels)
    assert np.array_equal(got_up[..., inner_up, :], up*scale)
    empty = scale == 0.
    assert np.all(got_down[..., space, ~empty] == 0.)
    assert np.all(np.isnan(got_down[..., space, empty]))
    expect = heating_rate(got_up, got_down, spec.atmosphere.pressure,
                          spec.atmosphere.temperature, thickness, surface)
    assert np.array_equal(out["heating_rate"], expect, equal_nan=True)


class FakeXarray(object):
    """The slice of xarray the assembly touches, to check dims, coordinates and units."""
    class DataArray(object):
        def __init__(self, data, dims, attrs=None):
            self.data, self.dims, self.attrs = np.asarray(data), tuple(dims), dict(attrs or {})

    class Dataset(object):
        def __init__(self, data_vars, coords):
            self.data_vars, self.coords = data_vars, coords


@pytest.mark.parametrize("bands", [False, True])
def test_dataset_units_and_dims(monkeypatch, bands):
    monkeypatch.setattr(spectroscopy, "_XARRAY", [FakeXarray])
    spec = make_spectroscopy((3, 5))
    edges = [600., 600.5, 601.] if bands else None
    request = flux_request_of(spec, band_edges=edges)
    values = spec._flux_interfaces(fake_sweeps(spec, request), request)
    out = spec._create_flux_dataset(values, request)
    axis = "band" if bands else "wavenumber"
    assert out.data_vars["upward_flux"].dims == ("dim_0", "interface", axis)
    assert out.data_vars["downward_flux"].dims == ("dim_0", "interface", axis)
    assert out.data_vars["heating_rate"].dims == ("dim_0", "dim_1", axis)
    assert out.data_vars["upward_flux"].data.shape[1] == 6
    flux_units = "W m-2" if bands else "W m-2 (cm-1)-1"
    heating_units = "K day-1" if bands else "K day-1 (cm-1)-1"
    assert out.data_vars["upward_flux"].attrs == {"units": flux_units}
    assert out.data_vars["downward_flux"].attrs == {"units": flux_units}
    assert out.data_vars["heating_rate"].attrs == {"units": heating_units}
    assert set(out.coords) == ({"band_lower", "band_upper", "band_points"} if bands
                               else {"wavenumber"})

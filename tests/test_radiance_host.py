"""CPU-only checks of Spectroscopy.compute_radiance: the Planck constants (Python, C header and
CODATA agree; Stefan-Boltzmann from a numpy Planck function), the argument checks (all raised
before anything touches the GPU) and the naming and shapes of the result."""
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from pylbl_amd import spectroscopy
from pylbl_amd.spectroscopy import PLANCK_C1, PLANCK_C2

ROOT = Path(__file__).resolve().parents[1]

# CODATA 2018: exact by the definition of the SI units.
H, C, K = 6.62607015e-34, 299792458., 1.380649e-23
SIGMA = 5.670374419e-8          # Stefan-Boltzmann [W m-2 K-4], CODATA 2018


def planck(nu, t):
    """B(nu, T) [W m-2 sr-1 (cm-1)-1] in the order the docs state."""
    nu = np.asarray(nu, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        b = (((PLANCK_C1*nu)*nu)*nu)/np.expm1((PLANCK_C2*nu)/t)
    return np.where(nu > 0., b, 0.)


def test_constants_are_codata():
    assert PLANCK_C1 == pytest.approx(2.*H*C**2*1.e8, rel=2.e-16)
    assert PLANCK_C2 == pytest.approx(H*C/K*1.e2, rel=2.e-16)


def test_constants_match_the_c_header():
    header = (ROOT / "include" / "lbl_amd.h").read_text()
    found = {}
    for name in ("LBL_PLANCK_C1", "LBL_PLANCK_C2"):
        match = re.search(r"#define\s+" + name + r"\s+([0-9.eE+-]+)", header)
        assert match is not None, name
        found[name] = float(match.group(1))
    assert found["LBL_PLANCK_C1"] == PLANCK_C1
    assert found["LBL_PLANCK_C2"] == PLANCK_C2


def test_planck_integrates_to_stefan_boltzmann():
    """pi * integral of B over 1-5000 cm-1 at 300 K is sigma T^4 (the tails hold ~5e-8 of it)."""
    t = 300.
    nu = np.linspace(1., 5000., 499901)
    b = planck(nu, t)
    step = nu[1] - nu[0]
    integral = step*(np.sum(b) - 0.5*(b[0] + b[-1]))
    assert np.pi*integral == pytest.approx(SIGMA*t**4, rel=1.e-6)


def test_planck_is_zero_at_and_below_zero_wavenumber():
    assert np.array_equal(planck([-1., 0.], 300.), [0., 0.])


def make_spectroscopy(shape=(5,), **keywords):
    tables = [synthetic.line_table("H2O", 590., 610., num_lines=50, seed=1)]
    full = synthetic.standard_atmosphere(int(np.prod(shape)))
    atmos = synthetic.Atmos(p=full.p.reshape(shape), t=full.t.reshape(shape),
                            vmr={"H2O": full.vmr["H2O"].reshape(shape)})
    return Spectroscopy(atmos, np.arange(600., 601., 0.01), MemoryDatabase(tables), **keywords)


@pytest.mark.parametrize("keywords, match", [
    (dict(path_length=np.ones(4)), "shape"),
    (dict(path_length=np.ones((3, 4))), "shape"),
    (dict(path_length=np.ones((3, 5, 1))), "shape"),
    (dict(path_length=-np.ones((3, 5))), ">= 0"),
    (dict(path_length=np.full((3, 5), np.nan)), "finite"),
    (dict(path_length=np.full((3, 5), np.inf)), "finite"),
    (dict(boundary_temperature=np.ones(5)), "boundary_temperature"),
    (dict(boundary_temperature=np.ones((3, 5))), "boundary_temperature"),
    (dict(boundary_temperature=0.), "boundary temperatures"),
    (dict(boundary_temperature=-280.), "boundary temperatures"),
    (dict(boundary_temperature=np.inf), "boundary temperatures"),
    (dict(boundary_temperature=np.array([280., np.nan, 290.])), "boundary temperatures"),
    (dict(boundary_temperature=np.array([280., 0., 290.])), "boundary temperatures"),
    (dict(boundary_emissivity=1.5), "emissivities"),
    (dict(boundary_emissivity=-0.1), "emissivities"),
    (dict(boundary_emissivity=np.nan), "emissivities"),
    (dict(boundary_emissivity=np.array([1., 1.01, 0.9])), "emissivities"),
    (dict(boundary_emissivity=np.ones(4)), "boundary_emissivity"),
    (dict(direction="up"), "direction"),
    (dict(direction=None), "direction"),
    (dict(quantities=("radiance", "optical_depth")), "quantities"),
    (dict(quantities="transmittance"), "quantities"),
    (dict(quantities=()), "quantities"),
    (dict(cumulative="from_first"), "cumulative"),
    (dict(cumulative=None), "cumulative"),
    (dict(band_edges=[600.5]), "band_edges"),
    (dict(band_edges=[601., 600.]), "increasing"),
    (dict(band_edges=[600., np.nan]), "finite"),
    (dict(band_edges=[600., 601.], quantities="brightness_temperature"), "brightness"),
    (dict(band_edges=[600., 601.], quantities=("radiance", "brightness_temperature")),
     "brightness"),
    (dict(range_policy="everything"), "range_policy"),
])
def test_bad_arguments_raise_before_the_gpu(keywords, match):
    spec = make_spectroscopy((3, 5))
    arguments = dict(path_length=np.ones((3, 5)), boundary_temperature=290.)
    arguments.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_radiance(**arguments)
    assert spec.cache == {}             # no backend object was built: nothing touched the GPU


def test_bad_level_temperatures_raise_before_the_gpu():
    spec = make_spectroscopy((5,))
    spec.atmosphere.temperature[2] = 0.
    with pytest.raises(ValueError, match="temperatures"):
        spec.compute_radiance(np.ones(5))
    assert spec.cache == {}


def test_group_is_not_implemented():
    spec = make_spectroscopy(group=True)
    with pytest.raises(NotImplementedError, match="compute_radiance"):
        spec.compute_radiance(np.ones(5))
    assert spec.cache == {}


def request_of(spec, **keywords):
    arguments = dict(path_length=np.ones(spec.atmosphere.temperature.shape),
                     boundary_temperature=None, boundary_emissivity=1., direction="toward_last",
                     quantities=spectroscopy.RADIANCE_QUANTITIES, band_edges=None,
                     cumulative=False, range_policy="reference")
    arguments.update(keywords)
    return spec._radiance_request(**arguments)


def test_request_broadcasts_boundaries_to_one_value_per_path():
    spec = make_spectroscopy((2, 3, 5))
    request = request_of(spec, boundary_temperature=280., boundary_emissivity=np.full((2, 3), .5),
                         direction="toward_first")
    assert request.from_last and not request.cumulative
    assert np.array_equal(request.boundary_temperature, np.full(6, 280.))
    assert np.array_equal(request.boundary_emissivity, np.full(6, .5))
    temperatures = np.arange(6.).reshape(2, 3) + 250.
    request = request_of(spec, boundary_temperature=temperatures)
    assert np.array_equal(request.boundary_temperature, temperatures.ravel())
    assert request_of(spec).boundary_temperature is None
    one_path = request_of(make_spectroscopy((5,)), boundary_temperature=np.float64(280.))
    assert np.array_equal(one_path.boundary_temperature, [280.])


@pytest.mark.parametrize("shape", [(5,), (3, 5)])
@pytest.mark.parametrize("cumulative", [False, True])
@pytest.mark.parametrize("bands", [False, True])
def test_output_names_dims_and_shapes(monkeypatch, shape, cumulative, bands):
    """The dataset-assembly helper, fed arrays as the GPU side would return them."""
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])     # the dict form, xarray or not
    spec = make_spectroscopy(shape)
    edges = [599., 600.2, 600.2001, 600.5] if bands else None
    quantities = ("radiance",) if bands else spectroscopy.RADIANCE_QUANTITIES
    request = request_of(spec, band_edges=edges, cumulative=cumulative, quantities=quantities)
    assert request.quantities == quantities
    rows = int(np.prod(shape)) if cumulative else int(np.prod(shape[:-1]))
    width = 3 if bands else spec.grid.size
    values = {q: np.arange(rows*width, dtype=np.float64).reshape(rows, width) + i
              for i, q in enumerate(request.quantities)}
    out = spec._create_path_dataset(values, request)
    lead = list(shape) if cumulative else list(shape[:-1])
    assert set(out) == set(quantities) | ({"band_lower", "band_upper", "band_points"} if bands
                                          else {"wavenumber"})
    for q in quantities:
        assert out[q].shape == tuple(lead + [width])
        assert np.array_equal(out[q].reshape(rows, width), values[q])


class FakeXarray(object):
    """The slice of xarray the assembly touches, to check dims, coordinates and units."""
    class DataArray(object):
        def __init__(self, data, dims, attrs=None):
            self.data, self.dims, self.attrs = np.asarray(data), tuple(dims), dict(attrs or {})

    class Dataset(object):
        def __init__(self, data_vars, coords):
            self.data_vars, self.coords = data_vars, coords


@pytest.mark.parametrize("cumulative", [False, True])
def test_dataset_units_and_dims(monkeypatch, cumulative):
    monkeypatch.setattr(spectroscopy, "_XARRAY", [FakeXarray])
    spec = make_spectroscopy((3, 5))
    request = request_of(spec, cumulative=cumulative)
    rows = 15 if cumulative else 3
    out = spec._create_path_dataset({q: np.zeros((rows, spec.grid.size))
                                     for q in request.quantities}, request)
    dims = ("dim_0", "dim_1", "wavenumber") if cumulative else ("dim_0", "wavenumber")
    assert out.data_vars["radiance"].attrs == {"units": "W m-2 sr-1 (cm-1)-1"}
    assert out.data_vars["brightness_temperature"].attrs == {"units": "K"}
    for var in out.data_vars.values():
        assert var.dims == dims
    assert set(out.coords) == {"wavenumber"}

"""CPU-only checks of Spectroscopy.compute_path: band edges -> column ranges, the argument checks
(all raised before anything touches the GPU) and the naming and shapes of the result."""
import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from pylbl_amd import spectroscopy
from pylbl_amd.spectroscopy import band_columns


def brute_force_columns(grid, edges):
    """Band b as the list of columns j with e_b <= grid[j] < e_b+1."""
    return [[j for j in range(grid.size) if edges[b] <= grid[j] < edges[b + 1]]
            for b in range(len(edges) - 1)]


@pytest.mark.parametrize("edges", [
    [600.005, 600.0351, 600.1],                 # between grid points
    [600.01, 600.05, 600.06, 600.07],           # on grid points
    [590., 600.02, 600.5],                      # below the grid
    [600.08, 600.2, 700.],                      # above the grid
    [500., 550., 600.0149, 600.0151, 600.016],  # empty bands, a single point
    [599., 601.],                               # the whole grid
    [700., 800.],                               # nothing at all
])
def test_band_columns_match_membership(edges):
    grid = np.arange(600., 600.1, 0.005)
    starts = band_columns(grid, edges)
    assert starts.dtype == np.int64 and starts.shape == (len(edges),)
    for b, members in enumerate(brute_force_columns(grid, edges)):
        assert list(range(starts[b], starts[b + 1])) == members, b


def test_band_columns_single_point_band():
    grid = np.arange(600., 601., 0.01)
    starts = band_columns(grid, [grid[40], np.nextafter(grid[40], np.inf)])
    assert list(starts) == [40, 41]


def make_spectroscopy(shape=(5,), **keywords):
    tables = [synthetic.line_table("H2O", 590., 610., num_lines=50, seed=1)]
    full = synthetic.standard_atmosphere(int(np.prod(shape)))
    atmos = synthetic.Atmos(p=full.p.reshape(shape), t=full.t.reshape(shape),
                            vmr={"H2O": full.vmr["H2O"].reshape(shape)})
    return Spectroscopy(atmos, np.arange(600., 601., 0.01), MemoryDatabase(tables), **keywords)


@pytest.mark.parametrize("keywords, match", [
    (dict(path_length=np.ones(4)), "shape"),
    (dict(path_length=np.ones((5, 1))), "shape"),
    (dict(path_length=np.array([1., 1., -1., 1., 1.])), ">= 0"),
    (dict(path_length=np.array([1., 1., np.nan, 1., 1.])), "finite"),
    (dict(path_length=np.array([1., np.inf, 1., 1., 1.])), "finite"),
    (dict(quantities=("optical_depth", "radiance")), "quantities"),
    (dict(quantities="absorption"), "quantities"),
    (dict(quantities=()), "quantities"),
    (dict(cumulative="to_top"), "cumulative"),
    (dict(cumulative=True), "cumulative"),
    (dict(band_edges=[600.5]), "band_edges"),
    (dict(band_edges=[[600., 601.]]), "band_edges"),
    (dict(band_edges=[600.5, 600.5, 601.]), "increasing"),
    (dict(band_edges=[601., 600.]), "increasing"),
    (dict(band_edges=[600., np.nan]), "finite"),
    (dict(band_edges=[-np.inf, 600.]), "finite"),
    (dict(range_policy="everything"), "range_policy"),
])
def test_bad_arguments_raise_before_the_gpu(keywords, match):
    spec = make_spectroscopy()
    arguments = dict(path_length=np.ones(5))
    arguments.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_path(**arguments)
    assert spec.cache == {}             # no backend object was built: nothing touched the GPU


def test_group_is_not_implemented():
    spec = make_spectroscopy(group=True)
    with pytest.raises(NotImplementedError):
        spec.compute_path(np.ones(5))
    assert spec.cache == {}


def request_of(spec, **keywords):
    arguments = dict(path_length=np.ones(spec.atmosphere.temperature.shape))
    arguments.update(keywords)
    return spec._path_request(arguments.pop("path_length"),
                              arguments.pop("quantities", spectroscopy.PATH_QUANTITIES),
                              arguments.pop("band_edges", None), arguments.pop("cumulative", None),
                              "reference")


@pytest.mark.parametrize("shape", [(5,), (3, 5)])
@pytest.mark.parametrize("cumulative", [None, "from_first", "from_last"])
@pytest.mark.parametrize("bands", [False, True])
def test_output_names_dims_and_shapes(monkeypatch, shape, cumulative, bands):
    """The dataset-assembly helper, fed arrays as the GPU side would return them: one row per
    path (or per level when cumulative), one column per grid point (or band)."""
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])     # the dict form, xarray or not
    spec = make_spectroscopy(shape)
    edges = [599., 600.2, 600.2001, 600.5] if bands else None
    request = request_of(spec, band_edges=edges, cumulative=cumulative)
    rows = int(np.prod(shape)) if cumulative else int(np.prod(shape[:-1]))
    width = 3 if bands else spec.grid.size
    values = {q: np.arange(rows*width, dtype=np.float64).reshape(rows, width) + i
              for i, q in enumerate(request.quantities)}
    out = spec._create_path_dataset(values, request)
    lead = list(shape) if cumulative else list(shape[:-1])
    for i, q in enumerate(("optical_depth", "transmittance")):
        assert out[q].shape == tuple(lead + [width])
        assert np.array_equal(out[q].reshape(rows, width), values[q])
    if bands:
        assert "wavenumber" not in out
        assert np.array_equal(out["band_lower"], edges[:-1])
        assert np.array_equal(out["band_upper"], edges[1:])
        assert list(out["band_points"]) == [len(m) for m in brute_force_columns(spec.grid, edges)]
        assert out["band_points"][1] == 0
    else:
        assert np.array_equal(out["wavenumber"], spec.grid)
        assert "band_points" not in out


def test_output_keeps_only_the_quantities_asked_for(monkeypatch):
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    spec = make_spectroscopy((3, 5))
    request = request_of(spec, quantities="transmittance")
    assert request.quantities == ("transmittance",)
    out = spec._create_path_dataset({"transmittance": np.ones((3, spec.grid.size))}, request)
    assert set(out) == {"wavenumber", "transmittance"}
    assert out["transmittance"].shape == (3, spec.grid.size)


class FakeXarray(object):
    """The slice of xarray the assembly touches, to check dims and coordinates."""
    class DataArray(object):
        def __init__(self, data, dims, attrs=None):
            self.data, self.dims, self.attrs = np.asarray(data), tuple(dims), dict(attrs or {})

    class Dataset(object):
        def __init__(self, data_vars, coords):
            self.data_vars, self.coords = data_vars, coords


@pytest.mark.parametrize("cumulative", [None, "from_last"])
def test_dataset_dims_follow_the_atmosphere(monkeypatch, cumulative):
    monkeypatch.setattr(spectroscopy, "_XARRAY", [FakeXarray])
    spec = make_spectroscopy((3, 5))
    request = request_of(spec, band_edges=[600., 600.5, 601.], cumulative=cumulative)
    rows = 15 if cumulative else 3
    out = spec._create_path_dataset({q: np.zeros((rows, 2)) for q in request.quantities},
                                    request)
    dims = ("dim_0", "dim_1", "band") if cumulative else ("dim_0", "band")
    assert set(out.data_vars) == {"optical_depth", "transmittance"}
    for var in out.data_vars.values():
        assert var.dims == dims
    assert set(out.coords) == {"band_lower", "band_upper", "band_points"}
    assert all(c.dims == ("band",) for c in out.coords.values())

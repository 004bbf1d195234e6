"""CPU-only checks of pylbl_amd.instrument: every constructor's response() against the formulas
of the docs, the window columns, the NaN rules of the numpy reference, and the argument checks
of the constructors and of compute_path / compute_radiance (all raised before anything touches
the GPU)."""
import numpy as np
import pytest

from pylbl_amd import Instrument, MemoryDatabase, Spectroscopy, synthetic
from pylbl_amd.instrument import GAUSSIAN_G, brightness_temperature
from pylbl_amd.spectroscopy import PLANCK_C1, PLANCK_C2

GRID = np.arange(600., 610., 0.01)


def sinc(x):
    x = np.asarray(x, dtype=np.float64)
    out = np.ones_like(x)
    nz = x != 0.
    out[nz] = np.sin(np.pi*x[nz])/(np.pi*x[nz])
    return out


def window_mask(nu, lo, hi):
    return (nu[None, :] >= np.asarray(lo)[:, None]) & (nu[None, :] <= np.asarray(hi)[:, None])


def test_gaussian_constant_is_four_ln_two():
    assert GAUSSIAN_G == 4.*np.log(2.)


def test_boxcar_response():
    x = Instrument.boxcar([602., 605.5], 1.)
    w = x.response(GRID)
    expected = window_mask(GRID, [601.5, 605.], [602.5, 606.]).astype(float)
    np.testing.assert_array_equal(w, expected)


def test_triangle_response():
    x = Instrument.triangle([603., 604.], [0.5, 0.25])
    w = x.response(GRID)
    fwhm = np.array([0.5, 0.25])[:, None]
    d = GRID[None, :] - np.array([603., 604.])[:, None]
    expected = np.where(window_mask(GRID, [602.5, 603.75], [603.5, 604.25]),
                        1. - np.abs(d)/fwhm, 0.)
    np.testing.assert_allclose(w, expected, rtol=0., atol=1e-15)
    assert w[0, np.argmin(np.abs(GRID - 603.))] == pytest.approx(1.)


def test_gaussian_response_and_default_half_width():
    x = Instrument.gaussian([605.], 0.5)
    lo, hi = x.window()
    assert lo[0] == 605. - 1.5 and hi[0] == 605. + 1.5
    w = x.response(GRID)
    d = GRID - 605.
    expected = np.where((GRID >= 603.5) & (GRID <= 606.5), np.exp(-GAUSSIAN_G*(d/0.5)**2), 0.)
    np.testing.assert_allclose(w[0], expected, rtol=1e-15, atol=0.)
    # half maximum at fwhm/2
    half = Instrument.gaussian([605.], 0.5, half_width=1.)
    assert half.response(np.array([604.75, 605., 605.25]))[0] == pytest.approx([0.5, 1., 0.5])


@pytest.mark.parametrize("apodization", ["none", "hamming"])
def test_fts_response(apodization):
    length = 2.
    x = Instrument.fts([605.], length, apodization=apodization, half_width=2.)
    w = x.response(GRID)[0]
    d = GRID - 605.
    s = sinc(2.*length*d)
    if apodization == "hamming":
        shift = 1./(2.*length)
        s = 0.54*s + 0.23*(sinc(2.*length*(d - shift)) + sinc(2.*length*(d + shift)))
    expected = np.where(window_mask(GRID, [603.], [607.])[0], s, 0.)
    np.testing.assert_allclose(w, expected, rtol=1e-13, atol=1e-15)
    # the peak: 1, or 0.54 with Hamming's side lobes at the sinc's first zeros
    assert w[np.argmin(np.abs(d))] == pytest.approx(1. if apodization == "none" else 0.54)
    if apodization == "none":       # zeros of the sinc at multiples of 1/(2L)
        assert x.response(np.array([605.25, 605.5]))[0] == pytest.approx([0., 0.], abs=1e-15)


def test_tabulated_response_shared_and_per_channel():
    offsets = [-1., 0., 0.5, 1.]
    table = [0., 1., 0.25, 0.]
    shared = Instrument.tabulated([603., 606.], offsets, table)
    w = shared.response(GRID)
    for i, c in enumerate([603., 606.]):
        expected = np.where((GRID >= c - 1.) & (GRID <= c + 1.),
                            np.interp(GRID - c, offsets, table), 0.)
        np.testing.assert_allclose(w[i], expected, rtol=0., atol=1e-15)
    rows = [[0., 1., 0.25, 0.], [1., 1., 1., 1.]]
    own = Instrument.tabulated([603., 606.], offsets, rows)
    w = own.response(GRID)
    np.testing.assert_array_equal(w[1], np.where((GRID >= 605.) & (GRID <= 607.), 1., 0.))


def test_window_columns_are_searchsorted_and_closed():
    grid = np.arange(0., 10.)
    x = Instrument.boxcar([3., 5.5], 2.)      # [2, 4] and [4.5, 6.5]
    start, end = x.columns(grid)
    np.testing.assert_array_equal(start, [2, 5])
    np.testing.assert_array_equal(end, [5, 7])      # 4 is inside the closed window [2, 4]
    np.testing.assert_array_equal(start, np.searchsorted(grid, [2., 4.5], "left"))
    np.testing.assert_array_equal(end, np.searchsorted(grid, [4., 6.5], "right"))


def test_nan_rules_of_the_reference():
    grid = np.arange(0., 10.)
    values = np.arange(20.).reshape(2, 10)
    x = Instrument.boxcar([3., 5.5, 0.5, 9.5, 2.5], [2., 0.5, 2., 2., 0.8])
    out = x.apply(grid, values)
    assert out.shape == (2, 5)
    np.testing.assert_allclose(out[:, 0], values[:, 2:5].mean(axis=1))
    assert np.all(np.isnan(out[:, 1]))      # [5.25, 5.75]: no point
    assert np.all(np.isnan(out[:, 2]))      # [-0.5, 1.5]: partly below the grid
    assert np.all(np.isnan(out[:, 3]))      # [8.5, 10.5]: partly above it
    assert np.all(np.isnan(out[:, 4]))      # [2.1, 2.9]: no point
    # weights that sum to 0 (w = -Delta at Delta = -1, 0, 1) or to < 0
    zero = Instrument.tabulated([5.], [-1., 1.], [1., -1.])
    assert zero.response(grid).sum() == 0.
    assert np.all(np.isnan(zero.apply(grid, values)))
    negative = Instrument.tabulated([5.], [-1., 1.], [-1., 0.])
    assert negative.response(grid).sum() < 0.
    assert np.all(np.isnan(negative.apply(grid, values)))
    # tabulated with a table that is 0 at every point of the window
    flat = Instrument.tabulated([5.], [-1., 1.], [0., 0.])
    assert np.all(np.isnan(flat.apply(grid, values)))


def test_unsorted_centres_keep_their_order():
    x = Instrument.gaussian([606., 602., 604.], 0.3)
    y = Instrument.gaussian([602., 604., 606.], 0.3)
    values = np.sin(GRID)[None, :]
    np.testing.assert_allclose(x.apply(GRID, values)[0], y.apply(GRID, values)[0][[2, 0, 1]],
                               rtol=1e-14)


def test_boxcar_matches_band_means():
    from pylbl_amd.spectroscopy import band_columns
    edges = np.arange(600.005, 609.01, 1.)          # no grid point on an edge
    starts = band_columns(GRID, edges)
    values = np.cos(GRID*3.)[None, :]
    means = np.array([values[0, a:b].mean() for a, b in zip(starts[:-1], starts[1:])])
    x = Instrument.boxcar((edges[:-1] + edges[1:])/2., np.diff(edges))
    np.testing.assert_allclose(x.apply(GRID, values)[0], means, rtol=1e-13)


def test_brightness_temperature_of_channels():
    nu = np.array([600., 650., 700., 700.])
    t = 280.
    radiance = (((PLANCK_C1*nu)*nu)*nu)/np.expm1((PLANCK_C2*nu)/t)
    radiance[2] = -1.
    radiance[3] = np.nan
    bt = brightness_temperature(radiance, nu)
    np.testing.assert_allclose(bt[:2], t, rtol=1e-13)
    assert bt[2] == 0. and np.isnan(bt[3])


def test_instrument_is_immutable():
    x = Instrument.boxcar([601.], 1.)
    with pytest.raises(AttributeError):
        x.foo = 1
    with pytest.raises(ValueError):
        x.centers[0] = 5.


@pytest.mark.parametrize("build, match", [
    (lambda: Instrument.boxcar([], 1.), "at least one"),
    (lambda: Instrument.boxcar([601., np.nan], 1.), "finite"),
    (lambda: Instrument.boxcar([601., np.inf], 1.), "finite"),
    (lambda: Instrument.boxcar([601.], 0.), "width"),
    (lambda: Instrument.boxcar([601.], -1.), "width"),
    (lambda: Instrument.boxcar([601., 602.], [1., 1., 1.]), "width"),
    (lambda: Instrument.triangle([601.], np.nan), "fwhm"),
    (lambda: Instrument.gaussian([601.], 0.), "fwhm"),
    (lambda: Instrument.gaussian([601.], 0.5, half_width=0.), "half_width"),
    (lambda: Instrument.gaussian([601.], 0.5, half_width=np.inf), "half_width"),
    (lambda: Instrument.fts([601.], 1.), "half_width"),
    (lambda: Instrument.fts([601.], 0., half_width=1.), "max_path_difference"),
    (lambda: Instrument.fts([601.], 1., apodization="kaiser", half_width=1.), "apodization"),
    (lambda: Instrument.tabulated([601.], [0.], [1.]), "offsets"),
    (lambda: Instrument.tabulated([601.], [0., 0., 1.], [1., 1., 1.]), "increasing"),
    (lambda: Instrument.tabulated([601.], [1., 0.], [1., 1.]), "increasing"),
    (lambda: Instrument.tabulated([601.], [0., np.nan], [1., 1.]), "finite"),
    (lambda: Instrument.tabulated([601.], [0., 1.], [1., 1., 1.]), "response"),
    (lambda: Instrument.tabulated([601., 602.], [0., 1.], np.ones((3, 2))), "response"),
    (lambda: Instrument.tabulated([601.], [0., 1.], [1., np.nan]), "finite"),
])
def test_bad_constructors_raise(build, match):
    with pytest.raises(ValueError, match=match):
        build()


def make_spectroscopy(shape=(3, 5)):
    tables = [synthetic.line_table("H2O", 590., 610., num_lines=50, seed=1)]
    full = synthetic.standard_atmosphere(int(np.prod(shape)))
    atmos = synthetic.Atmos(p=full.p.reshape(shape), t=full.t.reshape(shape),
                            vmr={"H2O": full.vmr["H2O"].reshape(shape)})
    return Spectroscopy(atmos, np.arange(600., 601., 0.01), MemoryDatabase(tables))


@pytest.mark.parametrize("method", ["compute_path", "compute_radiance"])
@pytest.mark.parametrize("keywords, match", [
    (dict(band_edges=[600., 601.], instrument=Instrument.boxcar([600.5], 0.5)), "not both"),
    (dict(instrument="boxcar"), "Instrument"),
])
def test_bad_path_arguments_raise_before_the_gpu(method, keywords, match):
    spec = make_spectroscopy()
    arguments = dict(path_length=np.ones((3, 5)))
    arguments.update(keywords)
    with pytest.raises(ValueError, match=match):
        getattr(spec, method)(**arguments)
    assert spec.cache == {}


def test_instrument_needs_an_increasing_grid():
    spec = make_spectroscopy()
    spec.grid = spec.grid[::-1].copy()
    with pytest.raises(ValueError, match="increasing"):
        spec.compute_path(np.ones((3, 5)), instrument=Instrument.boxcar([600.5], 0.5))
    assert spec.cache == {}


@pytest.mark.parametrize("kind", ["uniform", "jittered"])
@pytest.mark.parametrize("name", ["boxcar", "triangle", "gaussian", "fts", "fts-hamming",
                                  "tabulated"])
def test_probe_channel_sets_reach_every_tile_and_segment_edge(kind, name):
    """The channel sets of tests/test_gpu_instrument_limits.py's identity probe, through a numpy
    mirror of the sort and tiling of lbl_instrument_create: they reach the edges a rewrite of
    the apply breaks first."""
    from tests import instrument_cases as cases
    grid = cases.probe_grid(kind)
    assert grid.size % 8 != 0 and np.all(np.diff(grid) > 0.)
    x = cases.probe_instrument(name, grid)
    need = cases.TABULATED_CASES if name == "tabulated" else cases.CASES
    missing = [case for case in need if case not in cases.coverage(x, grid)]
    assert not missing, missing
    tiles = cases.tiling(x, grid)
    # every column of a valid window lies in one of its channel's items
    for c in np.flatnonzero(tiles["valid"]):
        spans = [tiles["items"][i] for i in range(tiles["first_item"][c],
                                                  tiles["first_item"][c] + tiles["n_items"][c])]
        assert all(t == tiles["tile"][c] for t, _, _ in spans)
        assert spans[0][1] <= tiles["begin"][c] < spans[0][2]
        assert spans[-1][1] < tiles["end"][c] <= spans[-1][2]
        assert all(a[2] == b[1] for a, b in zip(spans, spans[1:]))


def test_launch_chunk_of_the_apply():
    from tests import instrument_cases as cases
    assert cases.launch_chunk(8192, 150) == 64               # the partial-sum cap
    assert cases.launch_chunk(8191, 150) == 128
    assert cases.launch_chunk(5, 65535 + 77) == 65535          # the grid's y dimension
    assert cases.launch_chunk(0, 70) == 70                     # no valid channel

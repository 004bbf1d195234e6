"""Spectroscopy.compute_kdistribution on the GPU against plain numpy applied to
compute_absorption("total") of the same Spectroscopy: the sorted block bit for bit, quantiles bit
for bit, interval means within 1e-12 x the mean of |k| of the long-double mean; runs of one and two
levels give the same bits; an empty band gives NaN; one band may hold the whole grid."""
import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from tests import kdistribution_cases as cases

pytestmark = pytest.mark.gpu

GASES = ("H2O", "CO2", "O3")
SHAPE = (2, 3)
GRID = np.arange(600., 660., 0.01)              # 6000 points: a band of more than one chunk
EDGES = np.array([590., 599.5, 610., 610.004, 655., 660.5])    # empty, ~1000, empty, ~4500, ~500
ALL = ("absorption_g_mean", "absorption_g_quantile", "sorted_absorption")
_CACHE = {}


def spectroscopy(**keywords):
    if "tables" not in _CACHE:
        _CACHE["tables"] = [synthetic.line_table(name, 576., 684., num_lines=2000, seed=70 + i)
                            for i, name in enumerate(GASES)]
    full = synthetic.standard_atmosphere(int(np.prod(SHAPE)))
    atmosphere = synthetic.Atmos(p=full.p.reshape(SHAPE), t=full.t.reshape(SHAPE),
                                 vmr={k: full.vmr[k].reshape(SHAPE) for k in GASES})
    spec = Spectroscopy(atmosphere, GRID, MemoryDatabase(_CACHE["tables"]))
    for name, value in keywords.items():
        setattr(spec, name, value)
    return spec


def total():
    """compute_absorption("total") [2, 3, grid], formed once and left unchanged."""
    if "total" not in _CACHE:
        beta = np.array(spectroscopy().compute_absorption("total")["absorption"])
        beta.setflags(write=False)
        _CACHE["total"] = beta
    return _CACHE["total"]


def reference(g_edges, g_points):
    beta = total()
    starts = np.searchsorted(GRID, EDGES, side="left")
    flat = beta.reshape(-1, GRID.size)
    ordered = cases.sort_bands(flat, starts)
    in_band = np.zeros(GRID.size, dtype=bool)
    for b in range(starts.size - 1):
        in_band[starts[b]:starts[b + 1]] = True
    ordered[:, ~in_band] = np.nan
    return starts, ordered


def test_quantities_against_numpy():
    g_edges, g_points = cases.gauss_edges(16), cases.gauss_points(16)
    starts, ordered = reference(g_edges, g_points)
    out = spectroscopy().compute_kdistribution(EDGES, quantities=ALL)
    points = np.diff(starts)
    assert points[0] == 0 and points[2] == 0 and points[1] > 0 and points[3] > 4096
    assert np.array_equal(out["band_points"], np.diff(starts))
    assert cases.same_bits(out["g_lower"], g_edges[:-1]) and cases.same_bits(out["g_upper"], g_edges[1:])
    assert cases.same_bits(out["g_weight"], np.diff(g_edges)) and cases.same_bits(out["g_point"], g_points)
    assert np.array_equal(np.asarray(out["g_interval_points"]).sum(axis=1), np.diff(starts))
    got = np.asarray(out["sorted_absorption"])
    assert got.shape == SHAPE + (GRID.size,)
    nan = np.isnan(ordered)
    assert np.array_equal(np.isnan(got.reshape(ordered.shape)), nan)
    assert cases.same_bits(got.reshape(ordered.shape)[~nan], ordered[~nan])
    g = np.asarray(out["g"])
    assert g[starts[1]] == 0.5/points[1] and g[starts[2] - 1] == (points[1] - 0.5)/points[1]
    assert starts[-1] == GRID.size and not np.any(np.isnan(g))
    means = np.asarray(out["absorption_g_mean"]).reshape(-1, 5, 16)
    quantiles = np.asarray(out["absorption_g_quantile"]).reshape(-1, 5, 16)
    assert np.asarray(out["absorption_g_mean"]).shape == SHAPE + (5, 16)
    worst = 0.
    for level in range(ordered.shape[0]):
        for b in range(5):
            band = ordered[level, starts[b]:starts[b + 1]]
            assert cases.same_bits_or_nan(quantiles[level, b], cases.quantiles(band, g_points))
            if band.size == 0:
                assert np.all(np.isnan(means[level, b])) and np.all(np.isnan(quantiles[level, b]))
                continue
            mean, magnitude = cases.interval_means(band, g_edges)
            assert np.array_equal(np.isnan(means[level, b]), np.isnan(mean))
            ok = ~np.isnan(mean)
            error = np.abs(means[level, b][ok].astype(np.longdouble) - mean[ok])
            worst = max(worst, float(np.max(error/(cases.MEAN_BOUND*magnitude[ok]))))
            assert np.all(error <= cases.MEAN_BOUND*magnitude[ok])
            assert np.array_equal(np.asarray(out["g_interval_points"])[b],
                                  np.diff(cases.interval_bounds(band.size, g_edges)))
    print("worst mean error / bound: %.3g" % worst)


@pytest.mark.parametrize("levels", [1, 2])
def test_runs_of_levels_give_the_same_bits(levels):
    """A device_output_limit that holds beta and the scratch of `levels` levels only."""
    g_edges = [0., 0.25, 0.9, 1.]
    whole = spectroscopy().compute_kdistribution(EDGES, g_edges, [0., 0.4, 1.], quantities=ALL)
    limit = levels*2*GRID.size*8 + 64
    cut = spectroscopy(device_output_limit=limit).compute_kdistribution(
        EDGES, g_edges, [0., 0.4, 1.], quantities=ALL)
    for name in ALL:
        assert cases.same_bits(np.asarray(cut[name]), np.asarray(whole[name])), name
    again = spectroscopy().compute_kdistribution(EDGES, g_edges, [0., 0.4, 1.], quantities=ALL)
    for name in ALL:
        assert cases.same_bits(np.asarray(again[name]), np.asarray(whole[name])), name


def test_one_band_holds_the_whole_grid():
    beta = total().reshape(-1, GRID.size)
    out = spectroscopy().compute_kdistribution(
        [599., 661.], g_edges=1, g_points=[0., 0.5, 1.],
        quantities=("absorption_g_mean", "absorption_g_quantile", "sorted_absorption"))
    ordered = np.stack([cases.key_sort(row) for row in beta])
    assert cases.same_bits(np.asarray(out["sorted_absorption"]).reshape(ordered.shape), ordered)
    quantiles = np.asarray(out["absorption_g_quantile"]).reshape(-1, 3)
    assert cases.same_bits(quantiles[:, 0], ordered[:, 0])
    assert cases.same_bits(quantiles[:, 2], ordered[:, -1])
    for level in range(ordered.shape[0]):
        assert cases.same_bits(quantiles[level], cases.quantiles(ordered[level], [0., 0.5, 1.]))
    mean = np.mean(ordered.astype(np.longdouble), axis=1)
    error = np.abs(np.asarray(out["absorption_g_mean"]).reshape(-1).astype(np.longdouble) - mean)
    assert np.all(error <= cases.MEAN_BOUND*np.mean(np.abs(ordered).astype(np.longdouble), axis=1))
    only = spectroscopy().compute_kdistribution([599., 661.], g_edges=1)
    assert "sorted_absorption" not in only and "absorption_g_quantile" not in only
    assert cases.same_bits(np.asarray(only["absorption_g_mean"]),
                           np.asarray(out["absorption_g_mean"]))

"""Spectroscopy.compute_kdistribution at the shapes test_gpu_kdistribution.py does not run, each
against plain numpy applied to compute_absorption("total") of the same Spectroscopy and keywords
(tests/kdistribution_cases.py): remove_pedestal and range_policy; atmospheres of shape (5,), (1, 1)
and (5, 1) cut into runs of 2, 2 and 1 levels, all quantities and the means alone; bands of exactly
0, 1, 2 and 4097 points with Q = 1 and Q = 64 and g points that are neither sorted nor distinct;
and what the quantities must satisfy among themselves.

Bounds, none from the code under test: sorted rows and quantiles bit for bit; interval means within
1e-12 x the mean of |k| of the long-double mean; run cuts give identical bits."""
import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from tests import kdistribution_cases as cases

pytestmark = pytest.mark.gpu

LD = np.longdouble
GASES = ("H2O", "CO2")
GRID = np.arange(600., 630., 0.01)                      # 3000 points
EDGES = np.array([599., 604.995, 604.996, 612.495, 629.985, 631.])
POINTS = [500, 0, 750, 1749, 1]                         # of the bands of EDGES
ALL = ("absorption_g_mean", "absorption_g_quantile", "sorted_absorption")
# 0, 1, 4097 and 2 points of a grid of 4100: the first edge below the grid, the last above it.
EDGE_GRID = 600. + 0.01*np.arange(4100)
EDGE_EDGES = np.array([598., 599.5, 600.005, 640.975, 642.])
G_POINTS = [1., 0., 0.5, 0.5]
_CACHE = {}
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for what, ratio in sorted(WORST.items()):
        print("\nworst error / bound, kdistribution shapes, %s: %.3g" % (what, ratio))


def spectroscopy(shape, grid=GRID, **keywords):
    if "tables" not in _CACHE:
        _CACHE["tables"] = [synthetic.line_table(name, 576., 684., num_lines=200, seed=40 + i)
                            for i, name in enumerate(GASES)]
    full = synthetic.standard_atmosphere(int(np.prod(shape)))
    atmosphere = synthetic.Atmos(p=full.p.reshape(shape), t=full.t.reshape(shape),
                                 vmr={k: full.vmr[k].reshape(shape) for k in GASES})
    spec = Spectroscopy(atmosphere, grid, MemoryDatabase(_CACHE["tables"]))
    for name, value in keywords.items():
        setattr(spec, name, value)
    return spec


def total(shape, grid=GRID, **policies):
    """compute_absorption("total", **policies) [levels, grid], formed once and left unchanged."""
    key = (shape, grid.size) + tuple(sorted(policies.items()))
    if key not in _CACHE:
        beta = np.array(spectroscopy(shape, grid).compute_absorption("total", **policies)
                        ["absorption"]).reshape(-1, grid.size)
        beta.setflags(write=False)
        _CACHE[key] = beta
    return _CACHE[key]


def against_numpy(what, out, beta, grid, edges, g_edges, g_points, shape):
    """Every quantity and coordinate of `out` against the numpy oracle applied to `beta`."""
    starts = np.searchsorted(grid, edges, side="left")
    bands, q, p = starts.size - 1, len(g_edges) - 1, len(g_points)
    ordered = cases.sort_bands(beta, starts)
    got = np.asarray(out["sorted_absorption"])
    assert got.shape == tuple(shape) + (grid.size,), what
    got = got.reshape(ordered.shape)
    in_band = np.zeros(grid.size, dtype=bool)
    in_band[starts[0]:starts[-1]] = True
    assert np.all(np.isnan(got[:, ~in_band])), what
    assert cases.same_bits(got[:, in_band], ordered[:, in_band]), what
    assert np.array_equal(out["band_points"], np.diff(starts)), what
    assert cases.same_bits(out["g_lower"], g_edges[:-1]) and cases.same_bits(out["g_upper"], g_edges[1:])
    assert cases.same_bits(out["g_weight"], np.diff(g_edges)) and cases.same_bits(out["g_point"], g_points)
    assert cases.same_bits(out["band_lower"], edges[:-1]) and cases.same_bits(out["band_upper"], edges[1:])
    g = np.asarray(out["g"])
    assert g.shape == (grid.size,) and np.array_equal(np.isnan(g), ~in_band), what
    means = np.asarray(out["absorption_g_mean"])
    quantiles = np.asarray(out["absorption_g_quantile"])
    assert means.shape == tuple(shape) + (bands, q) and quantiles.shape == tuple(shape) + (bands, p)
    means, quantiles = means.reshape(-1, bands, q), quantiles.reshape(-1, bands, p)
    interval_points = np.asarray(out["g_interval_points"])
    assert interval_points.shape == (bands, q)
    for b in range(bands):
        n = starts[b + 1] - starts[b]
        bounds = cases.interval_bounds(n, g_edges)
        assert np.array_equal(interval_points[b], np.diff(bounds)), (what, b)
        if n > 0:
            expected = (np.arange(n) + 0.5)/n
            assert cases.same_bits(g[starts[b]:starts[b + 1]], expected), (what, b)
        for level in range(ordered.shape[0]):
            band = ordered[level, starts[b]:starts[b + 1]]
            assert cases.same_bits_or_nan(quantiles[level, b], cases.quantiles(band, g_points)), \
                (what, level, b)
            if n == 0:
                assert np.all(np.isnan(means[level, b])) and np.all(np.isnan(quantiles[level, b]))
                continue
            assert np.all(np.isfinite(band)), (what, level, b)
            mean, magnitude = cases.interval_means(band, g_edges)
            empty = np.isnan(mean)
            mine = means[level, b].astype(LD)
            assert np.array_equal(np.isnan(mine), empty), (what, level, b)
            error = np.abs(mine[~empty] - mean[~empty])
            allowed = cases.MEAN_BOUND*magnitude[~empty]
            WORST["means"] = max(WORST.get("means", 0.), float(np.max(error/allowed)))
            assert np.all(error <= allowed), (what, level, b)
            # -- what the quantities satisfy among themselves, in long double ------------------
            long = band.astype(LD)
            counts = np.diff(bounds)
            gap = abs(np.sum(counts[~empty].astype(LD)*mine[~empty]) - np.sum(long))
            allowed = cases.MEAN_BOUND*np.sum(np.abs(long))
            WORST["sums"] = max(WORST.get("sums", 0.), float(gap/allowed))
            assert gap <= allowed, (what, level, b)
            for interval in np.flatnonzero(~empty):
                first, last = long[bounds[interval]], long[bounds[interval + 1] - 1]
                assert first <= mine[interval] <= last, (what, level, b, interval)
            for point, at in enumerate(g_points):
                if at == 0.:
                    assert cases.same_bits(quantiles[level, b, point], band[0]), (what, level, b)
                if at == 1.:
                    assert cases.same_bits(quantiles[level, b, point], band[-1]), (what, level, b)
            rising = np.argsort(g_points, kind="stable")
            assert np.all(np.diff(quantiles[level, b][rising]) >= 0.), (what, level, b)
            if n == 1:
                assert cases.same_bits(quantiles[level, b], np.full(p, band[0])), (what, level, b)
                assert not empty[0] and np.all(empty[1:]), (what, b)


@pytest.mark.parametrize("range_policy", ["reference", "skip"])
@pytest.mark.parametrize("remove_pedestal", [None, True, False])
def test_policies(remove_pedestal, range_policy):
    """The keywords reach the absorption the distribution is formed of."""
    policies = dict(remove_pedestal=remove_pedestal, range_policy=range_policy)
    shape = (2,)
    g_edges, g_points = cases.gauss_edges(16), cases.gauss_points(16)
    out = spectroscopy(shape).compute_kdistribution(EDGES, quantities=ALL, **policies)
    against_numpy(policies, out, total(shape, **policies), GRID, EDGES, g_edges, g_points, shape)


def test_policies_differ():
    """The cases of test_policies are different cases: the blocks they start from differ."""
    shape = (2,)
    blocks = [total(shape, remove_pedestal=pedestal, range_policy=policy)
              for pedestal in (True, False) for policy in ("reference", "skip")]
    assert not cases.same_bits(blocks[0], blocks[2])        # the pedestal


@pytest.mark.parametrize("shape", [(5,), (1, 1), (5, 1)])
def test_atmosphere_shapes_and_run_cuts(shape):
    """Runs of 2, 2 and 1 levels (a limit for two levels), and a limit that does not hold one
    level -- runs of one level, as compute_path takes them -- give the bits of the uncut call,
    which is held to the oracle; so does a request for the means alone."""
    g_edges, g_points = np.array([0., 0.25, 0.9, 1.]), np.array([0., 0.4, 1.])
    whole = spectroscopy(shape).compute_kdistribution(EDGES, g_edges, g_points, quantities=ALL)
    against_numpy(shape, whole, total(shape), GRID, EDGES, g_edges, g_points, shape)
    levels = int(np.prod(shape))
    assert np.diff(np.searchsorted(GRID, EDGES)).tolist() == POINTS
    v0, vn, n_per_v = synthetic.grid_arguments(GRID)
    level_bytes = 2*(vn - v0)*n_per_v*8         # beta and the sort's scratch
    from pylbl_amd import paths
    for limit, lengths in ((2*level_bytes + 64, [2, 2, 1]), (level_bytes - 8, [1]*5)):
        _, runs = paths._cut_runs(levels, shape[-1], level_bytes, limit)
        assert [b - a for a, b in runs] == ([1] if levels == 1 else lengths)
        cut = spectroscopy(shape, device_output_limit=limit).compute_kdistribution(
            EDGES, g_edges, g_points, quantities=ALL)
        for name in ALL:
            assert cases.same_bits(np.asarray(cut[name]), np.asarray(whole[name])), (limit, name)
        only = spectroscopy(shape, device_output_limit=limit).compute_kdistribution(
            EDGES, g_edges, g_points)
        assert "sorted_absorption" not in only and "absorption_g_quantile" not in only
        assert cases.same_bits(np.asarray(only["absorption_g_mean"]),
                               np.asarray(whole["absorption_g_mean"])), limit


@pytest.mark.parametrize("q", [1, 64])
def test_band_edges(q):
    """Bands of exactly 0, 1, 4097 and 2 points, the first edge below the grid and the last above
    it; g points 1, 0, 0.5, 0.5.  A band of one point has that value at every g point and a mean
    in its first interval alone."""
    shape = (2,)
    g_edges, g_points = cases.gauss_edges(q), np.array(G_POINTS)
    starts = np.searchsorted(EDGE_GRID, EDGE_EDGES, side="left")
    assert np.diff(starts).tolist() == [0, 1, 4097, 2]
    assert EDGE_EDGES[0] < EDGE_GRID[0] and EDGE_EDGES[-1] > EDGE_GRID[-1]
    out = spectroscopy(shape, EDGE_GRID).compute_kdistribution(EDGE_EDGES, q, G_POINTS,
                                                               quantities=ALL)
    against_numpy(("edges", q), out, total(shape, EDGE_GRID), EDGE_GRID, EDGE_EDGES, g_edges,
                  g_points, shape)
    quantiles = np.asarray(out["absorption_g_quantile"])
    assert cases.same_bits(quantiles[..., 2], quantiles[..., 3])       # the repeated g point
    # runs of one level: the same bits
    cut = spectroscopy(shape, EDGE_GRID, device_output_limit=8).compute_kdistribution(
        EDGE_EDGES, q, G_POINTS, quantities=ALL)
    for name in ALL:
        assert cases.same_bits(np.asarray(cut[name]), np.asarray(out[name])), name

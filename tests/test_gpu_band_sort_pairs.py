"""lbl_band_distribution_weighted fed directly (Engine.band_distribution_weighted on rows held in
torch tensors), in the style of test_gpu_band_sort_shapes.py.  Band lengths
(kdistribution_weighted_cases.LENGTHS): 1, 7, 8, 9, 127..130, 4095..4097 (no and one merge pass),
2*4096 + 5 and 3*4096 + 1 (a run without a partner, an odd and an even number of passes),
6143..6145 and one band of 2^15 + 1 -- each alone in a row and all packed side by side with
unaligned starts, empty bands between and unbanded columns at both ends; 3 rows; padded strides
and a base 8 bytes off 16-byte alignment with sentinels in the padding and the unbanded columns.
Values on which ties decide: all equal, two values, plateaus that straddle the chunk and tile
boundaries (as equal bits and as +-0), +-0 mixes, NaNs of several payloads (the one whose key is
the pad key among them, in short chunks too), +-inf, and random ones.

Bounds, none from the code under test: pi is numpy's stable argsort of the integer keys exactly;
the sorted values, the means and the quantiles are numpy's bits and lbl_band_distribution's on a
copy; with a weight row W and WK are exact (a gather and one product); the sums lie within
MEAN_BOUND = 1e-12 x the sum of the magnitudes of their terms of the long-double sums (the bound
the project holds its ordered band means to); with row temperatures W lies within 1e-14 of the
long-double Planck function -- six roundings of 1.1e-16, the two of x = (C2 nu)/T amplified by
x e^x/(e^x - 1) <= 9 on this grid (nu <= 1100 cm-1, T >= 180 K), and an expm1 of a few ulp -- and
the sums hold the same bound against it; layouts and cutting the rows over two calls give
identical bits; refused calls write nothing."""
import numpy as np
import pytest

from tests import kdistribution_cases as cases
from tests import kdistribution_weighted_cases as wc
from tests.sweep_cases import LAYOUTS

pytestmark = pytest.mark.gpu

F64, LD, U64 = np.float64, np.longdouble, np.uint64
SENTINEL, INDEX_SENTINEL = wc.SENTINEL, wc.INDEX_SENTINEL
G_EDGES = np.array([0., 0.3, 0.30000000000000004, 0.55, 0.9, 1.])
G_POINTS = np.array([0., 0.013, 0.5, 0.77, 1.])
PLANCK_BOUND = LD(1e-14)
WORST = {}


class Rows(object):
    """A torch tensor [rows, row stride] on the GPU, as the engine's blocks."""
    def __init__(self, tensor):
        assert tensor.dim() == 2 and tensor.stride(1) == 1 and tensor.stride(0) == tensor.shape[1]
        self.tensor = tensor
        self.pointer, self.shape = tensor.data_ptr(), tuple(tensor.shape)


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    yield default_engine(0)
    for what, ratio in sorted(WORST.items()):
        print("\nworst error / bound, %s: %.3g" % (what, ratio))


def block(values, rows, columns, layout, fill):
    """float64 [rows, stride] on the GPU in `layout`: `values` [rows, columns] (None: `fill`) in
    the first `columns` values of each row, `fill` in the padding."""
    import torch
    layout = LAYOUTS[layout]
    stride = layout.stride(columns)
    host = np.full((rows, stride), fill, dtype=F64)
    if values is not None:
        host[:, :columns] = values
    flat = torch.full((rows*stride + 2,), fill, dtype=torch.float64, device="cuda:0")
    view = flat[layout.offset:layout.offset + rows*stride].view(rows, stride)
    view.copy_(torch.from_numpy(host))
    return view


def index_block(rows, stride):
    import torch
    return torch.full((rows, stride), INDEX_SENTINEL, dtype=torch.int32, device="cuda:0")


def plain(rows, width):
    import torch
    return torch.full((rows, width), SENTINEL, dtype=torch.float64, device="cuda:0")


def tables(starts):
    """(flat interval starts, point index, point fraction) of the bands, stated per band."""
    counts = np.diff(starts)
    index = np.full((counts.size, len(G_POINTS)), -1, dtype=np.int64)
    fraction = np.zeros((counts.size, len(G_POINTS)))
    for b, n in enumerate(counts):
        for p, g in enumerate(G_POINTS):
            if n > 0:
                index[b, p], fraction[b, p] = cases.quantile_index(n, g)
    return wc.flat_intervals(starts, G_EDGES), index, fraction


def run(engine, values, starts, weights=None, temperatures=None, grid=-1, layout="aligned",
        leave_out=()):
    """One call on `values` [rows, columns] with a weight row [columns] or row temperatures, and
    every output but those of `leave_out`: {name: numpy array}; the sentinels of the padding are
    checked to come back untouched."""
    import torch
    rows, columns = values.shape
    bands = starts.size - 1
    intervals, index, fraction = tables(starts)
    data = block(values, rows, columns, layout, SENTINEL)
    stride = data.shape[1]
    index_stride = stride + (3 if layout in ("padded", "odd") else 0)
    made = {"scratch": block(None, rows, columns, layout, np.nan),
            "index_rows": index_block(rows, index_stride),
            "index_scratch": index_block(rows, index_stride),
            "weight_rows": block(None, rows, columns, layout, SENTINEL),
            "weighted_rows": block(None, rows, columns, layout, SENTINEL),
            "weight_sums": plain(rows, intervals.size - 1),
            "weighted_sums": plain(rows, intervals.size - 1),
            "means": plain(rows, intervals.size - 1),
            "quantiles": plain(rows, bands*len(G_POINTS))}
    made = {name: tensor for name, tensor in made.items() if name not in leave_out}
    keywords = {name: Rows(tensor) for name, tensor in made.items()}
    if {"means", "weight_sums", "weighted_sums"} & set(made):
        keywords.update(interval_start=intervals)
    if "quantiles" in made:
        keywords.update(point_index=index, point_fraction=fraction)
    weight_row = None
    if weights is not None:
        weight_row = block(np.asarray(weights)[None, :], 1, columns, "exact", SENTINEL)
        keywords.update(weight_row=Rows(weight_row))
    else:
        keywords.update(row_temperature=temperatures, grid=grid)
    engine.order_after_stream(torch.cuda.current_stream("cuda:0").cuda_stream)
    engine.band_distribution_weighted(Rows(data), columns, starts, index_stride=index_stride,
                                      **keywords)
    engine.synchronize()
    host = data.cpu().numpy()
    assert np.all(host[:, columns:] == SENTINEL), "the padding of the rows was written"
    out = {"sorted": np.ascontiguousarray(host[:, :columns])}
    order = made["index_rows"].cpu().numpy()
    assert np.all(order[:, columns:] == INDEX_SENTINEL), "the padding of index_rows was written"
    out["index_rows"] = np.ascontiguousarray(order[:, :columns])
    for name in ("weight_rows", "weighted_rows"):
        if name in made:
            host = made[name].cpu().numpy()
            assert np.all(host[:, columns:] == SENTINEL), "the padding of %s was written" % name
            out[name] = np.ascontiguousarray(host[:, :columns])
    for name in ("weight_sums", "weighted_sums", "means"):
        if name in made:
            out[name] = wc.per_band(made[name].cpu().numpy(), bands, len(G_EDGES) - 1)
    if "quantiles" in made:
        out["quantiles"] = made["quantiles"].cpu().numpy().reshape(rows, bands, len(G_POINTS))
    return out


def run_plain(engine, values, starts):
    """lbl_band_distribution on a copy: {sorted, means, quantiles}."""
    import torch
    rows, columns = values.shape
    bands = starts.size - 1
    intervals, index, fraction = tables(starts)
    data = block(values, rows, columns, "aligned", SENTINEL)
    scratch = block(None, rows, columns, "aligned", np.nan)
    means, quantiles = plain(rows, intervals.size - 1), plain(rows, bands*len(G_POINTS))
    engine.order_after_stream(torch.cuda.current_stream("cuda:0").cuda_stream)
    engine.band_distribution(Rows(data), columns, starts, scratch=Rows(scratch),
                             interval_start=intervals, means=Rows(means), point_index=index,
                             point_fraction=fraction, quantiles=Rows(quantiles))
    engine.synchronize()
    return {"sorted": np.ascontiguousarray(data.cpu().numpy()[:, :columns]),
            "means": wc.per_band(means.cpu().numpy(), bands, len(G_EDGES) - 1),
            "quantiles": quantiles.cpu().numpy().reshape(rows, bands, len(G_POINTS))}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(a.view(U64 if a.dtype == F64 else a.dtype),
                       b.view(U64 if b.dtype == F64 else b.dtype))


def check_sums(what, name, got, terms, starts):
    """got [rows, bands, Q] against the long-double sums of `terms` [rows, columns] (float64 or
    long double), interval by interval, wherever every term is finite."""
    bands, q = starts.size - 1, len(G_EDGES) - 1
    exact, size = wc.interval_sums(terms, wc.flat_intervals(starts, G_EDGES))
    exact, size = wc.per_band(exact, bands, q), wc.per_band(size, bands, q)
    finite = np.isfinite(size)
    assert np.any(finite), what
    error = np.abs(got[finite].astype(LD) - exact[finite])
    allowed = cases.MEAN_BOUND*size[finite]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(error == 0, LD(0.), error/allowed)
    print("%s, %s: worst error / bound %.3g" % (what, name, float(np.max(ratio))))
    WORST[name] = max(WORST.get(name, 0.), float(np.max(ratio)))
    assert np.all(error <= allowed), (what, name)
    empty = per_band_empty(starts)
    assert np.all(got[:, empty] == 0.), (what, name, "an interval without columns is 0")


def per_band_empty(starts):
    counts = np.stack([np.diff(cases.interval_bounds(n, G_EDGES)) for n in np.diff(starts)])
    return counts == 0


def check(what, got, values, starts, weights, reference=None):
    """Everything a call with a weight row returns against the mirror."""
    order, ordered = wc.sorted_rows(values, starts)
    assert np.array_equal(got["index_rows"], order), (what, "pi")
    assert cases.same_bits(got["sorted"], ordered), (what, "sorted")
    assert cases.same_bits(got["sorted"], cases.sort_bands(values, starts)), (what, "sorted")
    w, wk = wc.gathered(order, ordered, starts, weights)
    assert cases.same_bits(got["weight_rows"], w), (what, "W")
    assert cases.same_bits_or_nan(got["weighted_rows"], wk), (what, "WK")
    w, wk = wc.gathered(order, ordered, starts, weights, fill=0.)
    check_sums(what, "weight sums", got["weight_sums"], w, starts)
    check_sums(what, "weighted sums", got["weighted_sums"], wk, starts)
    if reference is not None:
        for name in ("sorted", "means", "quantiles"):
            assert same_bits(got[name], reference[name]), (what, name, "lbl_band_distribution's")


def with_ends(band_values, rows):
    """The band's values with 5 unbanded sentinel columns before and 7 after: (values, starts)."""
    n = band_values.shape[1]
    values = np.full((rows, n + 12), SENTINEL)
    values[:, 5:5 + n] = band_values
    return values, np.array([5, 5 + n], dtype=np.int64)


def weights_of(columns, rng):
    """Finite weights >= 0, a tenth of them 0."""
    return np.where(rng.random(columns) < 0.1, 0., rng.lognormal(0., 2., columns))


@pytest.mark.parametrize("kind", wc.VALUE_KINDS)
def test_every_length_as_a_single_band(engine, kind):
    """Each length alone in a row, unbanded sentinel columns on both sides."""
    rng = np.random.default_rng(700 + wc.VALUE_KINDS.index(kind))
    for n in wc.LENGTHS:
        values, starts = with_ends(wc.values_of(kind, n, rng)[None, :], 1)
        weights = weights_of(values.shape[1], rng)
        got = run(engine, values, starts, weights)
        for name in ("sorted", "weight_rows", "weighted_rows"):
            assert np.all(got[name][:, :5] == SENTINEL) and np.all(got[name][:, 5 + n:] == SENTINEL)
        assert np.all(got["index_rows"][:, :5] == INDEX_SENTINEL)
        assert np.all(got["index_rows"][:, 5 + n:] == INDEX_SENTINEL)
        check((kind, n), got, values, starts, weights,
              run_plain(engine, values, starts) if n in (9, 4097, 3*4096 + 1) else None)


@pytest.mark.parametrize("kind", wc.VALUE_KINDS)
def test_packed_row_layouts_and_row_cuts(engine, kind):
    """Every length side by side in one row, unaligned starts, empty bands between and unbanded
    columns at both ends, three rows; padded and odd strides, a base 8 bytes off alignment and the
    rows cut over two calls give the bits of the aligned call, in every output."""
    rng = np.random.default_rng(800 + wc.VALUE_KINDS.index(kind))
    starts, columns, real = cases.packed_starts(wc.LENGTHS)
    assert np.count_nonzero(np.diff(starts) == 0) >= 5 and np.any(starts[real] % 2 == 1)
    values = np.full((3, columns), SENTINEL)
    for r in range(3):
        for b in real:
            values[r, starts[b]:starts[b + 1]] = wc.values_of(kind, starts[b + 1] - starts[b], rng)
    weights = weights_of(columns, rng)
    base = run(engine, values, starts, weights)
    for name in ("sorted", "weight_rows", "weighted_rows"):
        assert np.all(base[name][:, :5] == SENTINEL) and np.all(base[name][:, -7:] == SENTINEL)
    assert np.all(base["index_rows"][:, :5] == INDEX_SENTINEL)
    assert np.all(base["index_rows"][:, -7:] == INDEX_SENTINEL)
    check((kind, "packed"), base, values, starts, weights, run_plain(engine, values, starts))
    empty = np.diff(starts) == 0
    assert np.all(base["weight_sums"][:, empty] == 0.) and np.all(np.isnan(base["means"][:, empty]))
    cut = [run(engine, values[:1], starts, weights), run(engine, values[1:], starts, weights)]
    for key in base:
        joined = np.concatenate([part[key] for part in cut])
        assert same_bits(joined, base[key]), (kind, "rows cut over two calls", key)
    for layout in ("padded", "offset", "odd"):
        got = run(engine, values, starts, weights, layout=layout)
        for key in base:
            assert same_bits(got[key], base[key]), (kind, layout, key)


@pytest.mark.parametrize("kind", ["random", "plateau", "two values"])
def test_planck_weights_from_row_temperatures(engine, kind):
    """Row temperatures 180, 288 and 320 K on a grid whose first columns have nu <= 0."""
    rng = np.random.default_rng(900)
    starts, columns, real = cases.packed_starts([130, 4097, 6145, 2*4096 + 5])
    starts[0] = 0                                   # the columns with nu <= 0 lie in a band
    grid = -0.03 + 0.01*np.arange(columns) + np.where(np.arange(columns) > 4, 600., 0.)
    assert np.count_nonzero(grid <= 0.) == 4 and grid[4] > 0. and grid.max() < 1100.
    assert np.all(np.diff(grid) > 0.)
    handle = engine.load_grid(grid)
    temperatures = np.array(wc.PLANCK_TEMPERATURES)
    values = np.full((3, columns), SENTINEL)
    for r in range(3):
        for b in real:
            values[r, starts[b]:starts[b + 1]] = wc.values_of(kind, starts[b + 1] - starts[b], rng)
    try:
        base = run(engine, values, starts, temperatures=temperatures, grid=handle)
        cut = [run(engine, values[:2], starts, temperatures=temperatures[:2], grid=handle),
               run(engine, values[2:], starts, temperatures=temperatures[2:], grid=handle)]
        odd = run(engine, values, starts, temperatures=temperatures, grid=handle, layout="odd")
    finally:
        engine.free_grid(handle)
    order, ordered = wc.sorted_rows(values, starts)
    assert np.array_equal(base["index_rows"], order) and cases.same_bits(base["sorted"], ordered)
    exact = wc.planck_weights(LD, grid, temperatures)
    in_band = order != INDEX_SENTINEL
    w = np.zeros(values.shape, dtype=LD)
    for b in range(starts.size - 1):
        a, e = int(starts[b]), int(starts[b + 1])
        w[:, a:e] = np.take_along_axis(exact[:, a:e], order[:, a:e].astype(np.int64), axis=1)
    wk = w*np.where(in_band, ordered, 0.).astype(LD)
    got_w = base["weight_rows"]
    assert np.all(got_w[~in_band] == SENTINEL)
    assert np.all(got_w[in_band][w[in_band] == 0] == 0.) and np.any(w[in_band] == 0)
    error = np.abs(got_w[in_band].astype(LD) - w[in_band])
    WORST["planck W"] = float(np.max(error/np.maximum(PLANCK_BOUND*w[in_band], LD(1e-300))))
    assert np.all(error <= PLANCK_BOUND*w[in_band])
    assert cases.same_bits(base["weighted_rows"][in_band], (got_w*ordered)[in_band])
    check_sums((kind, "planck"), "planck weight sums", base["weight_sums"], w, starts)
    check_sums((kind, "planck"), "planck weighted sums", base["weighted_sums"], wk, starts)
    # a band's total weight does not depend on pi, and a warmer row weighs more
    totals = np.sum(base["weight_sums"], axis=-1)
    assert np.all(totals[2, real] > totals[1, real]) and np.all(totals[1, real] > totals[0, real])
    for key in base:
        assert same_bits(np.concatenate([part[key] for part in cut]), base[key]), (kind, key)
        assert same_bits(odd[key], base[key]), (kind, "odd", key)


def test_outputs_are_optional_and_short_bands_need_no_scratch(engine):
    rng = np.random.default_rng(11)
    values = rng.normal(0., 1., (2, 9000))
    starts = np.array([0, 4096, 4096, 8192, 9000], dtype=np.int64)
    weights = weights_of(9000, rng)
    full = run(engine, values, starts, weights, leave_out=("scratch", "index_scratch"))
    check("no scratch", full, values, starts, weights)
    alone = run(engine, values, starts, weights,
                leave_out=("scratch", "index_scratch", "weight_rows", "weighted_rows",
                           "weight_sums", "weighted_sums", "means", "quantiles"))
    assert set(alone) == {"sorted", "index_rows"}
    assert same_bits(alone["index_rows"], full["index_rows"])
    assert same_bits(alone["sorted"], full["sorted"])
    one = run(engine, values, starts, weights, leave_out=("weight_sums", "means", "quantiles"))
    assert same_bits(one["weighted_sums"], full["weighted_sums"])


def test_refused_calls_write_nothing(engine):
    import torch
    from pylbl_amd.errors import EngineError
    rng = np.random.default_rng(12)
    columns = 9000
    values = rng.normal(0., 1., (2, columns))
    tensors = {name: block(values if name == "values" else None, 2, columns, "aligned", SENTINEL)
               for name in ("values", "scratch", "weight_rows", "weighted_rows")}
    tensors.update(index_rows=index_block(2, columns), index_scratch=index_block(2, columns),
                   weight_row=block(np.ones((1, columns)), 1, columns, "aligned", SENTINEL),
                   sums=plain(2, 2), more=plain(2, 2))
    rows = {name: Rows(tensor) for name, tensor in tensors.items()}
    grid = engine.load_grid(600. + 0.01*np.arange(columns))
    short = engine.load_grid(600. + 0.01*np.arange(100))
    good = dict(band_start=[0, 5000, columns], index_rows=rows["index_rows"],
                scratch=rows["scratch"], index_scratch=rows["index_scratch"],
                index_stride=columns, weight_row=rows["weight_row"],
                weight_rows=rows["weight_rows"], weighted_rows=rows["weighted_rows"],
                interval_start=[0, 2500, columns], weight_sums=rows["sums"],
                weighted_sums=rows["more"])
    planck = dict(good, weight_row=None, row_temperature=[250., 260.], grid=grid)
    before = {name: tensor.cpu().numpy().copy() for name, tensor in tensors.items()}
    bad = [dict(good, scratch=None), dict(good, index_scratch=None),   # a band above 4096
           dict(good, band_start=[0, 10, 5]), dict(good, band_start=[0, columns + 1]),
           dict(good, band_start=[-1, 5]),
           dict(planck, grid=grid + 1000), dict(planck, grid=short),
           dict(planck, row_temperature=[250., 0.]), dict(planck, row_temperature=[np.nan, 250.]),
           dict(planck, row_temperature=[-1., 250.]),
           dict(good, index_stride=columns - 1),
           dict(good, weight_rows=None), dict(good, weighted_rows=None),
           dict(good, weight_rows=None, weighted_rows=None),            # sums without rows
           dict(good, interval_start=[0, 9, 3]),
           dict(good, scratch=rows["values"]), dict(good, weight_rows=rows["scratch"]),
           dict(good, weighted_rows=rows["weight_rows"]),
           dict(good, index_scratch=rows["index_rows"]),
           dict(good, weight_row=rows["weight_rows"])]
    try:
        for keywords in bad:
            with pytest.raises(EngineError):
                engine.band_distribution_weighted(rows["values"], columns, **keywords)
        # both weights or neither: refused by the binding already, as the entry would
        for keywords in (dict(good, weight_row=None),
                         dict(good, row_temperature=[250., 260.], grid=grid)):
            with pytest.raises(ValueError):
                engine.band_distribution_weighted(rows["values"], columns, **keywords)
        engine.synchronize()
        for name, tensor in tensors.items():
            assert np.array_equal(tensor.cpu().numpy(), before[name], equal_nan=True), name
        # ... and the engine stays usable: the good calls run.
        engine.order_after_stream(torch.cuda.current_stream("cuda:0").cuda_stream)
        engine.band_distribution_weighted(rows["values"], columns, **good)
        engine.synchronize()
        order, ordered = wc.sorted_rows(values, np.array([0, 5000, columns]))
        assert np.array_equal(tensors["index_rows"].cpu().numpy(), order)
        assert cases.same_bits(tensors["values"].cpu().numpy(), ordered)
    finally:
        engine.free_grid(grid)
        engine.free_grid(short)

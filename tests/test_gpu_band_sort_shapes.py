"""lbl_band_distribution fed directly (Engine.band_distribution on rows held in torch tensors), in
the style of test_gpu_sweep_shapes.py: every segment length of tests/kdistribution_cases.py (1..130,
around the powers of two up to 2^15, 3 2^k + 5, and 2^18 + 1 -- no, one and up to seven merge
passes, runs without a partner), as a single band and packed side by side into one row with empty
bands between and unbanded columns at both ends; random, equal, sorted, reversed and two-valued
values and a mix of duplicates, +-0, +-inf, denormals, negatives and NaN; 1 and 3 rows, a padded
row stride, a base 8 bytes off 16-byte alignment, sentinels in the padding and the unbanded columns.

Bounds, none from the code under test: the sorted rows are numpy's sort of the integer keys bit
for bit; quantiles are the numpy expression bit for bit (NaN where that is NaN: the payload of a
NaN made by inf - inf is the machine's own); interval means are within 1e-12 x the mean of |k| of
the long-double mean (finite inputs), and the counts times the means give the band's sum within the
same bound; layouts and repeated calls give identical bits."""
import numpy as np
import pytest

from tests import kdistribution_cases as cases
from tests.sweep_cases import LAYOUTS

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
SENTINEL = cases.SENTINEL
G_EDGES = np.array([0., 0.3, 0.30000000000000004, 0.55, 0.9, 1.])
G_POINTS = np.array([0., 0.013, 0.5, 0.77, 1.])
WORST = {}


class Rows(object):
    """A float64 torch tensor [rows, row stride] on the GPU, as the engine's blocks."""
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
    """[rows, stride] on the GPU in `layout`: `values` [rows, columns] (None: `fill`) in the first
    `columns` values of each row, `fill` in the padding."""
    import torch
    layout = LAYOUTS[layout]
    stride = layout.stride(columns)
    host = np.full((rows, stride), fill, dtype=F64)
    if values is not None:
        host[:, :columns] = values
    flat = torch.full((rows*stride + 2,), fill, dtype=torch.float64, device="cuda:0")
    view = flat[layout.offset:layout.offset + rows*stride].view(rows, stride)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 16 == 8*(layout.offset % 2)
    return view


def plain(rows, width):
    import torch
    return torch.full((rows, width), SENTINEL, dtype=torch.float64, device="cuda:0")


def tables(starts, g_edges=G_EDGES, g_points=G_POINTS):
    """(flat interval starts, point index, point fraction) of the bands, stated per band."""
    counts = np.diff(starts)
    intervals = np.concatenate([starts[b] + cases.interval_bounds(n, g_edges)
                                for b, n in enumerate(counts)]).astype(np.int64)
    index = np.full((counts.size, len(g_points)), -1, dtype=np.int64)
    fraction = np.zeros((counts.size, len(g_points)))
    for b, n in enumerate(counts):
        for p, g in enumerate(g_points):
            if n > 0:
                index[b, p], fraction[b, p] = cases.quantile_index(n, g)
    return intervals, index, fraction


WANT = ("scratch", "means", "quantiles")


def queue(engine, values, starts, layout="aligned", g_edges=G_EDGES, g_points=G_POINTS, want=WANT,
          asynchronous=False):
    """Queues one call on `values` [rows, columns] and returns its blocks for collect(): `want`
    names what the call is given beside the values -- scratch, means, quantiles."""
    import torch
    rows, columns = values.shape
    bands = starts.size - 1
    intervals, index, fraction = tables(starts, g_edges, g_points)
    call = {"columns": columns, "bands": bands, "q": len(g_edges) - 1, "p": len(g_points),
            "data": block(values, rows, columns, layout, SENTINEL)}
    keywords = {}
    if "scratch" in want:
        call["scratch"] = block(None, rows, columns, layout, np.nan)
        keywords.update(scratch=Rows(call["scratch"]))
    if "means" in want:
        call["means"] = plain(rows, intervals.size - 1)
        keywords.update(interval_start=intervals, means=Rows(call["means"]))
    if "quantiles" in want:
        call["quantiles"] = plain(rows, bands*len(g_points))
        keywords.update(point_index=index, point_fraction=fraction,
                        quantiles=Rows(call["quantiles"]))
    engine.order_after_stream(torch.cuda.current_stream("cuda:0").cuda_stream)
    engine.band_distribution(Rows(call["data"]), columns, starts, asynchronous=asynchronous,
                             **keywords)
    return call


def collect(call):
    """{sorted [rows, columns], means [rows, bands, Q], quantiles [rows, bands, P]} of a call of
    queue() that has run (those it was given); the padding of the rows is checked to come back
    untouched."""
    columns, bands, q = call["columns"], call["bands"], call["q"]
    host = call["data"].cpu().numpy()
    rows = host.shape[0]
    assert np.all(host[:, columns:] == SENTINEL), "the padding of the rows was written"
    out = {"sorted": np.ascontiguousarray(host[:, :columns])}
    if "means" in call:
        flat = np.full((rows, bands*(q + 1)), np.nan)
        flat[:, :-1] = call["means"].cpu().numpy()
        out["means"] = np.ascontiguousarray(flat.reshape(rows, bands, q + 1)[:, :, :q])
    if "quantiles" in call:
        out["quantiles"] = call["quantiles"].cpu().numpy().reshape(rows, bands, call["p"])
    return out


def run(engine, values, starts, layout="aligned", g_edges=G_EDGES, g_points=G_POINTS, want=WANT):
    """{sorted [rows, columns], means [rows, bands, Q], quantiles [rows, bands, P]} of one call;
    the padding of the rows is checked to come back untouched."""
    call = queue(engine, values, starts, layout, g_edges, g_points, want)
    engine.synchronize()
    return collect(call)


def check(what, got, values, starts, finite, g_edges=G_EDGES, g_points=G_POINTS, worst=None):
    """finite: the means are held to their bound (in every band whose values are all finite)."""
    worst = WORST if worst is None else worst
    expected = cases.sort_bands(values, starts)
    assert cases.same_bits(got["sorted"], expected), what
    for r in range(values.shape[0]):
        for b in range(starts.size - 1):
            band = expected[r, starts[b]:starts[b + 1]]
            assert cases.same_bits_or_nan(got["quantiles"][r, b], cases.quantiles(band, g_points)), \
                (what, r, b)
            if band.size == 0:
                assert np.all(np.isnan(got["means"][r, b])), (what, r, b)
            if not finite or band.size == 0 or not np.all(np.isfinite(band)):
                continue
            mean, magnitude = cases.interval_means(band, g_edges)
            empty = np.isnan(mean)
            assert np.array_equal(np.isnan(got["means"][r, b]), empty), (what, r, b)
            error = np.abs(got["means"][r, b][~empty].astype(LD) - mean[~empty])
            allowed = cases.MEAN_BOUND*magnitude[~empty]
            with np.errstate(invalid="ignore"):
                ratio = np.where(error == 0, LD(0.), error/allowed)    # (a band of zeros: 0/0)
            worst["means"] = max(worst.get("means", 0.), float(np.max(ratio)))
            assert np.all(error <= allowed), (what, r, b)
            # counts weighted by means give the band's sum
            counts = np.diff(cases.interval_bounds(band.size, g_edges))
            total = np.sum(counts[~empty].astype(LD)*got["means"][r, b][~empty].astype(LD))
            exact, size = np.sum(band.astype(LD)), LD(band.size)
            allowed = cases.MEAN_BOUND*np.sum(np.abs(band.astype(LD)))
            if abs(total - exact) > 0:
                worst["sums"] = max(worst.get("sums", 0.), float(abs(total - exact)/allowed))
            assert abs(total - exact) <= allowed and size > 0, (what, r, b)


def with_ends(band_values, rows):
    """The band's values with 5 unbanded sentinel columns before and 7 after: (values, starts)."""
    n = band_values.shape[1]
    values = np.full((rows, n + 12), SENTINEL)
    values[:, 5:5 + n] = band_values
    return values, np.array([5, 5 + n], dtype=np.int64)


@pytest.mark.parametrize("kind", cases.VALUE_KINDS)
def test_every_length_as_a_single_band(engine, kind):
    """Each length alone in a row, unbanded sentinel columns on both sides."""
    rng = np.random.default_rng(500 + cases.VALUE_KINDS.index(kind))
    for n in cases.LENGTHS:
        values, starts = with_ends(cases.values_of(kind, n, rng)[None, :], 1)
        got = run(engine, values, starts)
        assert np.all(got["sorted"][:, :5] == SENTINEL) and np.all(got["sorted"][:, 5 + n:] == SENTINEL)
        check((kind, n), got, values, starts, kind != "mix")
    print("worst error / bound so far:", WORST)


@pytest.mark.parametrize("kind", cases.VALUE_KINDS)
def test_packed_row_and_layouts(engine, kind):
    """Every length side by side in one row with empty bands between and unbanded columns at both
    ends; three rows in a padded stride and 8 bytes off alignment, and a repeated call, give the
    bits of the aligned call."""
    rng = np.random.default_rng(600 + cases.VALUE_KINDS.index(kind))
    starts, columns, real = cases.packed_starts(cases.LENGTHS)
    assert np.count_nonzero(np.diff(starts) == 0) >= 50 and len(real) == len(cases.LENGTHS)
    values = np.full((3, columns), SENTINEL)
    for r in range(3):
        for b in real:
            values[r, starts[b]:starts[b + 1]] = cases.values_of(kind, starts[b + 1] - starts[b], rng)
    base = run(engine, values, starts)
    assert np.all(base["sorted"][:, :5] == SENTINEL) and np.all(base["sorted"][:, -7:] == SENTINEL)
    check((kind, "packed"), base, values, starts, kind != "mix")
    empty = np.diff(starts) == 0
    assert np.all(np.isnan(base["means"][:, empty])) and np.all(np.isnan(base["quantiles"][:, empty]))
    one = run(engine, values[:1], starts)
    for layout in ("aligned", "padded", "offset", "odd"):
        got = run(engine, values, starts, layout)
        for key in base:
            assert cases.same_bits(got[key], base[key]), (kind, layout, key)
            assert cases.same_bits(one[key], base[key][:1]), (kind, "one row", key)
    print("worst error / bound so far:", WORST)


def test_short_bands_need_no_scratch_and_refusals(engine):
    """Bands up to 4096 columns sort without scratch; the entry's refusals launch nothing."""
    import torch
    from pylbl_amd.errors import EngineError
    rng = np.random.default_rng(7)
    values = rng.normal(0., 1., (2, 9000))
    starts = np.array([0, 4096, 4096, 8192, 9000], dtype=np.int64)
    data = block(values, 2, 9000, "aligned", SENTINEL)
    engine.order_after_stream(torch.cuda.current_stream("cuda:0").cuda_stream)
    engine.band_distribution(Rows(data), 9000, starts)
    engine.synchronize()
    assert cases.same_bits(data.cpu().numpy()[:, :9000], cases.sort_bands(values, starts))
    before = data.cpu().numpy()
    for bad in (dict(band_start=[0, 4097]),                         # needs scratch
                dict(band_start=[0, 10, 5]), dict(band_start=[0, 9001]), dict(band_start=[-1, 5]),
                dict(band_start=[0, 5], scratch=Rows(data)),
                dict(band_start=[0, 5], interval_start=[0, 9, 3], means=Rows(plain(2, 2)))):
        with pytest.raises(EngineError):
            engine.band_distribution(Rows(data), 9000, **bad)
    engine.synchronize()
    assert cases.same_bits(data.cpu().numpy(), before)

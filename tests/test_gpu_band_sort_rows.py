"""lbl_band_distribution beyond the shapes of test_gpu_band_sort_shapes.py (whose helpers this
file uses): more rows than one launch holds (65 535 + 2, short bands and one merged band of 4097
columns), every choice of outputs (sort alone, means alone, quantiles alone, all), Q = 1 and 64,
P = 1 and 3, bands x points around the quantile kernel's block of 256, the lengths of
cases.EXTRA_LENGTHS (partner runs around one tile, three runs, an unpaired run of several tiles
that a later pass merges), inputs made for merge path's splits (cases.MERGE_KINDS: a perfect
interleave, a plateau of equal bits and one of -0 / +0 across runs 0 and 1, blocks in reverse
order), and two asynchronous calls with different tables queued without a wait between them.

Bounds, none from the code under test: sorted rows are numpy's sort of the integer keys bit for
bit (torch.sort for the 65 537 x 4097 block: on positive finite values equal values have equal
bits, so that sort is unique too); quantiles are the numpy expression bit for bit; interval means
are within 1e-12 x the mean of |k| of the long-double mean wherever the band is finite."""
import time

import numpy as np
import pytest

from tests import kdistribution_cases as cases
from tests.test_gpu_band_sort_shapes import (G_EDGES, G_POINTS, Rows, check, collect, plain, queue,
                                             run, tables, with_ends)

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
SENTINEL = cases.SENTINEL
GRID_Y = 65535                      # rows per launch: the grid's y limit
WORST = {}
NAMED = (GRID_Y - 1, GRID_Y, GRID_Y + 1)


@pytest.fixture(scope="module")
def engine():
    from pylbl_amd.engine import default_engine
    yield default_engine(0)
    for what, ratio in sorted(WORST.items()):
        print("\nworst error / bound, rows file, %s: %.3g" % (what, ratio))


def first_bad(ok):
    """The rows (up to five) where `ok` [rows] or [rows, ...] does not hold."""
    ok = np.asarray(ok).reshape(len(ok), -1).all(axis=1)
    return np.flatnonzero(~ok)[:5].tolist()


def bits_equal(a, b):
    return np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)


def bits_or_nan(got, expected):
    nan = np.isnan(expected)
    return np.where(nan, np.isnan(got), bits_equal(got, expected))


def check_rows(what, got, values, starts, held, rows=None):
    """check() for many rows of short bands, with the oracles that take all rows at once; `rows`
    are named in the messages first.  held [rows]: the rows whose means are held to the bound,
    as check()'s `finite` -- not those of the "mix" pool, whose zeros and denormals have means
    that fp64 does not hold to 1e-12 of their size."""
    expected = cases.sort_band_rows(values, starts)
    ok = {"sorted": bits_equal(got["sorted"], expected).all(axis=1)}
    quantile_ok, mean_ok = [], []
    for b in range(starts.size - 1):
        band = expected[:, starts[b]:starts[b + 1]]
        quantile_ok.append(bits_or_nan(got["quantiles"][:, b], cases.quantile_rows(band, G_POINTS))
                           .all(axis=1))
        if band.shape[1] == 0:
            mean_ok.append(np.isnan(got["means"][:, b]).all(axis=1))
            continue
        finite = held & np.isfinite(band).all(axis=1)
        mean, magnitude = cases.interval_mean_rows(band[finite], G_EDGES)
        mine = got["means"][finite, b]
        empty = np.isnan(mean)
        with np.errstate(invalid="ignore"):
            error = np.abs(mine.astype(LD) - mean)
            allowed = cases.MEAN_BOUND*magnitude
            good = np.where(empty, np.isnan(mine), error <= allowed)
            ratio = np.where(empty | (error == 0), LD(0.), error/allowed)   # (zeros: 0/0)
            WORST["means"] = max(WORST.get("means", 0.), float(np.max(ratio, initial=0.)))
        here = np.ones(values.shape[0], dtype=bool)
        here[finite] = good.all(axis=1)
        mean_ok.append(here)
    ok["quantiles"] = np.all(quantile_ok, axis=0)
    ok["means"] = np.all(mean_ok, axis=0)
    for r in rows or ():
        for name, flags in ok.items():
            assert flags[r], "%s: row %d, %s" % (what, r, name)
    for name, flags in ok.items():
        assert flags.all(), "%s: %s, rows %s" % (what, name, first_bad(flags))


def test_rows_beyond_one_launch_short(engine):
    """65 535 + 2 rows of 24 columns: bands of 1, 9, 0 and 8 columns between unbanded sentinel
    columns; lognormal rows, every third one from the "mix" pool.  Every row against the oracle;
    the rows on both sides of the launch boundary by name."""
    rng = np.random.default_rng(65535)
    rows, columns = GRID_Y + 2, 24
    starts = np.array([3, 4, 13, 13, 21], dtype=np.int64)
    values = rng.lognormal(-8., 3., (rows, columns))
    mixed = np.arange(rows) % 3 == 2
    assert mixed[NAMED[0]] and not mixed[NAMED[1]] and not mixed[NAMED[2]]
    values[mixed] = cases.values_of("mix", int(mixed.sum())*columns, rng).reshape(-1, columns)
    values[:, :3] = SENTINEL
    values[:, 21:] = SENTINEL
    got = run(engine, values, starts)
    outside = np.concatenate([got["sorted"][:, :3], got["sorted"][:, 21:]], axis=1)
    assert np.all(outside == SENTINEL), first_bad(outside == SENTINEL)
    check_rows("short rows", got, values, starts, ~mixed, NAMED)
    # a padded stride: the same bits
    padded = run(engine, values, starts, "padded")
    for key in got:
        same = bits_or_nan(padded[key], got[key])
        assert same.all(), (key, first_bad(same))


def test_rows_beyond_one_launch_merged(engine):
    """65 535 + 2 rows, one band of 4097 columns in a stride of 4098: one merge pass, so the
    result comes back from the scratch block.  Positive finite values made on the device in slices
    of 8192 rows, each from its own seed, made again after the call and put through torch.sort:
    every row bit for bit.  Ten rows also against the numpy oracle with quantiles and means."""
    import torch
    rows, columns, stride, step = GRID_Y + 2, 4097, 4098, 8192
    starts = np.array([0, columns], dtype=np.int64)
    device = "cuda:0"

    def made(first):
        generator = torch.Generator(device=device).manual_seed(4097 + first)
        count = min(step, rows - first)
        # (0, 1] scaled: positive, finite, no zero
        return (1. - torch.rand((count, columns), dtype=torch.float64, device=device,
                                generator=generator))*3.5e-4

    data = torch.full((rows, stride), SENTINEL, dtype=torch.float64, device=device)
    scratch = torch.full((rows, stride), np.nan, dtype=torch.float64, device=device)
    for first in range(0, rows, step):
        data[first:first + step, :columns] = made(first)
    rng = np.random.default_rng(4097)
    sample = sorted({0, 1} | set(NAMED) | set(rng.choice(rows, 5, replace=False).tolist()))
    before = data[sample].cpu().numpy()
    assert np.all(before[:, :columns] > 0.) and np.all(np.isfinite(before))
    intervals, index, fraction = tables(starts)
    means, quantiles = plain(rows, intervals.size - 1), plain(rows, G_POINTS.size)
    torch.cuda.synchronize()
    started = time.perf_counter()
    engine.order_after_stream(torch.cuda.current_stream(device).cuda_stream)
    engine.band_distribution(Rows(data), columns, starts, scratch=Rows(scratch),
                             interval_start=intervals, means=Rows(means), point_index=index,
                             point_fraction=fraction, quantiles=Rows(quantiles))
    engine.synchronize()
    print("\n65 537 x 4097 sorted, means and quantiles: %.3f s" % (time.perf_counter() - started))
    del scratch
    assert bool(torch.all(data[:, columns:] == SENTINEL)), "the padding of the rows was written"
    for first in range(0, rows, step):
        expected = torch.sort(made(first), dim=1).values
        got = data[first:first + step, :columns]
        if not torch.equal(got, expected):
            bad = torch.nonzero(torch.any(got != expected, dim=1)).flatten()[:5] + first
            raise AssertionError("sorted rows %s differ from torch.sort" % bad.tolist())
        del expected
    # g = 0 and g = 1 are the row's least and greatest value, in every row
    assert G_POINTS[0] == 0. and G_POINTS[-1] == 1.
    assert torch.equal(quantiles[:, 0], data[:, 0]) and \
        torch.equal(quantiles[:, -1], data[:, columns - 1])
    after = data[sample].cpu().numpy()
    got = {"sorted": after[:, :columns],
           "means": means[sample].cpu().numpy().reshape(len(sample), 1, -1),
           "quantiles": quantiles[sample].cpu().numpy().reshape(len(sample), 1, -1)}
    del data, means, quantiles
    torch.cuda.empty_cache()
    for i, r in enumerate(sample):
        one = {key: value[i:i + 1] for key, value in got.items()}
        check("row %d of 65 537 x 4097" % r, one, before[i:i + 1, :columns], starts, True,
              worst=WORST)


def banded_row(bands, rng):
    """One row of `bands` bands: cases.EXTRA_LENGTHS and 1, 2, 4096, 4097 columns, a band of
    [-inf, 1, +inf], empty bands and short ones up to the count: (values [1, columns], starts)."""
    lengths = cases.EXTRA_LENGTHS + [1, 2, 4096, 4097, 3]
    lengths += [0 if i % 5 == 4 else 1 + i % 7 for i in range(bands - len(lengths))]
    assert len(lengths) == bands
    starts = 5 + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    values = np.full((1, starts[-1] + 7), SENTINEL)
    values[0, starts[0]:starts[-1]] = rng.lognormal(-8., 3., starts[-1] - starts[0])
    special = lengths.index(3)
    values[0, starts[special]:starts[special + 1]] = [np.inf, -np.inf, 1.]
    return values, starts, lengths


@pytest.mark.parametrize("q", [1, 64])
@pytest.mark.parametrize("points, bands", [(1, 255), (1, 256), (1, 257), (3, 85), (3, 86)])
def test_requested_outputs(engine, q, points, bands):
    """Sort alone (with scratch), means alone, quantiles alone and all three: what is there has
    the bits of the call for all three, which is held to the oracle.  bands x points = 255, 256,
    257 and 258 around the quantile kernel's block of 256."""
    rng = np.random.default_rng(1000*q + 10*bands + points)
    g_edges = cases.gauss_edges(q)
    g_points = np.array([0.5]) if points == 1 else np.array([0., 0.5, 1.])
    values, starts, lengths = banded_row(bands, rng)
    assert bands*points in (255, 256, 257, 258) and starts.size - 1 == bands
    whole = run(engine, values, starts, g_edges=g_edges, g_points=g_points)
    assert set(whole) == {"sorted", "means", "quantiles"}
    check((q, points, bands), whole, values, starts, True, g_edges, g_points, worst=WORST)
    one = lengths.index(1)
    value = values[0, starts[one]]
    assert cases.same_bits(whole["quantiles"][0, one], np.full(points, value))
    assert abs(LD(whole["means"][0, one, 0]) - LD(value)) <= cases.MEAN_BOUND*abs(LD(value))
    assert np.all(np.isnan(whole["means"][0, one, 1:]))       # only the first interval has one
    special = lengths.index(3)
    assert np.isnan(whole["quantiles"][0, special, 0])
    assert np.isnan(cases.quantiles(np.array([-np.inf, 1., np.inf]), g_points)[0])
    for want in (("scratch",), ("scratch", "means"), ("scratch", "quantiles")):
        part = run(engine, values, starts, g_edges=g_edges, g_points=g_points, want=want)
        assert set(part) == {"sorted"} | set(want[1:])
        for key in part:
            same = bits_or_nan(part[key], whole[key])
            assert same.all(), (want, key, np.argwhere(~same)[:5].tolist())
            if key == "sorted":
                assert cases.same_bits(part[key], whole[key]), want


MERGE_LENGTHS = cases.EXTRA_LENGTHS + [8192, 2**15 + 1]
MERGE_CASES = [(kind, False) for kind in cases.MERGE_KINDS] + [("plateau", True)]


@pytest.mark.parametrize("kind, signed_zeros", MERGE_CASES)
def test_merge_kinds(engine, kind, signed_zeros):
    """The inputs made for merge path's splits, a single band of every length, 1 and 3 rows,
    aligned and in an odd stride."""
    rng = np.random.default_rng(900 + MERGE_CASES.index((kind, signed_zeros)))
    for n in MERGE_LENGTHS:
        for rows in (1, 3):
            band = np.stack([cases.merge_values_of(kind, n, rng, signed_zeros=signed_zeros)
                             for _ in range(rows)])
            values, starts = with_ends(band, rows)
            base = None
            for layout in ("aligned", "odd"):
                got = run(engine, values, starts, layout)
                what = (kind, signed_zeros, n, rows, layout)
                assert np.all(got["sorted"][:, :5] == SENTINEL), what
                assert np.all(got["sorted"][:, 5 + n:] == SENTINEL), what
                check(what, got, values, starts, True, worst=WORST)
                if signed_zeros:
                    lo, hi = cases.plateau_bounds(n)
                    zeros = got["sorted"][:, 5 + lo:5 + hi]
                    half = (hi - lo)//2
                    assert np.all(zeros == 0.) and np.all(np.signbit(zeros[:, :half])) and \
                        not np.any(np.signbit(zeros[:, half:])), what
                if base is not None:
                    for key in got:
                        assert cases.same_bits(got[key], base[key]), (what, key)
                base = got


@pytest.mark.parametrize("kind", cases.VALUE_KINDS)
def test_extra_lengths_every_kind(engine, kind):
    """cases.EXTRA_LENGTHS, each alone in a row, for every kind of values."""
    rng = np.random.default_rng(700 + cases.VALUE_KINDS.index(kind))
    for n in cases.EXTRA_LENGTHS:
        values, starts = with_ends(cases.values_of(kind, n, rng)[None, :], 1)
        got = run(engine, values, starts)
        assert np.all(got["sorted"][:, :5] == SENTINEL) and np.all(got["sorted"][:, 5 + n:] == SENTINEL)
        check((kind, n), got, values, starts, kind != "mix", worst=WORST)


def test_two_async_calls_with_different_tables():
    """Two calls with different tables queued asynchronously on a new engine without a wait
    between them: 3 bands and 2 points, then 200 bands and 5 points, whose tables need a larger
    block than the first call's -- the first call's tables must outlive the reallocation.  Both
    match the oracle and the same calls made with a wait."""
    from pylbl_amd.engine import Engine
    rng = np.random.default_rng(31)
    engine = Engine(0)
    try:
        few = np.array([2, 6147, 6148, 6500], dtype=np.int64)          # 6145, 1, 352 columns
        lengths = [4097 if i == 150 else (0 if i % 9 == 8 else 1 + (37*i) % 61)
                   for i in range(200)]
        many = 3 + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        cases_ = [(few, cases.gauss_edges(3), np.array([0.25, 1.])),
                  (many, G_EDGES, G_POINTS)]
        words = [sum(x.size for x in tables(starts, g_edges, g_points))
                 for starts, g_edges, g_points in cases_]
        assert words[1] > 4*words[0]
        values = []
        for starts, _, _ in cases_:
            row = np.full((2, starts[-1] + 4), SENTINEL)
            row[:, starts[0]:starts[-1]] = rng.lognormal(-8., 3., (2, starts[-1] - starts[0]))
            values.append(row)
        calls = [queue(engine, v, starts, "aligned", g_edges, g_points, asynchronous=True)
                 for v, (starts, g_edges, g_points) in zip(values, cases_)]
        engine.synchronize()
        for call, v, (starts, g_edges, g_points) in zip(calls, values, cases_):
            got = collect(call)
            check(("async", starts.size - 1), got, v, starts, True, g_edges, g_points, worst=WORST)
            waited = run(engine, v, starts, "aligned", g_edges, g_points)
            for key in got:
                assert cases.same_bits(got[key], waited[key]), (starts.size - 1, key)
    finally:
        engine.close()

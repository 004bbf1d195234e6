"""Cases and plain-numpy oracles of the k-distribution tests (lbl_band_distribution,
Spectroscopy.compute_kdistribution): nothing here is imported from pylbl_amd.

The order: with u the 64 bits of a value, key = u ^ 2^63 for a clear sign bit, ~u for a set one,
keys compared as unsigned integers.  The oracle sorts the keys with numpy.sort and maps them back,
so the expected rows are unique bit for bit."""
import numpy as np

F64, LD, U64 = np.float64, np.longdouble, np.uint64
SIGN = U64(1) << U64(63)
SENTINEL = -12345.678
MEAN_BOUND = LD(1e-12)      # x mean |k|: the bound the project holds its band means to

# Segment lengths: every N in 1..130, then around the powers of two and 3 2^k + 5 for k = 7..15.
SMALL_LENGTHS = list(range(1, 131))
LARGE_LENGTHS = [n for k in range(7, 16) for n in (2**k - 1, 2**k, 2**k + 1, 3*2**k + 5)]
# 3 2^15 + 5 values are only four chunks of 32 768 (two passes): one longer segment, nine such
# chunks, so that every chunk size of CHUNKS meets four passes and a run without a partner.
LARGE_LENGTHS.append(2**18 + 1)
LENGTHS = SMALL_LENGTHS + LARGE_LENGTHS
VALUE_KINDS = ("random", "equal", "sorted", "reversed", "two values", "mix")
FINITE_KINDS = VALUE_KINDS[:5]
HOST_LENGTHS = (0, 1, 2, 3, 16, 17, 10001)
CHUNKS = [2**k for k in range(7, 16)]       # every power-of-two chunk from 128 to 32 768


def keys(values):
    u = np.ascontiguousarray(values, dtype=F64).view(U64)
    return np.where(u & SIGN != 0, ~u, u ^ SIGN)


def from_keys(k):
    k = np.ascontiguousarray(k, dtype=U64)
    return np.where(k & SIGN != 0, k ^ SIGN, ~k).astype(U64).view(F64)


def key_sort(values):
    """A 1-d array sorted ascending by the integer key: the same bits, permuted."""
    return from_keys(np.sort(keys(values)))


def sort_bands(rows, starts):
    """[rows, columns] with every band of every row sorted by the key; other columns as they are."""
    out = np.array(rows, dtype=F64)
    for r in range(out.shape[0]):
        for b in range(len(starts) - 1):
            out[r, starts[b]:starts[b + 1]] = key_sort(out[r, starts[b]:starts[b + 1]])
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F64), np.ascontiguousarray(b, dtype=F64)
    return a.shape == b.shape and np.array_equal(a.view(U64), b.view(U64))


def same_bits_or_nan(got, expected):
    """The same bits wherever the expected value is a number or an infinity, NaN where it is NaN
    (the payload of a NaN that arithmetic makes, inf - inf or 0*inf, is the machine's own)."""
    got, expected = np.asarray(got, dtype=F64), np.asarray(expected, dtype=F64)
    nan = np.isnan(expected)
    return got.shape == expected.shape and np.array_equal(np.isnan(got), nan) and \
        same_bits(got[~nan], expected[~nan])


def gauss_edges(count):
    _, w = np.polynomial.legendre.leggauss(count)
    edges = np.concatenate([[0.], np.cumsum(w/2.)])
    edges[-1] = 1.
    return edges


def gauss_points(count):
    x, _ = np.polynomial.legendre.leggauss(count)
    return (x + 1.)/2.


def interval_bounds(n, g_edges):
    """[Q + 1] sample bounds of a band of n points, one edge at a time: ceil(G n) in fp64."""
    return np.array([int(np.ceil(F64(g)*F64(n))) for g in g_edges], dtype=np.int64)


def quantile_index(n, g):
    """(i, f) of one g point of a band of n >= 1 points, the issue's statement."""
    x = min(max(F64(g)*F64(n) - F64(0.5), F64(0.)), F64(n - 1))
    i = int(np.floor(x))
    return i, F64(x) - F64(i)


def quantiles(sorted_band, g_points):
    """k_i + f*(k_min(i+1, N-1) - k_i) at every g point; NaN for an empty band."""
    n = sorted_band.size
    out = np.full(len(g_points), np.nan)
    if n == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        for p, g in enumerate(g_points):
            i, f = quantile_index(n, g)
            k = sorted_band[i]
            out[p] = k + f*(sorted_band[min(i + 1, n - 1)] - k)
    return out


def interval_means(sorted_band, g_edges):
    """(long-double mean, long-double mean of |k|) per interval; NaN for one without samples."""
    bounds = interval_bounds(sorted_band.size, g_edges)
    mean = np.full(len(g_edges) - 1, np.nan, dtype=LD)
    magnitude = np.full(len(g_edges) - 1, np.nan, dtype=LD)
    for q in range(len(g_edges) - 1):
        part = sorted_band[bounds[q]:bounds[q + 1]].astype(LD)
        if part.size:
            mean[q] = np.sum(part)/LD(part.size)
            magnitude[q] = np.sum(np.abs(part))/LD(part.size)
    return mean, magnitude


def merge_passes(n, chunk):
    """Merge passes a segment of n values takes after chunks of `chunk` are sorted."""
    runs, passes = -(-n//chunk), 0
    while runs > 1:
        runs, passes = -(-runs//2), passes + 1
    return passes


def unpaired_passes(n, chunk):
    """How many of those passes meet an odd number (> 1) of runs: a last run without a partner."""
    runs, found = -(-n//chunk), 0
    while runs > 1:
        found += runs % 2
        runs = -(-runs//2)
    return found


def values_of(kind, n, rng):
    """n float64 values of a kind."""
    if kind == "random":
        return rng.lognormal(-8., 3., n)
    if kind == "equal":
        return np.full(n, 3.25e-7)
    if kind == "sorted":
        return np.sort(rng.lognormal(-8., 3., n))
    if kind == "reversed":
        return np.sort(rng.lognormal(-8., 3., n))[::-1].copy()
    if kind == "two values":
        return np.where(rng.random(n) < 0.5, 1.5e-3, 2.5e-9)
    assert kind == "mix"
    pool = np.array([0., -0., np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, 1e-310, -1e-310, -1., 1.,
                     -3.5e7, 3.5e7, 1e-30, 1e-30, 7.25, 7.25, 7.25], dtype=F64)
    nan = np.array([0x7FF8000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF],
                   dtype=U64).view(F64)
    out = rng.choice(np.concatenate([pool, nan, rng.normal(0., 1., 8)]), n)
    return np.ascontiguousarray(out, dtype=F64)


def packed_starts(lengths):
    """Band starts of the lengths side by side in one row, an empty band after every third and
    unbanded columns at both ends: (starts [B + 1], columns, indices of the real bands).  Every
    second gap between bands is closed by a band of no columns, so the starts stay one list."""
    starts, at, real = [5], 5, []
    for i, n in enumerate(lengths):
        real.append(len(starts) - 1)
        at += n
        starts.append(at)
        if i % 3 == 2:
            starts.append(at)           # an empty band
    return np.array(starts, dtype=np.int64), at + 7, real
